"""The RESCAL sides step: N object-side and NS subject-side negatives per
positive and L2 (gamma_e, gamma_r) on the positive's rows, through every
layer: the per-triple kernel and its CPU twin, the grouped MFMA path, the host
checks of both bindings, and Rescal.train_batch.

Numerical checks follow tests/test_kernel_reference.py: one half of one output
at a time against the fp64 reference of tests/rescal_sides_refs.py,
err = max|got - ref64| / max|ref64| <= 16 * max(e32, 2^-23) with e32 the same
error of the reference evaluated in fp32 (step_refs.assert_half_close, which
prints a RATIO line per half). Outputs are prefilled with NaN and followed by a
sentinel row. Inputs are those of test_kernel_reference.rescal_case:
embeddings scaled 0.3, R scaled 0.1, accumulators U(0, 0.1).

Largest err / max(e32, 2^-23) observed per family (bound: 16):

    family                          CPU twin   MI355X
    rescal_step_sides                 2.66      5.18
    rescal_step_sides_grouped           -       2.24
    rescal_model_sides                1.00      0.87

The model cases name 8 * (2 + 2 + 2) = 48 different entities, so their store
has 56 of them (48 and the spare rows that must not change), not 40.
"""
import functools

import numpy as np
import pytest
import torch

import rescal_sides_refs as rsr
import step_refs as sr
from adapm_amd import _C

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda:0", id="gpu", marks=pytest.mark.gpu)]
GPU = pytest.mark.gpu

LR, EPS = 0.05, 1e-6
GE, GR = 0.01, 0.02  # distinct, so that a swap between the two shows
ROLES = ("s", "r", "o", "neg_o", "neg_s")


def _fam(name, device):
    return f"{name}[{'cpu' if device == 'cpu' else 'gpu'}]"


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _rows(g, n, L, scale=0.3, acc=0.1):
    """[n][2L] store rows: N(0, scale^2) embeddings | U(0, acc) accumulators."""
    a = torch.rand(n, L, generator=g) * acc if acc else torch.zeros(n, L)
    return torch.cat([torch.randn(n, L, generator=g) * scale, a], dim=1)


def _inputs(g, B, G, N, NS, D, acc=0.1):
    """(s, r, o, neg_o, neg_s) with G relation rows."""
    s, o, neg_o, neg_s = (_rows(g, n, D, acc=acc) for n in (B, B, B * N, B * NS))
    r = _rows(g, G, D * D, scale=0.1, acc=acc)
    return s, r, o, neg_o, neg_s


def _refs(ins, N, NS, D, ge=GE, gr=GR):
    return tuple(rsr.rescal_sides_ref(*ins, N, NS, D, LR, EPS, ge, gr, dt)
                 for dt in (torch.float64, torch.float32))


# A case is built once (inputs, fp64 and fp32 reference) and shared by the CPU
# and GPU twins of a test; nothing modifies it afterwards.
@functools.lru_cache(maxsize=4)
def sides_case(B, N, NS, D, fresh=False):
    g = torch.Generator().manual_seed(21000 + D + 7 * N + 13 * NS)
    ins = _inputs(g, B, B, N, NS, D, acc=0.0 if fresh else 0.1)
    return (ins,) + _refs(ins, N, NS, D)


def _call_sides(device, ins, B, N, NS, D, ge=GE, gr=GR):
    """_C.rescal_step_sides on guarded outputs -> ({role: out, "loss": out}, guards)."""
    bufs = {n: sr.Guarded(t.shape[0], t.shape[1], device) for n, t in zip(ROLES, ins)}
    loss = sr.guarded_vec(B, device)
    _C.rescal_step_sides(*[t.to(device) for t in ins], *[b.out for b in bufs.values()], loss.out,
                         N, NS, D, LR, EPS, ge, gr)
    _sync(device)
    got = {n: b.out for n, b in bufs.items()}
    got["loss"] = loss.out
    return got, {**bufs, "loss": loss}


def _check_guards(guards, what):
    for n, b in guards.items():
        b.check(f"{what} {n}")


def run_sides(device, B, N, NS, D, fresh=False):
    ins, ref64, ref32 = sides_case(B, N, NS, D, fresh)
    what = f"rescal sides B={B} N={N} NS={NS} D={D}{' fresh' if fresh else ''}"
    got, guards = _call_sides(device, ins, B, N, NS, D)
    sr.assert_step_close(got, ref64, ref32, what, _fam("rescal_step_sides", device))
    _check_guards(guards, what)


# ------------------------------------------------------------ 1. per-triple step

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [1, 5, 64, 65, 128, 196])
def test_sides_step_dims(device, D):
    """The thread-loop edges (KT = 256 threads, 64-lane waves) and the limit
    D = 196, where R and the six D-vectors take 158,384 B of LDS."""
    run_sides(device, 3, 2, 2, D)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("N,NS", [(0, 0), (0, 3), (3, 0), (1, 2)])
def test_sides_step_negatives(device, N, NS):
    run_sides(device, 3, N, NS, 65)


@pytest.mark.parametrize("device", DEVICES)
def test_sides_step_fresh_rows(device):
    """Accumulators 0."""
    run_sides(device, 3, 2, 2, 5, fresh=True)


@pytest.mark.parametrize("device", DEVICES)
def test_sides_step_grid_stride(device):
    """More samples than the launch has workgroups (cap 8192)."""
    run_sides(device, 8200, 1, 1, 4)


def _scaled_positive(seed, B, D, target):
    """N = NS = 0 inputs whose positive o is rescaled (psi is linear in it)
    so that psi_0 = target."""
    g = torch.Generator().manual_seed(seed)
    s, r, o, neg_o, neg_s = _inputs(g, B, B, 0, 0, D)
    psi = _refs((s, r, o, neg_o, neg_s), 0, 0, D)[0]["psi"][:, 0]
    o[:, :D] *= (target / psi).float()[:, None]
    return s, r, o, neg_o, neg_s


@pytest.mark.parametrize("device", DEVICES)
def test_sides_step_large_psi_loss(device):
    """psi_0 = 30 and no negatives: the whole loss of a sample is
    log1p(exp(-30)) = 9.4e-14, which 1 + exp(x) in fp32 rounds away."""
    B, D = 2, 65
    ins = _scaled_positive(22000, B, D, 30.0)
    ref64, ref32 = _refs(ins, 0, 0, D)
    assert ((ref64["psi"][:, 0] - 30.0).abs() < 1e-3).all()
    assert ((ref64["loss"] > 9.3e-14) & (ref64["loss"] < 9.5e-14)).all()
    got, guards = _call_sides(device, ins, B, 0, 0, D)
    assert (got["loss"].cpu() != 0).all(), f"loss {got['loss'].cpu().tolist()} reads 0"
    sr.assert_step_close(got, ref64, ref32, "rescal sides psi=30",
                         _fam("rescal_step_sides", device))
    _check_guards(guards, "psi=30")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [5, 65])
def test_sides_reduces_to_the_one_sided_step(device, D):
    """NS = 0 and both gammas 0: the same bits as rescal_step."""
    B, N = 4, 3
    g = torch.Generator().manual_seed(23000 + D)
    s, r, o, neg, none = (t.to(device) for t in _inputs(g, B, B, N, 0, D))
    want = [torch.full_like(t, float("nan")) for t in (s, r, o, neg)]
    want_loss = torch.full((B,), float("nan"), device=device)
    _C.rescal_step(s, r, o, neg, *want, want_loss, N, D, LR, EPS)
    got = [torch.full_like(t, float("nan")) for t in (s, r, o, neg)]
    got_loss = torch.full((B,), float("nan"), device=device)
    _C.rescal_step_sides(s, r, o, neg, none, *got, torch.empty_like(none), got_loss, N, 0, D,
                         LR, EPS, 0.0, 0.0)
    _sync(device)
    for name, a, b in zip(("ds", "drl", "do", "dneg"), got, want):
        assert not torch.isnan(b).any()
        assert torch.equal(a, b), f"{name}: max diff {(a - b).abs().max().item():g}"
    assert torch.equal(got_loss, want_loss)


@pytest.mark.parametrize("device", DEVICES)
def test_sides_regulariser_alone_moves_the_positive(device):
    """N = NS = 0 and psi_0 = 85: the logistic gradient is sigmoid(-85), about
    1e-37, so s, o and R take the AdaGrad step of gamma * row and nothing else.
    (psi_0 = -85 would not do: there the gradient is -1.)"""
    B, D = 2, 65
    ins = _scaled_positive(24000, B, D, 85.0)
    psi = _refs(ins, 0, 0, D)[0]["psi"][:, 0]
    assert (psi > 80).all()
    got, guards = _call_sides(device, ins, B, 0, 0, D)
    for name, rows, gamma, L in (("s", ins[0], GE, D), ("r", ins[1], GR, D * D),
                                 ("o", ins[2], GE, D)):
        reg = [sr.adagrad_halves(sr._f32(gamma) * rows[:, :L].to(dt), rows[:, L:].to(dt),
                                 sr._f32(LR), sr._f32(EPS))
               for dt in (torch.float64, torch.float32)]
        out = got[name].cpu()
        for half, part in ((0, "delta"), (1, "g2")):
            assert reg[0][half].abs().min() > 0
            sr.assert_half_close(out[:, half * L:(half + 1) * L], reg[0][half], reg[1][half],
                                 f"regulariser alone {name}.{part}",
                                 _fam("rescal_step_sides", device))
    assert torch.isfinite(got["loss"]).all()
    _check_guards(guards, "regulariser alone")


# ------------------------------------------------------------ 2. grouped step

@functools.lru_cache(maxsize=2)
def grouped_case(sizes, N, NS, D):
    starts = np.cumsum((0,) + sizes).astype(np.int32)
    B, G = int(starts[-1]), len(sizes)
    g = torch.Generator().manual_seed(25000 + D + G)
    ins = _inputs(g, B, G, N, NS, D)
    s, rm, o, neg_o, neg_s = ins
    ref64, ref32 = (rsr.rescal_sides_grouped_ref(s, rm, starts, o, neg_o, neg_s, N, NS, D, LR,
                                                 EPS, GE, GR, dt)
                    for dt in (torch.float64, torch.float32))
    return ins, starts, ref64, ref32


def run_grouped(sizes, N, NS, D):
    device = "cuda:0"
    ins, starts, ref64, ref32 = grouped_case(tuple(sizes), N, NS, D)
    bufs = {n: sr.Guarded(t.shape[0], t.shape[1], device) for n, t in zip(ROLES, ins)}
    loss = _C.rescal_step_sides_grouped(*[t.to(device) for t in ins],
                                        *[b.out for b in bufs.values()],
                                        torch.from_numpy(starts), N, NS, D, LR, EPS, GE, GR)
    _sync(device)
    got = {n: b.out for n, b in bufs.items()}
    got["loss"] = loss
    what = f"rescal_sides_grouped G={len(sizes)} B={sum(sizes)} max={max(sizes)} D={D}"
    sr.assert_step_close(got, ref64, ref32, what, "rescal_step_sides_grouped[gpu]")
    _check_guards(bufs, what)
    dr = bufs["r"].out.cpu()
    for gi, size in enumerate(sizes):
        if size == 0:
            assert not dr[gi].any(), f"{what}: dR of empty group {gi} is not [0 | 0]"


@GPU
@pytest.mark.parametrize("D", [4, 20, 32, 68, 128])
def test_sides_grouped_dims(D):
    """Groups of 0, 1, 17 (> one m-tile) and 40 (> a K chunk) rows; D below,
    at and above one n-tile and not a multiple of 16. gamma_r > 0 and the
    empty group's drl is still [0 | 0]."""
    run_grouped([0, 1, 17, 40, 3], 2, 2, D)


@GPU
def test_sides_grouped_grid_stride():
    run_grouped([8200], 1, 1, 4)  # cap 8192 of the middle phase


@GPU
def test_sides_grouped_adagrad_grid_stride():
    """130 relation matrices of 128 x 128 are 2,129,920 values, past the
    8192 x 256 threads of the AdaGrad epilogue; groups of 1 and 2 among empty
    ones, so gamma_r * Bg * R_g differs between them."""
    run_grouped([0] * 60 + [1] + [0] * 60 + [2] + [0] * 8, 2, 2, 128)


@GPU
def test_sides_grouped_reduces_to_the_one_sided_step():
    """NS = 0 and both gammas 0: the same bits as rescal_step_grouped."""
    device, N, D = "cuda:0", 3, 20
    sizes = (0, 1, 17, 3)
    starts = torch.from_numpy(np.cumsum((0,) + sizes).astype(np.int32))
    B, G = sum(sizes), len(sizes)
    g = torch.Generator().manual_seed(26000)
    s, rm, o, neg, none = (t.to(device) for t in _inputs(g, B, G, N, 0, D))
    want = [torch.full_like(t, float("nan")) for t in (s, rm, o, neg)]
    want_loss = _C.rescal_step_grouped(s, rm, o, neg, *want, starts, N, D, LR, EPS)
    got = [torch.full_like(t, float("nan")) for t in (s, rm, o, neg)]
    got_loss = _C.rescal_step_sides_grouped(s, rm, o, neg, none, *got, torch.empty_like(none),
                                            starts, N, 0, D, LR, EPS, 0.0, 0.0)
    _sync(device)
    for name, a, b in zip(("ds", "drl", "do", "dneg"), got, want):
        assert not torch.isnan(b).any()
        assert torch.equal(a, b), f"{name}: max diff {(a - b).abs().max().item():g}"
    assert torch.equal(got_loss, want_loss)


# ------------------------------------------------------------ 3. guards

def _guard_args(device, D=4, B=2, N=2, NS=2, ns_rows=None):
    """Well-formed arguments of both entry points (one group of B triples),
    outputs prefilled with NaN. ns_rows overrides the row count of neg_s."""
    rows = lambda n, L: torch.zeros(n, 2 * L, device=device)
    ins = [rows(B, D), rows(B, D * D), rows(B, D), rows(B * N, D),
           rows(B * NS if ns_rows is None else ns_rows, D)]
    outs = [torch.full_like(t, float("nan")) for t in ins]
    return ins, outs


def _per_triple(ins, outs, N, NS, D, ge=GE, gr=GR):
    loss = torch.full((ins[0].shape[0],), float("nan"), device=outs[0].device)
    outs.append(loss)
    _C.rescal_step_sides(*ins, *outs[:5], loss, N, NS, D, LR, EPS, ge, gr)


def _grouped(ins, outs, N, NS, D, ge=GE, gr=GR):
    B = ins[0].shape[0]
    ins = [ins[0], ins[1][:1].contiguous(), *ins[2:]]  # one group: one relation row
    outs[1] = outs[1][:1].contiguous()
    _C.rescal_step_sides_grouped(*ins, *outs[:5], torch.tensor([0, B], dtype=torch.int32),
                                 N, NS, D, LR, EPS, ge, gr)


def _refused(device, entry, match, ins, outs, *tail, **kw):
    with pytest.raises(RuntimeError, match=match):
        entry(ins, outs, *tail, **kw)
    _sync(device)
    for t in outs:  # nothing ran: every output is as it was
        assert torch.isnan(t).all()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("entry", [_per_triple, _grouped], ids=["per_triple", "grouped"])
def test_sides_guards(device, entry):
    """What both entry points refuse on the host, before anything is launched."""
    D = 4
    _refused(device, entry, r"neg_s and dneg_s must be \[B\*NS\]\[2D\]",
             *_guard_args(device, ns_rows=3), 2, 2, D)
    ins, outs = _guard_args(device)
    outs[4] = outs[4][:3].contiguous()
    _refused(device, entry, r"neg_s and dneg_s must be \[B\*NS\]\[2D\]", ins, outs, 2, 2, D)
    _refused(device, entry, "must be >= 0", *_guard_args(device, NS=0), 2, -1, D)
    _refused(device, entry, "must be >= 0", *_guard_args(device, N=0), -1, 2, D)
    _refused(device, entry, "gamma_e = -0.5 .* must be >= 0", *_guard_args(device), 2, 2, D,
             ge=-0.5)
    _refused(device, entry, "gamma_r = -0.25 must be >= 0", *_guard_args(device), 2, 2, D,
             gr=-0.25)
    # mixed devices: one tensor elsewhere ("meta" holds no data and needs no GPU)
    other = "cpu" if device != "cpu" else "meta"
    for i in (2, 4):
        ins, outs = _guard_args(device)
        ins[i] = torch.zeros(ins[i].shape, device=other)
        _refused(device, entry, "different devices", ins, outs, 2, 2, D)
    ins, outs = _guard_args(device)
    outs[3] = torch.full(outs[3].shape, float("nan"), device=other)
    with pytest.raises(RuntimeError, match="different devices"):
        entry(ins, outs, 2, 2, D)
    _sync(device)
    assert all(torch.isnan(t).all() for t in outs if t.device.type != "meta")


@pytest.mark.parametrize("device", DEVICES)
def test_sides_per_triple_dimension_limit(device):
    D = 197
    _refused(device, _per_triple, "D = 197 must be <= 196", *_guard_args(device, D=D, B=1, N=1, NS=1),
             1, 1, D)


@pytest.mark.parametrize("device", DEVICES)
def test_sides_grouped_dimension_multiple_of_4(device):
    D = 6
    _refused(device, _grouped, "D = 6 must be a positive multiple of 4",
             *_guard_args(device, D=D), 2, 2, D)


# ------------------------------------------------------------ 4. model

SPARE_ROWS = 7
E_M, R_M, D_M, B_M, N_M, NS_M = 56, 3, 4, 8, 2, 2


def _reset_runtime():
    import adapm_amd

    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    return adapm_amd


class RescalStore:
    """A world-1 store of known rows with RESCAL's two value lengths, and the
    model on it."""

    def __init__(self, device, seed, **cfg_kw):
        from adapm_amd.models.kge import ComplExConfig, Rescal

        adapm_amd = _reset_runtime()
        self.device = device
        adapm_amd.setup(num_keys=E_M + R_M, num_threads=1, device=device)
        self.server = adapm_amd.Server(torch.from_numpy(Rescal.value_lengths(E_M, R_M, D_M)))
        self.worker = adapm_amd.Worker(0, self.server)
        self.g = torch.Generator().manual_seed(seed)
        self.ekeys = np.arange(E_M, dtype=np.int64)
        self.rkeys = E_M + np.arange(R_M, dtype=np.int64)
        self.worker.set(self.ekeys, _rows(self.g, E_M, D_M).to(device))
        self.worker.set(self.rkeys, _rows(self.g, R_M, D_M * D_M, scale=0.1).to(device))
        self.worker.wait_sync()
        self.snapshot = self.pull_all()
        cfg = ComplExConfig(num_entities=E_M, num_relations=R_M, dim=D_M, neg_samples=N_M,
                            batch_size=B_M, lr=LR, eps=EPS, **cfg_kw)
        self.model = Rescal(cfg, self.server, self.worker)

    def pull_all(self):
        """(entity rows [E][2D], relation rows [R][2D^2])"""
        ent = torch.empty(E_M, 2 * D_M, device=self.device)
        rel = torch.empty(R_M, 2 * D_M * D_M, device=self.device)
        self.worker.pull(self.ekeys, ent)
        self.worker.pull(self.rkeys, rel)
        _sync(self.device)
        return ent.cpu(), rel.cpu()

    def close(self):
        self.worker.finalize()
        self.server.shutdown()


def _check_rows(snap, after, L, keys, deltas64, deltas32, min_rest, what, family):
    """The _check_store of tests/test_kge_sides.py for one value length:
    `after` == snapshot + reference deltas summed by key, per half over the
    named rows; every other row bit-identical."""
    exp = [snap.clone().to(dt).index_add_(0, keys, d.to(dt))
           for d, dt in ((deltas64, torch.float64), (deltas32, torch.float32))]
    named = torch.unique(keys)
    for half, part in ((0, "emb"), (1, "acc")):
        cols = slice(half * L, (half + 1) * L)
        sr.assert_half_close(after[named][:, cols], exp[0][named][:, cols], exp[1][named][:, cols],
                             f"{what} {part}", family)
    rest = torch.ones(snap.shape[0], dtype=torch.bool)
    rest[named] = False
    assert int(rest.sum()) >= min_rest
    assert torch.equal(after[rest].view(torch.int32), snap[rest].view(torch.int32)), \
        f"{what}: a row that the batch does not name changed"


def run_model(device, grouped):
    st = RescalStore(device, 27000, neg_samples_subject=NS_M, gamma_entity=GE, gamma_relation=GR)
    try:
        assert st.model.cfg.sides
        perm = torch.randperm(E_M, generator=st.g)  # every entity key once
        cuts = np.cumsum([0, B_M, B_M, B_M * N_M, B_M * NS_M])
        assert cuts[-1] <= E_M - SPARE_ROWS
        ks, ko, kno, kns = (perm[a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:]))
        rel = torch.tensor([2, 0, 0, 2, 0, 0, 2, 0])  # relation 1 stays unnamed
        triples = torch.stack([ks, rel, ko], dim=1).numpy().astype(np.int64)
        neg_keys = torch.cat([kno, kns]).numpy()
        ent, rels = st.snapshot
        if grouped:  # the relation rows receive the delta of the group-summed gradient
            gid, rkeys = rel, torch.arange(R_M)
            ins = (ent[ks], rels, ent[ko], ent[kno], ent[kns])
        else:        # and here the sum of their per-triple deltas
            gid, rkeys = torch.arange(B_M), rel
            ins = (ent[ks], rels[rel], ent[ko], ent[kno], ent[kns])
        ref64, ref32 = (rsr._rescal_sides(ins[0], ins[1], gid, *ins[2:], N_M, NS_M, D_M, LR, EPS,
                                          GE, GR, dt) for dt in (torch.float64, torch.float32))
        loss = st.model.train_batch(triples, sync_loss=False, grouped=grouped, neg_keys=neg_keys)
        st.model.drain()
        st.worker.wait_sync()
        after_ent, after_rel = st.pull_all()
        fam = f"rescal_model_sides[{'gpu' if grouped else 'cpu'}]"
        what = f"model sides grouped={grouped}"
        # the grouped step runs its samples sorted by relation
        order = np.argsort(rel.numpy(), kind="stable") if grouped else np.arange(B_M)
        sr.assert_half_close(loss, ref64["loss"][order], ref32["loss"][order], f"{what} loss", fam)
        ekeys = torch.cat([ks, ko, kno, kns])
        e64, e32 = (torch.cat([torch.cat(ref[n], dim=1) for n in ("s", "o", "neg_o", "neg_s")])
                    for ref in (ref64, ref32))
        _check_rows(ent, after_ent, D_M, ekeys, e64, e32, SPARE_ROWS, f"{what} entities", fam)
        r64, r32 = (torch.cat(ref["r"], dim=1) for ref in (ref64, ref32))
        if grouped:  # the unnamed relation is an empty group there: delta [0 | 0], not pushed
            named = torch.unique(rel)
            rkeys, r64, r32 = named, r64[named], r32[named]
        _check_rows(rels, after_rel, D_M * D_M, rkeys, r64, r32, 1, f"{what} relations", fam)
    finally:
        st.close()


def test_model_sides_cpu_store():
    """One train_batch on a CPU store, grouped=False: the pulled rows equal
    before + delta_ref; relation rows named by several triples receive the sum
    of their per-triple deltas."""
    run_model("cpu", grouped=False)


@GPU
def test_model_sides_grouped_gpu():
    """The same on the GPU with grouped=True, where a relation row receives
    the delta of its group."""
    run_model("cuda:0", grouped=True)


def test_model_defaults_never_reach_the_sides_step(monkeypatch):
    """A default config trains as before: neither sides entry point is called."""
    from adapm_amd.models import kge

    def refuse(*a):
        raise AssertionError("the sides step ran under a default config")

    monkeypatch.setattr(kge._C, "rescal_step_sides", refuse)
    monkeypatch.setattr(kge._C, "rescal_step_sides_grouped", refuse)
    st = RescalStore("cpu", 28000)
    try:
        assert not st.model.cfg.sides
        g = np.random.default_rng(5)
        triples = np.stack([g.integers(0, E_M, B_M), g.integers(0, R_M, B_M),
                            g.integers(0, E_M, B_M)], axis=1).astype(np.int64)
        loss = st.model.train_batch(triples)
        st.model.drain()
        assert np.isfinite(loss) and loss > 0
    finally:
        st.close()
