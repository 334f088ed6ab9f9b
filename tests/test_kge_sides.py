"""The ComplEx sides step: N object-side and NS subject-side negatives per
positive and L2 (gamma_e, gamma_r) on the positive's rows, through every
layer: the classic kernel and its CPU twin, the fused slab-direct kernel on
the identity, device-sampled and general paths, and the model.

Numerical checks follow tests/test_kernel_reference.py: one half of one output
at a time against the fp64 reference of tests/sides_refs.py,
err = max|got - ref64| / max|ref64| <= 16 * max(e32, 2^-23) with e32 the same
error of the reference evaluated in fp32 (step_refs.assert_half_close, which
prints a RATIO line per half). Outputs are prefilled with NaN and followed by a
sentinel row.

The shared-row case steps with lr = 0, as tests/test_kge_fused_unique.py does:
with a learning rate, whether a workgroup reads a shared row before or after
another workgroup's update is a race that async-PS semantics allow, and no
bound on rounding error covers it. With lr = 0 the embeddings stay put, every
occurrence's gradient is that of the snapshot, and the accumulators become
snapshot + sum of g^2 over occurrences in whatever order the atomics land.
"""
import functools
import sys
import types

import numpy as np
import pytest
import torch

import sides_refs
import step_refs as sr
from adapm_amd import _C

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda:0", id="gpu", marks=pytest.mark.gpu)]
GPU = pytest.mark.gpu

LANES = [1, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025, 2047, 2048]
LR, EPS = 0.05, 1e-6
GE, GR = 0.05, 0.02


def _fam(name, device):
    return f"{name}[{'cpu' if device == 'cpu' else 'gpu'}]"


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _rows(g, n, L, scale=0.3, acc=0.1):
    """[n][2L] store rows: N(0, scale^2) embeddings | U(0, acc) accumulators."""
    a = torch.rand(n, L, generator=g) * acc if acc else torch.zeros(n, L)
    return torch.cat([torch.randn(n, L, generator=g) * scale, a], dim=1)


ROLES = ("s", "r", "o", "neg_o", "neg_s")


def _refs(ins, N, NS, D, lr=LR, ge=GE, gr=GR):
    return tuple(sides_refs.complex_sides_ref(*ins, N, NS, D, lr, EPS, ge, gr, dt)
                 for dt in (torch.float64, torch.float32))


# A case is built once (inputs, fp64 and fp32 reference) and shared by the CPU
# and GPU twins of a test; nothing modifies it afterwards.
@functools.lru_cache(maxsize=8)
def sides_case(B, N, NS, L, regime=None):
    D = 2 * L
    g = torch.Generator().manual_seed(11000 + L + 7 * N + 13 * NS)
    scale, acc = (0.04, 0.0) if regime == "a" else (0.3, 0.1)
    ins = tuple(_rows(g, n, D, scale, acc) for n in (B, B, B, B * N, B * NS))
    ref64, ref32 = _refs(ins, N, NS, D)
    if regime == "a":  # fresh rows: accumulators 0, g^2 on both sides of eps
        for name in ROLES:
            g2 = ref64[name][1]
            assert (g2 < EPS).any() and (g2 > EPS).any(), \
                f"regime (a): g^2 of {name} in [{g2.min():.3g}, {g2.max():.3g}] does not straddle eps"
    return ins, ref64, ref32


def _call_sides(device, ins, B, N, NS, D, lr=LR, ge=GE, gr=GR):
    """_C.kge_complex_step_sides on guarded outputs -> ({role: out, "loss": out}, guards)."""
    bufs = {n: sr.Guarded(t.shape[0], t.shape[1], device) for n, t in zip(ROLES, ins)}
    loss = sr.guarded_vec(B, device)
    _C.kge_complex_step_sides(*[t.to(device) for t in ins], *[b.out for b in bufs.values()],
                              loss.out, N, NS, D, lr, EPS, ge, gr)
    _sync(device)
    got = {n: b.out for n, b in bufs.items()}
    got["loss"] = loss.out
    return got, {**bufs, "loss": loss}


def run_sides(device, B, N, NS, L, regime=None):
    ins, ref64, ref32 = sides_case(B, N, NS, L, regime)
    what = f"sides B={B} N={N} NS={NS} L={L} {regime or ''}"
    got, guards = _call_sides(device, ins, B, N, NS, 2 * L)
    sr.assert_step_close(got, ref64, ref32, what, _fam("complex_sides", device))
    for n, b in guards.items():
        b.check(f"{what} {n}")


# ------------------------------------------------------------ 1. classic step

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("L", LANES)
def test_sides_step_lanes(device, L):
    """Every lanes-per-thread instantiation and the lane counts around them."""
    run_sides(device, 3, 2, 2, L)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("N,NS", [(0, 0), (0, 3), (3, 0), (1, 2)])
@pytest.mark.parametrize("L", [65, 2048])
def test_sides_step_negatives(device, L, N, NS):
    run_sides(device, 3, N, NS, L)


@pytest.mark.parametrize("device", DEVICES)
def test_sides_step_fresh_rows(device):
    run_sides(device, 3, 2, 2, 65, "a")


@pytest.mark.parametrize("device", DEVICES)
def test_sides_step_grid_stride(device):
    """More samples than the launch has workgroups (cap 16384)."""
    run_sides(device, 16400, 1, 1, 1)


# ------------------------------------------------------------ 2. reduction

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("L", [65, 513])
def test_sides_reduces_to_the_one_sided_step(device, L):
    """NS = 0 and both gammas 0: the same numbers as kge_complex_step."""
    B, N, D = 4, 3, 2 * L
    g = torch.Generator().manual_seed(12000 + L)
    s, r, o, neg = (_rows(g, n, D).to(device) for n in (B, B, B, B * N))
    none = torch.empty(0, 2 * D, device=device)
    want = [torch.full_like(t, float("nan")) for t in (s, r, o, neg)]
    want_loss = torch.full((B,), float("nan"), device=device)
    _C.kge_complex_step(s, r, o, neg, *want, want_loss, N, D, LR, EPS)
    got = [torch.full_like(t, float("nan")) for t in (s, r, o, neg)]
    got_loss = torch.full((B,), float("nan"), device=device)
    _C.kge_complex_step_sides(s, r, o, neg, none, *got, torch.empty_like(none), got_loss, N, 0, D,
                              LR, EPS, 0.0, 0.0)
    _sync(device)
    for name, a, b in zip(("ds", "dr", "do", "dneg"), got, want):
        assert not torch.isnan(b).any()
        assert torch.equal(a, b), f"{name}: max diff {(a - b).abs().max().item():g}"
    assert torch.equal(got_loss, want_loss)


# ------------------------------------------------------------ 3. regulariser only

@pytest.mark.parametrize("device", DEVICES)
def test_sides_regulariser_alone_moves_the_positive(device):
    """N = NS = 0 and psi about 30: the logistic gradient is about 1e-13, and
    s, r and o still take the AdaGrad step of gamma * E."""
    B, L = 2, 65
    D = 2 * L
    g = torch.Generator().manual_seed(13000)
    s, r, o = (_rows(g, B, D) for _ in range(3))
    none = torch.empty(0, 2 * D)
    psi = _refs((s, r, o, none, none), 0, 0, D)[0]["psi"][:, 0]
    o[:, :D] *= (30.0 / psi).float()[:, None]  # psi is linear in o
    ins = (s, r, o, none, none)
    ref64, ref32 = _refs(ins, 0, 0, D)
    assert ((ref64["psi"] - 30.0).abs() < 1e-3).all()
    for name, rows, gamma in (("s", s, GE), ("r", r, GR), ("o", o, GE)):
        reg = sr.adagrad_halves(sr._f32(gamma) * rows[:, :D].double(), rows[:, D:].double(),
                                sr._f32(LR), sr._f32(EPS))
        for half in (0, 1):
            assert reg[half].abs().min() > 0
            assert torch.allclose(ref64[name][half], reg[half], rtol=1e-6, atol=0)
    got, guards = _call_sides(device, ins, B, 0, 0, D)
    sr.assert_step_close(got, ref64, ref32, "sides regulariser only", _fam("complex_sides", device))
    for n, b in guards.items():
        b.check(f"regulariser only {n}")


# ------------------------------------------------------------ stores

SPARE_ROWS = 7


def _reset_runtime():
    import adapm_amd

    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    return adapm_amd


class Store:
    """A world-1 store of known rows (the FusedStore pattern of
    test_kernel_reference.py, on either device)."""

    def __init__(self, num_keys, L, seed, device="cuda:0", rows=None):
        adapm_amd = _reset_runtime()
        self.num_keys, self.L, self.device = num_keys, L, device
        adapm_amd.setup(num_keys=num_keys, num_threads=1, device=device)
        self.server = adapm_amd.Server(2 * L)
        self.worker = adapm_amd.Worker(0, self.server)
        self.g = torch.Generator().manual_seed(seed)
        if rows is None:
            rows = _rows(self.g, num_keys, L)
        self.worker.set(np.arange(num_keys, dtype=np.int64), rows.to(device))
        self.snapshot = self.pull_all()

    def pull_all(self):
        out = torch.empty(self.num_keys, 2 * self.L, device=self.device)
        self.worker.pull(np.arange(self.num_keys, dtype=np.int64), out)
        _sync(self.device)
        return out.cpu()

    def close(self):
        self.worker.finalize()
        self.server.shutdown()


def _check_store(st, after, keys_by_role, ref64, ref32, what, family):
    """`after` == snapshot + per-occurrence reference deltas summed by key, per
    half over the named rows; every other row bit-identical."""
    snap, L = st.snapshot, st.L
    keys = torch.cat([keys_by_role[n] for n in ROLES])
    exp = []
    for ref, dt in ((ref64, torch.float64), (ref32, torch.float32)):
        d = torch.cat([torch.cat(ref[n], dim=1) for n in ROLES]).to(dt)
        exp.append(snap.clone().to(dt).index_add_(0, keys, d))
    named = torch.unique(keys)
    for half, part in ((0, "emb"), (1, "acc")):
        cols = slice(half * L, (half + 1) * L)
        sr.assert_half_close(after[named][:, cols], exp[0][named][:, cols], exp[1][named][:, cols],
                             f"{what} {part}", family)
    rest = torch.ones(st.num_keys, dtype=torch.bool)
    rest[named] = False
    assert int(rest.sum()) >= SPARE_ROWS
    assert torch.equal(after[rest].view(torch.int32), snap[rest].view(torch.int32)), \
        f"{what}: a row that the batch does not name changed"


def _unique_keys(st, B, N, NS):
    """All keys different, in a random order, SPARE_ROWS keys left alone."""
    perm = torch.randperm(st.num_keys, generator=st.g)
    out, a = {}, 0
    for name, n in zip(ROLES, (B, B, B, B * N, B * NS)):
        out[name] = perm[a:a + n].contiguous()
        a += n
    assert a <= st.num_keys - SPARE_ROWS
    return out


# ------------------------------------------------------------ 4. fused, all keys unique

def run_fused_sides(B, N, NS, D):
    st = Store(B * (3 + N + NS) + SPARE_ROWS, D, seed=14000 + D)
    try:
        keys = _unique_keys(st, B, N, NS)
        ins = tuple(st.snapshot[keys[n]] for n in ROLES)
        ref64, ref32 = _refs(ins, N, NS, D)
        before = st.server.raw.stats()
        loss = st.server.raw.kge_step_sides_fused(*[keys[n] for n in ROLES], N, NS, D, LR, EPS,
                                                  GE, GR)
        torch.cuda.synchronize()
        stats = st.server.raw.stats()
        assert stats["fused_plain_steps"] == before["fused_plain_steps"] + 1
        assert stats["pull_keys"] - before["pull_keys"] == B * (3 + N + NS)
        what = f"fused sides B={B} N={N} NS={NS} D={D}"
        sr.assert_half_close(loss, ref64["loss"], ref32["loss"], f"{what} loss", "fused_sides[gpu]")
        _check_store(st, st.pull_all(), keys, ref64, ref32, what, "fused_sides[gpu]")
    finally:
        st.close()


@GPU
@pytest.mark.parametrize("D", [130, 514, 2050, 4096])  # 1, 2, 8 and 8 lanes per thread
def test_fused_sides(D):
    run_fused_sides(3, 2, 2, D)


@GPU
def test_fused_sides_grid_stride():
    run_fused_sides(16400, 1, 1, 2)


# ------------------------------------------------------------ 5. shared rows

def _shared_batch(E, R, B, N, NS):
    """One relation for all positives; entity X is s of sample 0, o of sample
    1, an o' of sample 2 and an s' of sample 3; every other entity is unique."""
    rng = np.random.default_rng(15)
    ents = torch.from_numpy(rng.permutation(E)[:B * (2 + N + NS)].astype(np.int64))
    keys, a = {}, 0
    for name, n in (("s", B), ("o", B), ("neg_o", B * N), ("neg_s", B * NS)):
        keys[name] = ents[a:a + n].clone()
        a += n
    keys["r"] = torch.full((B,), E + 3, dtype=torch.int64)
    x = keys["s"][0].item()
    keys["o"][1] = x
    keys["neg_o"][2 * N] = x
    keys["neg_s"][3 * NS + 1] = x
    return keys


@GPU
def test_fused_sides_shared_rows():
    """The UNIQ kernel's atomic branch beside its plain one, and the all-atomic
    general path on a twin store. lr = 0: see the module docstring."""
    E, R, B, D, N, NS = 512, 8, 64, 8, 2, 2
    keys = _shared_batch(E, R, B, N, NS)
    args = (*[keys[n] for n in ROLES], N, NS, D, 0.0, EPS, GE, GR)
    after = {}
    for path in ("identity", "general"):
        st = Store(E + R, D, seed=15000)
        try:
            ins = tuple(st.snapshot[keys[n]] for n in ROLES)
            ref64, ref32 = _refs(ins, N, NS, D, lr=0.0)
            before = st.server.raw.stats()
            if path == "identity":
                loss = st.server.raw.kge_step_sides_fused(*args)
                torch.cuda.synchronize()
                assert st.server.raw.stats()["fused_plain_steps"] == before["fused_plain_steps"] + 1
            else:
                loss, missed = st.server.raw.kge_step_sides_fused_general(*args)
                torch.cuda.synchronize()
                assert missed.numel() == 0
            what = f"fused sides shared rows, {path}"
            sr.assert_half_close(loss, ref64["loss"], ref32["loss"], f"{what} loss",
                                 "fused_sides[gpu]")
            after[path] = st.pull_all()
            _check_store(st, after[path], keys, ref64, ref32, what, "fused_sides[gpu]")
            # embeddings do not move at lr = 0, whichever way they are written
            assert torch.equal(after[path][:, :D], st.snapshot[:, :D])
        finally:
            st.close()
    assert torch.equal(after["identity"][:, :D], after["general"][:, :D])


# ------------------------------------------------------------ 6. general path, CPU store

@pytest.mark.parametrize("N,NS", [(0, 2), (2, 0), (2, 2)])
def test_sides_general_cpu_store(N, NS):
    """kge_step_sides_fused_general on a CPU store (the offsets-mode twin),
    with a key array of no keys: the store afterwards is snapshot + the classic
    sides step's deltas."""
    B, D = 5, 6
    st = Store(B * (3 + N + NS) + SPARE_ROWS, D, seed=16000 + N, device="cpu")
    try:
        keys = _unique_keys(st, B, N, NS)
        ins = tuple(st.snapshot[keys[n]].contiguous() for n in ROLES)
        ref64, ref32 = _refs(ins, N, NS, D)
        loss, missed = st.server.raw.kge_step_sides_fused_general(
            *[keys[n] for n in ROLES], N, NS, D, LR, EPS, GE, GR)
        assert missed.numel() == 0 and loss.shape == (B,)
        after = st.pull_all()
        what = f"general sides cpu N={N} NS={NS}"
        sr.assert_half_close(loss, ref64["loss"], ref32["loss"], f"{what} loss", "general_sides[cpu]")
        _check_store(st, after, keys, ref64, ref32, what, "general_sides[cpu]")
        # and the classic step itself
        deltas = [torch.empty_like(t) for t in ins]
        closs = torch.empty(B)
        _C.kge_complex_step_sides(*ins, *deltas, closs, N, NS, D, LR, EPS, GE, GR)
        want = st.snapshot.clone().index_add_(0, torch.cat([keys[n] for n in ROLES]),
                                              torch.cat(deltas))
        assert torch.allclose(after, want, rtol=2e-4, atol=2e-5)
        assert torch.allclose(loss, closs, rtol=1e-5, atol=1e-6)
    finally:
        st.close()


# ------------------------------------------------------------ 7. device-sampled

@GPU
def test_sides_sampled_step_equals_host_key_step():
    """The drawn keys are the host stream's next B * (N + NS), object-side
    first; the loss is that of the host-key step on a twin store."""
    from adapm_amd.sampling import Uniform

    E, R, D, B, N, NS, seed = 1_000_000, 8, 2, 33, 3, 2, 31
    want_neg = np.random.default_rng(seed).integers(0, E, size=B * (N + NS), dtype=np.int64)
    free = np.setdiff1d(np.arange(4 * B * (N + NS), dtype=np.int64), want_neg)
    pos = [torch.from_numpy(np.ascontiguousarray(k)) for k in
           (free[:B], E + np.arange(B, dtype=np.int64) % R, free[B:2 * B])]
    rows = _rows(torch.Generator().manual_seed(17000), E + R, D)
    losses = []
    for sampled in (True, False):
        st = Store(E + R, D, seed=0, rows=rows)
        try:
            if sampled:
                us = Uniform(0, E, seed).native_stream("cuda:0")
                loss, neg = st.server.raw.kge_step_sides_fused_sampled(*pos, us, N, NS, D, LR, EPS,
                                                                       GE, GR)
                assert neg.is_cuda and neg.dtype == torch.int64
                assert np.array_equal(neg.cpu().numpy(), want_neg)
            else:
                neg = torch.from_numpy(want_neg)
                loss = st.server.raw.kge_step_sides_fused(*pos, neg[:B * N].contiguous(),
                                                          neg[B * N:].contiguous(), N, NS, D, LR,
                                                          EPS, GE, GR)
            torch.cuda.synchronize()
            losses.append(loss.cpu())
        finally:
            st.close()
    assert torch.isfinite(losses[0]).all() and torch.equal(losses[0], losses[1])


# ------------------------------------------------------------ 8. model
#
# The fake worker and server of test_model_steps.py: no process group and no
# store; pulled rows are a function of their keys.

B_M, NEG, NEG_S, DIM, ENT, REL, RANK = 4, 2, 2, 8, 32, 4, 1
ROW = 2 * DIM


def fake_rows(keys):
    k = torch.from_numpy(np.asarray(keys, dtype=np.int64))
    col = torch.arange(ROW, dtype=torch.float32)
    return (0.05 + 0.01 * (k % 7).float()[:, None] + 0.001 * col[None, :]).contiguous()


class FakeWorker:
    def __init__(self):
        self.log = []  # ("pull", keys) / ("push", keys, deltas)

    def pull(self, keys, vals, async_=False):
        keys = np.array(keys, dtype=np.int64)
        self.log.append(("pull", keys))
        vals.view(len(keys), ROW).copy_(fake_rows(keys))
        return 10_000

    def push(self, keys, vals, async_=False):
        self.log.append(("push", np.array(keys, dtype=np.int64), vals.clone()))
        return 0

    def wait(self, ts):
        pass

    def current_clock(self):
        return 0


class FakeRaw:
    def __init__(self):
        self.calls = []

    def layout_identity(self):
        return False

    def __getattr__(self, name):
        def general(*args):
            self.calls.append((name, args))
            return torch.zeros(len(args[0])), torch.zeros(0, dtype=torch.int64)
        return general


class KernelLog:
    """Stands in for the model's `_C`: forwards to the real one, logs the name
    and arguments of every call."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(_C, name)

        def logged(*args):
            self.calls.append((name, args))
            return fn(*args)
        return logged


def _model(monkeypatch, **cfg_kw):
    from adapm_amd.models import kge

    log = KernelLog()
    monkeypatch.setattr(kge, "_C", log)
    worker, raw = FakeWorker(), FakeRaw()
    rt = types.SimpleNamespace(device=torch.device("cpu"), rank=RANK, world=2)
    server = types.SimpleNamespace(rt=rt, sampling=None, raw=raw)
    cfg = kge.ComplExConfig(num_entities=ENT, num_relations=REL, dim=DIM, neg_samples=NEG,
                            batch_size=B_M, seed=3, **cfg_kw)
    return kge.ComplEx(cfg, server, worker), worker, raw, log


def _triples():
    g = np.random.default_rng(100)
    return np.stack([g.integers(0, ENT, B_M), g.integers(0, REL, B_M),
                     g.integers(0, ENT, B_M)], axis=1).astype(np.int64)


def test_model_defaults_take_the_one_sided_step(monkeypatch):
    model, worker, raw, log = _model(monkeypatch)
    assert not model.cfg.sides
    t = _triples()
    model.train_batch(t)
    model.train_prefetched(model.prefetch(t))
    assert [c[0] for c in log.calls] == ["kge_complex_step"] * 2
    assert all(len(e[1]) == B_M * (3 + NEG) for e in worker.log)
    model.train_batch_fused(t, force_general=True)
    (name, args), = raw.calls
    assert name == "kge_step_fused_general" and len(args) == 8 and args[4] == NEG


def test_model_sides_step_layout_and_deltas(monkeypatch):
    model, worker, raw, log = _model(monkeypatch, neg_samples_subject=NEG_S, gamma_entity=GE,
                                     gamma_relation=GR)
    assert model.cfg.sides
    t = _triples()
    draw = np.random.default_rng(3 + RANK).integers(0, ENT, size=B_M * (NEG + NEG_S),
                                                    dtype=np.int64)
    parts = [t[:, 0], ENT + t[:, 1], t[:, 2], draw[:B_M * NEG], draw[B_M * NEG:]]
    want_keys = np.concatenate(parts)
    loss = model.train_batch(t, sync_loss=False)
    (pull, pushed) = worker.log
    assert pull[0] == "pull" and np.array_equal(pull[1], want_keys)  # s | r | o | neg_o | neg_s
    assert pushed[0] == "push" and np.array_equal(pushed[1], want_keys)
    assert [c[0] for c in log.calls] == ["kge_complex_step_sides"]
    assert log.calls[0][1][-7:] == (NEG, NEG_S, DIM, model.cfg.lr, model.cfg.eps, GE, GR)
    ins = tuple(fake_rows(p) for p in parts)
    ref64, ref32 = (sides_refs.complex_sides_ref(*ins, NEG, NEG_S, DIM, model.cfg.lr,
                                                 model.cfg.eps, GE, GR, dt)
                    for dt in (torch.float64, torch.float32))
    deltas, a = {"loss": loss}, 0
    for name, p in zip(ROLES, parts):
        deltas[name] = pushed[2][a:a + len(p) * ROW].view(len(p), ROW)
        a += len(p) * ROW
    sr.assert_step_close(deltas, ref64, ref32, "model sides step", "model_sides[cpu]")

    # the fused general path and the prefetch pipeline take the sides step too
    model.train_batch_fused(t, force_general=True)
    (name, args), = raw.calls
    assert name == "kge_step_sides_fused_general"
    assert [len(a) for a in args[:5]] == [B_M, B_M, B_M, B_M * NEG, B_M * NEG_S]
    assert args[5:] == (NEG, NEG_S, DIM, model.cfg.lr, model.cfg.eps, GE, GR)
    model.train_prefetched(model.prefetch(t))
    assert log.calls[-1][0] == "kge_complex_step_sides"


def test_cli_gamma_entity_reaches_the_kernel(monkeypatch, capsys):
    from adapm_amd.models import kge

    _reset_runtime()
    log = KernelLog()
    monkeypatch.setattr(kge, "_C", log)
    monkeypatch.setattr(sys, "argv", [
        "kge", "--entities", "40", "--relations", "3", "--dim", "4", "--neg", "2",
        "--neg-samples-subject", "1", "--gamma-entity", "0.25", "--gamma-relation", "0.125",
        "--triples", "16", "--batch", "8", "--epochs", "1", "--eval-every", "0",
        "--device", "cpu"])
    kge.main()
    steps = [c for c in log.calls if c[0].startswith("kge_complex_step")]
    assert [c[0] for c in steps] == ["kge_complex_step_sides"] * 2
    assert all(c[1][-7:-4] == (2, 1, 4) and c[1][-2:] == (0.25, 0.125) for c in steps)


# ------------------------------------------------------------ 9. guards

def test_sides_guards():
    """What the sides step refuses, before it looks at the store or enqueues
    anything; a CPU store is enough."""
    D = 4
    st = Store(16, D, seed=19000, device="cpu")
    try:
        raw = st.server.raw
        k = torch.arange(2, dtype=torch.int64)
        neg = torch.arange(4, dtype=torch.int64) + 4
        none = torch.empty(0, dtype=torch.int64)
        tail = (LR, EPS, GE, GR)
        with pytest.raises(RuntimeError, match="kge_step_sides_fused: D/2 = 2050 exceeds .* limit of 2048"):
            raw.kge_step_sides_fused(k, k + 2, k + 4, neg, neg + 4, 2, 2, 4100, *tail)
        for N, NS in ((-1, 2), (2, -1)):
            with pytest.raises(RuntimeError, match="must be >= 0"):
                raw.kge_step_sides_fused(k, k + 2, k + 4, neg, neg + 4, N, NS, D, *tail)
            with pytest.raises(RuntimeError, match="must be >= 0"):
                raw.kge_step_sides_fused_general(k, k + 2, k + 4, neg, neg + 4, N, NS, D, *tail)
        with pytest.raises(RuntimeError, match="disagree on the batch"):
            raw.kge_step_sides_fused(k, k[:1] + 2, k + 4, neg, neg + 4, 2, 2, D, *tail)
        with pytest.raises(RuntimeError, match="disagree on the batch"):
            raw.kge_step_sides_fused(k, k + 2, k + 4, neg, neg[:3] + 4, 2, 2, D, *tail)
        with pytest.raises(RuntimeError, match="disagree on the batch"):
            raw.kge_step_sides_fused_general(k, k + 2, k + 4, neg[:3], neg + 4, 2, 2, D, *tail)
        # (3 + N + NS) * B must stay below 2^32 - 1
        with pytest.raises(RuntimeError, match="too many keys in one step"):
            raw.kge_step_sides_fused(k, k + 2, k + 4, none, none, 2 ** 30, 2 ** 30, D, *tail)
        assert torch.equal(st.pull_all(), st.snapshot)
    finally:
        st.close()

    # the classic binding: negative counts and tensors that are not [rows][2D]
    rows = lambda n: torch.zeros(n, 2 * D)
    ok = [rows(2), rows(2), rows(2), rows(4), rows(4)]
    for N, NS in ((-1, 2), (2, -1)):
        with pytest.raises(RuntimeError, match="must be >= 0"):
            _C.kge_complex_step_sides(*ok, *ok, torch.zeros(2), N, NS, D, *tail)
    bad = ok[:4] + [rows(3)]
    with pytest.raises(RuntimeError, match=r"neg_s and dneg_s must be \[B\*NS\]\[2D\]"):
        _C.kge_complex_step_sides(*bad, *ok, torch.zeros(2), 2, 2, D, *tail)
    with pytest.raises(RuntimeError, match=r"neg_s and dneg_s must be \[B\*NS\]\[2D\]"):
        _C.kge_complex_step_sides(*ok, *bad, torch.zeros(2), 2, 2, D, *tail)


@GPU
def test_sides_classic_dimension_limit():
    D = 4100
    rows = [torch.zeros(n, 2 * D, device="cuda") for n in (1, 1, 1, 1, 1)]
    with pytest.raises(RuntimeError, match="kge_complex_step_sides: D/2 = 2050 exceeds .* limit of 2048"):
        _C.kge_complex_step_sides(*rows, *[torch.empty_like(t) for t in rows],
                                  torch.empty(1, device="cuda"), 1, 1, D, LR, EPS, GE, GR)
    torch.cuda.synchronize()
