"""ComplEx step with chunk-shared negatives (csrc/kernels.h,
kge_complex_step_chunk) against the fp64 autograd reference of chunk_refs.py:
the raw step (CPU twin and the MFMA kernels), the fused identity step on a
whole store, the sampled entry, the model, and the guards. Every comparison
is one half of one output with the bound 16 * max(e32, 2^-23) of
step_refs.assert_half_close.

The shared-rows case steps with lr = 0 for the reason test_kge_sides.py
gives: embeddings stay put and the accumulators become the exact sum of g^2
over occurrences, whatever the order in which the workgroups run."""
import numpy as np
import pytest
import torch

import step_refs as sr
from chunk_refs import complex_chunk_ref

from adapm_amd import _C

GPU = pytest.mark.gpu
DEVICES = ["cpu", pytest.param("cuda:0", marks=GPU)]
LR, EPS = 0.05, 1e-6
ROLES = ("s", "r", "o", "neg")
SPARE_ROWS = 7
# (B, C, M, D): one element; off the tile; a short last chunk of 1; full tiles;
# C and M off the tile with three K-chunk tails; the M limit; the headline row
# length; one chunk shorter than C
SHAPES = [(1, 1, 1, 8), (17, 16, 15, 8), (33, 16, 17, 40), (64, 64, 16, 64), (70, 33, 40, 136),
          (5, 64, 3, 16), (65, 64, 256, 8), (130, 64, 64, 512)]
# The launches map one workgroup to every (chunk, block) and have no grid cap;
# this has more chunks than the 16384 blocks the older step kernels stop at.
MANY_CHUNKS = (16500, 1, 2, 8)


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _rows(g, n, D):
    """[n][2D] rows: N(0, 0.3^2) embeddings | U(0, 0.1) accumulators."""
    return torch.cat([torch.randn(n, D, generator=g) * 0.3, torch.rand(n, D, generator=g) * 0.1], 1)


def _n_neg(B, C, M):
    return -(-B // C) * M


def _refs(ins, C, M, D, lr=LR):
    return tuple(complex_chunk_ref(*ins, C, M, D, lr, EPS, dt)
                 for dt in (torch.float64, torch.float32))


def _raw_step(device, B, C, M, D):
    g = torch.Generator().manual_seed(1000 * B + 10 * M + D)
    ins = tuple(_rows(g, n, D) for n in (B, B, B, _n_neg(B, C, M)))
    bufs = [sr.Guarded(t.shape[0], 2 * D, device) for t in ins]
    loss = sr.guarded_vec(B, device)
    _C.kge_complex_step_chunk(*[t.to(device) for t in ins], *[b.out for b in bufs], loss.out,
                              C, M, D, LR, EPS)
    _sync(device)
    for b in bufs + [loss]:
        b.check(f"chunk step {B, C, M, D}")
    return ins, {**{n: b.out for n, b in zip(ROLES, bufs)}, "loss": loss.out}


# ------------------------------------------------------------ 1. raw step

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("B,C,M,D", SHAPES + [MANY_CHUNKS])
def test_raw_step(device, B, C, M, D):
    ins, got = _raw_step(device, B, C, M, D)
    sr.assert_step_close(got, *_refs(ins, C, M, D), f"chunk {B, C, M, D}",
                         f"kge_chunk[{device[:4]}]")


@pytest.mark.parametrize("device", DEVICES)
def test_chunk_of_one_is_the_complex_step(device):
    B, M, D = 9, 5, 24
    ins, got = _raw_step(device, B, 1, M, D)
    ref64, ref32 = (sr.complex_ref(*ins, M, D, LR, EPS, dt) for dt in (torch.float64, torch.float32))
    ref64.pop("psi"), ref32.pop("psi")
    mine = _refs(ins, 1, M, D)[0]
    assert all(torch.equal(mine[n][h], ref64[n][h]) for n in ROLES for h in (0, 1))
    sr.assert_step_close(got, ref64, ref32, "chunk C=1 vs complex_ref", f"kge_chunk[{device[:4]}]")


# ------------------------------------------------------------ 2. fused identity step

class Store:
    """A world-1 store of known rows on either device."""

    def __init__(self, num_keys, D, seed, device="cuda:0", sampling_entities=0):
        import adapm_amd

        adapm_amd._SETUP.clear()
        adapm_amd.runtime._RUNTIME = None
        self.num_keys, self.D, self.device = num_keys, D, device
        adapm_amd.setup(num_keys=num_keys, num_threads=1, device=device)
        self.server = adapm_amd.Server(2 * D)
        if sampling_entities:
            self.server.enable_sampling_support("local", True, "uniform", 0, sampling_entities)
        self.worker = adapm_amd.Worker(0, self.server)
        self.g = torch.Generator().manual_seed(seed)
        self.worker.set(np.arange(num_keys, dtype=np.int64), _rows(self.g, num_keys, D).to(device))
        self.snapshot = self.pull_all()

    def pull_all(self):
        out = torch.empty(self.num_keys, 2 * self.D, device=self.device)
        self.worker.pull(np.arange(self.num_keys, dtype=np.int64), out)
        _sync(self.device)
        return out.cpu()

    def unique_keys(self, B, n_neg):
        """All keys different, in a random order, SPARE_ROWS keys left alone."""
        perm = torch.randperm(self.num_keys - SPARE_ROWS, generator=self.g)
        return [perm[a:a + n].contiguous() for a, n in ((0, B), (B, B), (2 * B, B), (3 * B, n_neg))]

    def check(self, after, keys, C, M, lr, what, family, loss=None):
        """`after` == snapshot + the reference's per-occurrence deltas summed by
        key, half by half over the named rows; every other row keeps its bits."""
        D, snap = self.D, self.snapshot
        ref64, ref32 = _refs(tuple(snap[k] for k in keys), C, M, D, lr)
        if loss is not None:
            sr.assert_half_close(loss, ref64["loss"], ref32["loss"], f"{what} loss", family)
        allk = torch.cat(keys)
        exp = [snap.clone().to(dt).index_add_(0, allk, torch.cat([torch.cat(ref[n], 1) for n in ROLES]))
               for ref, dt in ((ref64, torch.float64), (ref32, torch.float32))]
        named = torch.unique(allk)
        for half, part in ((0, "emb"), (1, "acc")):
            cols = slice(half * D, (half + 1) * D)
            sr.assert_half_close(after[named][:, cols], exp[0][named][:, cols],
                                 exp[1][named][:, cols], f"{what} {part}", family)
        rest = torch.ones(self.num_keys, dtype=torch.bool)
        rest[named] = False
        assert int(rest.sum()) >= SPARE_ROWS
        assert torch.equal(after[rest].view(torch.int32), snap[rest].view(torch.int32)), \
            f"{what}: a row that the batch does not name changed"

    def close(self):
        self.worker.finalize()
        self.server.shutdown()


def _fused(st, keys, C, M, lr=LR, branch="plain"):
    before = st.server.raw.stats()
    loss = st.server.raw.kge_step_chunk_fused(*keys, C, M, st.D, lr, EPS)
    torch.cuda.synchronize()
    assert st.server.raw.stats()[f"fused_{branch}_steps"] == before[f"fused_{branch}_steps"] + 1
    return loss


@GPU
@pytest.mark.parametrize("branch", ["plain", "atomic"])
@pytest.mark.parametrize("B,C,M,D", SHAPES[:6] + [MANY_CHUNKS])
def test_fused_store(monkeypatch, branch, B, C, M, D):
    if branch == "atomic":
        monkeypatch.setenv("ADAPM_FUSED_ATOMIC", "1")  # read on a server's first fused step
    st = Store(3 * B + _n_neg(B, C, M) + SPARE_ROWS, D, seed=2000 + B)
    try:
        keys = st.unique_keys(B, _n_neg(B, C, M))
        loss = _fused(st, keys, C, M, branch=branch)
        st.check(st.pull_all(), keys, C, M, LR, f"fused {branch} {B, C, M, D}",
                 f"kge_chunk_fused[{branch}]", loss)
    finally:
        st.close()


# ------------------------------------------------------------ 3. shared rows

@GPU
def test_fused_shared_rows():
    """Key x is s of two positives in different chunks, o of a third, a
    negative of chunk 0 and twice a negative of chunk 2."""
    B, C, M, D = 10, 4, 6, 16
    st = Store(3 * B + _n_neg(B, C, M) + SPARE_ROWS, D, seed=3000)
    try:
        keys = st.unique_keys(B, _n_neg(B, C, M))
        x = keys[0][0]
        keys[0][5], keys[2][9] = x, x
        keys[3][2], keys[3][2 * M + 1], keys[3][2 * M + 4] = x, x, x
        _fused(st, keys, C, M, lr=0.0)
        after = st.pull_all()
        assert torch.equal(after[:, :D].view(torch.int32), st.snapshot[:, :D].view(torch.int32))
        st.check(after, keys, C, M, 0.0, "fused shared rows", "kge_chunk_fused[shared]")
    finally:
        st.close()


# ------------------------------------------------------------ 5. sampled entry

@GPU
@pytest.mark.parametrize("E,unique", [(1_000_000, True), (40, False)])
def test_sampled_equals_host_keys(E, unique):
    """The sampled entry draws ceil(B/C) * M keys; the host-keys step with
    those keys, from the same snapshot, gives the same store."""
    from adapm_amd.sampling import Uniform

    B, C, M, D, R = 21, 8, 5, 8, 21
    rng = np.random.default_rng(5)
    pos = [torch.from_numpy(k) for k in (rng.permutation(E)[:B], E + np.arange(B, dtype=np.int64),
                                         rng.permutation(E)[:B])]
    lr = LR if unique else 0.0
    stores, after = [], []
    try:
        for sampled in (True, False):
            st = Store(E + R, D, seed=5000)
            stores.append(st)
            if sampled:
                us = Uniform(0, E, 31).native_stream("cuda:0")
                loss, neg = st.server.raw.kge_step_chunk_fused_sampled(*pos, us, C, M, D, lr, EPS)
                assert neg.is_cuda and neg.shape == (_n_neg(B, C, M),)
                neg = neg.cpu()
                n_unique = len(torch.unique(torch.cat(pos + [neg])))
                if unique and n_unique != 3 * B + len(neg):
                    pytest.fail("the draw was expected to give unique keys")
            else:
                st.server.raw.kge_step_chunk_fused(*pos, neg, C, M, D, lr, EPS)
            torch.cuda.synchronize()
            after.append(st.pull_all())
        if unique:
            assert torch.equal(after[0].view(torch.int32), after[1].view(torch.int32))
        stores[0].check(after[0], pos + [neg], C, M, lr, f"sampled unique={unique}",
                        "kge_chunk_fused[sampled]")
    finally:
        for st in stores:
            st.close()


# ------------------------------------------------------------ 6. model

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("C,fused", [(0, False), (4, False), (4, True)])
def test_model(device, C, fused):
    """ComplEx with neg_chunk = C on a real store, negatives supplied; with
    neg_chunk = 0 the same calls give the step with negatives per positive."""
    from adapm_amd.models.kge import ComplEx, ComplExConfig

    E, R, B, M, D = 64, 10, 10, 3, 16
    st = Store(E + R, D, seed=6000 + C, device=device, sampling_entities=E)
    try:
        cfg = ComplExConfig(num_entities=E, num_relations=R, dim=D, neg_samples=M, lr=LR, eps=EPS,
                            neg_chunk=C)
        model = ComplEx(cfg, st.server, st.worker)
        perm = torch.randperm(E, generator=st.g)
        n_neg = _n_neg(B, C, M) if C else B * M
        triples = torch.stack([perm[:B], torch.arange(B), perm[B:2 * B]], 1).numpy()
        neg = perm[2 * B:2 * B + n_neg].contiguous()
        step = model.train_batch_fused if fused else model.train_batch
        loss = step(triples, sync_loss=False, neg_keys=neg.numpy())
        model.drain()
        st.worker.wait_sync()
        keys = [torch.from_numpy(k) for k in model.keys_of(triples)] + [neg]
        # neg_chunk = 0: chunks of one positive are the per-positive objective
        st.check(st.pull_all(), keys, C or 1, M, LR, f"model C={C} fused={fused}",
                 f"kge_chunk_model[{device[:4]}]", loss)
    finally:
        st.close()


# ------------------------------------------------------------ 7. guards

def _raw_args(device, B=4, C=2, M=3, D=8, n_neg=None, **bad):
    g = torch.Generator().manual_seed(7)
    n_neg = _n_neg(B, max(C, 1), M) if n_neg is None else n_neg
    t = [_rows(g, n, D).to(device) for n in (B, B, B, n_neg)]
    return (*t, *[torch.full_like(x, 7.0) for x in t], torch.full((B,), 7.0, device=device),
            C, M, D, LR, EPS)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("kw,msg", [
    (dict(C=0), "C = 0"), (dict(C=_C.KGE_CHUNK_MAX_C + 1), "C = "),
    (dict(M=_C.KGE_CHUNK_MAX_M + 1), "M = "), (dict(M=0), "M = 0"),
    (dict(n_neg=5), "neg and dneg"), (dict(D=7), "D = 7")])
def test_raw_guards(device, kw, msg):
    args = _raw_args(device, **kw)
    with pytest.raises(RuntimeError, match=msg):
        _C.kge_complex_step_chunk(*args)
    _sync(device)
    assert all(bool((t == 7.0).all()) for t in args[4:9]), "a refused call wrote its outputs"


@GPU
def test_raw_guard_d12_on_gpu():
    with pytest.raises(RuntimeError, match="D = 12"):
        _C.kge_complex_step_chunk(*_raw_args("cuda:0", D=12))
    _C.kge_complex_step_chunk(*_raw_args("cpu", D=12))  # the CPU twin takes any even D


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("C,M,D,n_neg,n_r,msg", [
    (0, 3, 8, 6, 4, "C = 0"), (65, 3, 8, 3, 4, "C = 65"), (2, 257, 8, 514, 4, "M = 257"),
    (2, 3, 12, 6, 4, "D = 12"), (2, 3, 8, 5, 4, "keys_neg"), (2, 3, 8, 6, 3, "disagree")])
def test_fused_guards(device, C, M, D, n_neg, n_r, msg):
    """Arguments are checked before the store is looked at: a CPU store
    refuses the bad call for the same reason as the GPU store."""
    st = Store(40, D, seed=7000, device=device)
    try:
        k = torch.arange(40)
        with pytest.raises(RuntimeError, match=msg):
            st.server.raw.kge_step_chunk_fused(k[:4], k[4:4 + n_r], k[8:12],
                                               k[12:12 + n_neg].contiguous(), C, M, D, LR, EPS)
        assert torch.equal(st.pull_all().view(torch.int32), st.snapshot.view(torch.int32))
    finally:
        st.close()


@pytest.mark.parametrize("field", ["neg_samples_subject", "gamma_entity", "gamma_relation",
                                   "dropout_entity", "dropout_relation"])
def test_config_guards(field):
    from adapm_amd.models.kge import ComplEx, ComplExConfig, Rescal

    with pytest.raises(ValueError, match=field):
        ComplEx(ComplExConfig(neg_chunk=4, **{field: 1}), None, None)
    with pytest.raises(ValueError, match="neg_chunk"):
        Rescal(ComplExConfig(neg_chunk=4), None, None)
