"""Every step, scoring and loss kernel against the fp64 references of
tests/step_refs.py, at the sizes and regimes where a kernel can go wrong:
every lanes-per-thread instantiation and the lane counts around their
boundaries, partial waves, N = 0, fresh (all-zero) accumulators, saturated
scores, the grid-stride loops, the MFMA tile edges, and the fused slab-direct
steps including rows whose padded length differs from their length.

Each case runs on the CPU twin and, marked `gpu`, on the HIP kernel. One half
of one output tensor is compared at a time with step_refs.assert_half_close:
err = max|got - ref64| / max|ref64| must stay within 16 * max(e32, 2^-23),
where e32 is the same error of the fp32 evaluation of the reference for that
very case. Outputs are prefilled with NaN and followed by a sentinel row.

Largest err / max(e32, 2^-23) observed per family (bound: 16; the raw err / e32
that every case also prints is larger only where e32 is below 2^-23):

    family                          CPU twin   MI355X
    kge_complex_step                  3.38      2.92
    w2v_sgns_step                     1.57      2.15
    mf_update_step                    1.15      2.77
    rescal_step                       1.55      4.38
    rescal_step_grouped                 -       4.23
    kge_complex_score, D % 4 != 0     1.33      1.00   (VALU scorer on the GPU)
    kge_complex_score, D % 4 == 0     4.53      1.40   (MFMA scorer on the GPU)
    mf_loss                           0.70      0.52
    kge_step_fused                      -       1.25
    w2v_step_fused                      -       1.97
    mf_step_fused                       -       1.41

mf_loss on the GPU read 15.6 at (B, R) = (16400, 1) while k_mf_loss added its
16384 per-workgroup shares with fp32 atomics, in whatever order they arrived;
it sums in double now. No other case came near the bound.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import step_refs as sr
from adapm_amd import _C

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda:0", id="gpu", marks=pytest.mark.gpu)]
GPU = pytest.mark.gpu

LANES = [1, 63, 64, 65, 255, 256, 257, 512, 513, 1024, 1025, 2047, 2048]
REGIME_LANES = [65, 2048]
LR, EPS, LAM = 0.05, 1e-6, 0.05
# |psi| targets of regime (b): below 1 and inside (20, 90), where softplusf
# has switched branch and __expf runs into its limits
PSI_TARGETS = [0.4, 30.0, 0.8, 60.0, 85.0, 22.0, 0.05, 45.0]


def _fam(name, device):
    return f"{name}[{'cpu' if device == 'cpu' else 'gpu'}]"


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _rows(g, n, L, scale=0.3, acc=0.1):
    """[n][2L] store rows: N(0, scale^2) embeddings | U(0, acc) accumulators."""
    a = torch.rand(n, L, generator=g) * acc if acc else torch.zeros(n, L)
    return torch.cat([torch.randn(n, L, generator=g) * scale, a], dim=1)


def _straddles_eps(ref64, names):
    for n in names:
        g2 = ref64[n][1]
        assert (g2 < EPS).any() and (g2 > EPS).any(), \
            f"regime (a): g^2 of {n} in [{g2.min():.3g}, {g2.max():.3g}] does not straddle eps"


def _psi_spread(ref64):
    a = ref64["psi"].abs()
    assert (a < 1).any() and ((a > 20) & (a < 90)).any(), f"regime (b): |psi| = {a.flatten().tolist()}"


def _scale_objects(psi, B, N, L, pos, neg):
    """Rescale the object rows' embeddings (psi is linear in them) so that
    |psi| cycles through PSI_TARGETS."""
    tgt = torch.tensor([PSI_TARGETS[i % len(PSI_TARGETS)] for i in range(B * (N + 1))],
                       dtype=torch.float64).view(B, N + 1)
    f = (tgt / psi.abs()).float()
    pos[:, :L] *= f[:, :1]
    neg.view(B, N, -1)[:, :, :L] *= f[:, 1:, None]


# ------------------------------------------------------------ cases
#
# A case is built once (inputs, fp64 and fp32 reference) and shared by the
# CPU and GPU twins of a test; nothing modifies it afterwards.

@functools.lru_cache(maxsize=8)
def complex_case(B, N, L, regime=None):
    D = 2 * L
    g = torch.Generator().manual_seed(1000 + L)
    scale, acc = (0.04, 0.0) if regime == "a" else (0.3, 0.1)
    s, r, o, neg = (_rows(g, n, D, scale, acc) for n in (B, B, B, B * N))
    if regime == "b":
        psi = sr.complex_ref(s, r, o, neg, N, D, LR, EPS, torch.float64)["psi"]
        _scale_objects(psi, B, N, D, o, neg)
    ref64, ref32 = (sr.complex_ref(s, r, o, neg, N, D, LR, EPS, dt)
                    for dt in (torch.float64, torch.float32))
    if regime == "a":
        _straddles_eps(ref64, ["s", "r", "o", "neg"])
    if regime == "b":
        _psi_spread(ref64)
    return (s, r, o, neg), ref64, ref32


@functools.lru_cache(maxsize=8)
def sgns_case(B, N, L, regime=None):
    g = torch.Generator().manual_seed(2000 + L)
    scale, acc = (2e-3, 0.0) if regime == "a" else (0.3, 0.1)
    ctr, ctx, neg = (_rows(g, n, L, scale, acc) for n in (B, B, B * N))
    if regime == "b":
        psi = sr.sgns_ref(ctr, ctx, neg, N, L, LR, EPS, torch.float64)["psi"]
        _scale_objects(psi, B, N, L, ctx, neg)
    ref64, ref32 = (sr.sgns_ref(ctr, ctx, neg, N, L, LR, EPS, dt)
                    for dt in (torch.float64, torch.float32))
    if regime == "a":
        _straddles_eps(ref64, ["ctr", "ctx", "neg"])
    if regime == "b":
        _psi_spread(ref64)
    return (ctr, ctx, neg), ref64, ref32


@functools.lru_cache(maxsize=8)
def mf_case(B, L, regime=None):
    g = torch.Generator().manual_seed(3000 + L)
    scale, acc = (5e-4, 0.0) if regime == "a" else (0.3, 0.1)
    w, h = _rows(g, B, L, scale, acc), _rows(g, B, L, scale, acc)
    x = torch.randn(B, generator=g)
    ref64, ref32 = (sr.mf_ref(w, h, x, L, LR, LAM, EPS, dt) for dt in (torch.float64, torch.float32))
    if regime == "a":
        _straddles_eps(ref64, ["w", "h"])
    return (w, h, x), ref64, ref32


@functools.lru_cache(maxsize=8)
def rescal_case(B, N, D):
    g = torch.Generator().manual_seed(4000 + D)
    s, o, neg = (_rows(g, n, D) for n in (B, B, B * N))
    r = _rows(g, B, D * D, scale=0.1)
    ref64, ref32 = (sr.rescal_ref(s, r, o, neg, N, D, LR, EPS, dt)
                    for dt in (torch.float64, torch.float32))
    return (s, r, o, neg), ref64, ref32


# ------------------------------------------------------------ runners

def _run_step(device, fn, ins, out_rows, n_loss, tail, ref64, ref32, what, family):
    """Call a classic step `fn(*inputs, *outputs, loss, *tail)` on guarded
    outputs shaped like `out_rows` ({name: input tensor}) and compare."""
    bufs = {n: sr.Guarded(t.shape[0], t.shape[1], device) for n, t in out_rows.items()}
    loss = sr.guarded_vec(n_loss, device)
    fn(*[t.to(device) for t in ins], *[b.out for b in bufs.values()], loss.out, *tail)
    _sync(device)
    got = {n: b.out for n, b in bufs.items()}
    got["loss"] = loss.out
    sr.assert_step_close(got, ref64, ref32, what, family)
    for n, b in {**bufs, "loss": loss}.items():
        b.check(f"{what} {n}")


def run_complex(device, B, N, L, regime=None):
    (s, r, o, neg), ref64, ref32 = complex_case(B, N, L, regime)
    _run_step(device, _C.kge_complex_step, (s, r, o, neg), {"s": s, "r": r, "o": o, "neg": neg}, B,
              (N, 2 * L, LR, EPS), ref64, ref32, f"complex B={B} N={N} L={L} {regime or ''}",
              _fam("complex", device))


def run_sgns(device, B, N, L, regime=None):
    (ctr, ctx, neg), ref64, ref32 = sgns_case(B, N, L, regime)
    _run_step(device, _C.w2v_sgns_step, (ctr, ctx, neg), {"ctr": ctr, "ctx": ctx, "neg": neg}, B,
              (N, L, LR, EPS), ref64, ref32, f"sgns B={B} N={N} L={L} {regime or ''}",
              _fam("sgns", device))


def run_mf(device, B, L, regime=None):
    (w, h, x), ref64, ref32 = mf_case(B, L, regime)
    _run_step(device, _C.mf_update_step, (w, h, x), {"w": w, "h": h}, B, (L, LR, LAM, EPS),
              ref64, ref32, f"mf B={B} L={L} {regime or ''}", _fam("mf", device))


def run_rescal(device, B, N, D):
    (s, r, o, neg), ref64, ref32 = rescal_case(B, N, D)
    _run_step(device, _C.rescal_step, (s, r, o, neg), {"s": s, "r": r, "o": o, "neg": neg}, B,
              (N, D, LR, EPS), ref64, ref32, f"rescal B={B} N={N} D={D}", _fam("rescal", device))


# ------------------------------------------------------------ classic steps

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("L", LANES)
def test_complex_step_lanes(device, L):
    run_complex(device, 3, 2, L)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("L", LANES)
def test_sgns_step_lanes(device, L):
    run_sgns(device, 3, 2, L)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("L", LANES)
def test_mf_step_lanes(device, L):
    run_mf(device, 3, L)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("N", [0, 1, 3])
@pytest.mark.parametrize("L", [65, 2048])
def test_complex_step_negatives(device, L, N):
    run_complex(device, 4, N, L)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("N", [0, 1, 3])
@pytest.mark.parametrize("L", [65, 2048])
def test_sgns_step_negatives(device, L, N):
    run_sgns(device, 4, N, L)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("L", REGIME_LANES)
def test_complex_step_regimes(device, L, regime):
    """(a) fresh rows: accumulators 0, g^2 on both sides of eps;
    (b) |psi| both below 1 and in (20, 90)."""
    run_complex(device, 4, 3, L, regime)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("regime", ["a", "b"])
@pytest.mark.parametrize("L", REGIME_LANES)
def test_sgns_step_regimes(device, L, regime):
    run_sgns(device, 4, 3, L, regime)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("L", REGIME_LANES)
def test_mf_step_fresh_rows(device, L):
    """Regime (a); MF has no logistic term, so there is no regime (b)."""
    run_mf(device, 4, L, "a")


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("kernel", ["complex", "sgns", "mf"])
def test_step_grid_stride(device, kernel):
    """More samples than the launch has workgroups (cap 16384)."""
    B = 16400
    if kernel == "complex":
        run_complex(device, B, 1, 1)
    elif kernel == "sgns":
        run_sgns(device, B, 1, 1)
    else:
        run_mf(device, B, 1)


# ------------------------------------------------------------ RESCAL per triple

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [1, 5, 64, 65, 128, 196])
def test_rescal_step_dims(device, D):
    """Up to the documented limit D = 196 (R staged in 156,032 B of LDS)."""
    run_rescal(device, 3, 2, D)


@pytest.mark.parametrize("device", DEVICES)
def test_rescal_step_grid_stride(device):
    run_rescal(device, 8200, 1, 4)  # cap 8192


# ------------------------------------------------------------ RESCAL grouped

@functools.lru_cache(maxsize=2)
def grouped_case(sizes, N, D):
    starts = np.cumsum((0,) + sizes).astype(np.int32)
    B, G = int(starts[-1]), len(sizes)
    g = torch.Generator().manual_seed(5000 + D + G)
    s, o, neg = (_rows(g, n, D) for n in (B, B, B * N))
    rm = _rows(g, G, D * D, scale=0.1)
    ref64, ref32 = (sr.rescal_grouped_ref(s, rm, starts, o, neg, N, D, LR, EPS, dt)
                    for dt in (torch.float64, torch.float32))
    return (s, rm, o, neg), starts, ref64, ref32


def run_grouped(sizes, N, D):
    device = "cuda:0"
    (s, rm, o, neg), starts, ref64, ref32 = grouped_case(tuple(sizes), N, D)
    bufs = {n: sr.Guarded(t.shape[0], t.shape[1], device)
            for n, t in (("s", s), ("r", rm), ("o", o), ("neg", neg))}
    loss = _C.rescal_step_grouped(*[t.to(device) for t in (s, rm, o, neg)],
                                  *[b.out for b in bufs.values()], torch.from_numpy(starts),
                                  N, D, LR, EPS)
    _sync(device)
    got = {n: b.out for n, b in bufs.items()}
    got["loss"] = loss
    what = f"rescal_grouped G={len(sizes)} B={sum(sizes)} max={max(sizes)} D={D}"
    sr.assert_step_close(got, ref64, ref32, what, "rescal_grouped[gpu]")
    for n, b in bufs.items():
        b.check(f"{what} {n}")
    dr = bufs["r"].out.cpu()
    for gi, size in enumerate(sizes):
        if size == 0:
            assert not dr[gi].any(), f"{what}: dR of empty group {gi} is not [0 | 0]"


@GPU
@pytest.mark.parametrize("D", [4, 20, 32, 68, 128])
def test_rescal_grouped_dims(D):
    """Groups of 0, 1, 17 (> one m-tile) and 40 (> a K chunk) rows; D below,
    at and above one n-tile and not a multiple of 16."""
    run_grouped([0, 1, 17, 40, 3], 2, D)


@GPU
def test_rescal_grouped_grid_stride():
    run_grouped([8200], 1, 4)  # cap 8192 of the per-triple middle phase


@GPU
def test_rescal_grouped_adagrad_grid_stride():
    """130 relation matrices of 128 x 128 are 2,129,920 values, past the
    8192 x 256 threads of the AdaGrad epilogue; all but two groups are empty."""
    run_grouped([0] * 60 + [1] + [0] * 60 + [2] + [0] * 8, 2, 128)


# ------------------------------------------------------------ scoring

def run_score(device, B, E, D, family):
    g = torch.Generator().manual_seed(6000 + 7 * D + B + E)
    s, r, cand = _rows(g, B, D), _rows(g, B, D), _rows(g, E, D)
    ref64, ref32 = (sr.complex_score_ref(s, r, cand, D, dt) for dt in (torch.float64, torch.float32))
    out = sr.Guarded(B, E, device)
    _C.kge_complex_score(s.to(device), r.to(device), cand.to(device), out.out, D)
    _sync(device)
    what = f"score B={B} E={E} D={D}"
    sr.assert_half_close(out.out, ref64, ref32, what, _fam(family, device))
    out.check(what)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [2, 6, 130, 514])
def test_score_valu(device, D):
    """D % 4 != 0: the VALU scorer on the GPU."""
    for B, E in itertools.product([1, 17], [1, 255, 257]):
        run_score(device, B, E, D, "score_valu")


@pytest.mark.parametrize("device", DEVICES)
def test_score_valu_grid_stride(device):
    run_score(device, 129, 128, 6, "score_valu")  # B * E = 16512 > 16384


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [4, 12, 20])
def test_score_mfma_partial_chunk(device, D):
    """D % 4 == 0 but not a multiple of the MFMA kernel's K chunk of 16."""
    for B, E in itertools.product([1, 17], [1, 255, 257]):
        run_score(device, B, E, D, "score_mfma")


# ------------------------------------------------------------ mf_loss

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("B,R", [(1, 1), (4097, 128), (16400, 1), (3, 257)])
def test_mf_loss(device, B, R):
    g = torch.Generator().manual_seed(7000 + B + R)
    w, h = torch.randn(B, 2 * R, generator=g), torch.randn(B, 2 * R, generator=g)
    x = torch.randn(B, generator=g)
    ref64, ref32 = (sr.mf_loss_ref(w, h, x, R, 0.02, dt) for dt in (torch.float64, torch.float32))
    got = _C.mf_loss(w.to(device), h.to(device), x.to(device), R, 0.02)
    _sync(device)
    for i, part in enumerate(("se", "reg")):
        sr.assert_half_close(got[i:i + 1], ref64[i:i + 1], ref32[i:i + 1],
                             f"mf_loss B={B} R={R} {part}", _fam("mf_loss", device))


# ------------------------------------------------------------ alias draw

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("N", [0, 1, 4096 * 256 + 7])
@pytest.mark.parametrize("n", [1, 5, 1000003])
def test_alias_draw(device, n, N):
    """Device draw == CPU twin == the counter hash written in numpy; the
    largest N is one grid-stride pass plus 7 draws."""
    g = torch.Generator().manual_seed(8000 + n)
    prob = torch.rand(n, generator=g)
    alias = torch.randint(0, n, (n,), generator=g, dtype=torch.int32)
    seed = 0x5DEECE66D + n
    want = sr.alias_draw_ref(prob, alias, seed, N)
    got = _C.alias_draw(prob.to(device), alias.to(device), seed, N)
    _sync(device)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), want)
    if device != "cpu":
        assert torch.equal(got.cpu(), _C.alias_draw(prob, alias, seed, N))


# ------------------------------------------------------------ fused steps
#
# Server.*_step_fused at world == 1, all keys unique: the store afterwards
# must be snapshot + fp64 deltas on the named rows, per half, and bit-identical
# everywhere else.

SPARE_ROWS = 7


class FusedStore:
    def __init__(self, n_named, L, seed):
        import adapm_amd

        adapm_amd._SETUP.clear()
        adapm_amd.runtime._RUNTIME = None
        self.num_keys, self.L = n_named + SPARE_ROWS, L
        adapm_amd.setup(num_keys=self.num_keys, num_threads=1, device="cuda:0")
        self.server = adapm_amd.Server(2 * L)
        self.worker = adapm_amd.Worker(0, self.server)
        g = torch.Generator().manual_seed(seed)
        self.worker.set(np.arange(self.num_keys, dtype=np.int64), _rows(g, self.num_keys, L).cuda())
        # named keys in a random order, SPARE_ROWS keys left alone
        self.keys = torch.randperm(self.num_keys, generator=g)[:n_named]
        self.snapshot = self.pull_all()

    def pull_all(self):
        out = torch.empty(self.num_keys, 2 * self.L, device="cuda")
        self.worker.pull(np.arange(self.num_keys, dtype=np.int64), out)
        torch.cuda.synchronize()
        return out.cpu()

    def take(self, n):
        k, self.keys = self.keys[:n].contiguous(), self.keys[n:]
        return k

    def check(self, roles, loss, ref64, ref32, what, family):
        """roles: {name: keys} in the reference's naming."""
        torch.cuda.synchronize()
        after, snap, L = self.pull_all(), self.snapshot, self.L
        sr.assert_half_close(loss, ref64["loss"], ref32["loss"], f"{what} loss", family)
        touched = torch.zeros(self.num_keys, dtype=torch.bool)
        for name, keys in roles.items():
            touched[keys] = True
            for half, part in ((0, "emb"), (1, "acc")):
                cols = slice(half * L, (half + 1) * L)
                before = snap[keys][:, cols]
                sr.assert_half_close(after[keys][:, cols], before.double() + ref64[name][half],
                                     before + ref32[name][half], f"{what} {name}.{part}", family)
        assert int(touched.sum()) == self.num_keys - SPARE_ROWS
        assert torch.equal(after[~touched].view(torch.int32), snap[~touched].view(torch.int32)), \
            f"{what}: a row that the batch does not name changed"

    def close(self):
        self.worker.finalize()
        self.server.shutdown()


def run_fused_complex(B, N, D):
    st = FusedStore(B * (3 + N), D, seed=9000 + D)
    try:
        ks, kr, ko, kn = st.take(B), st.take(B), st.take(B), st.take(B * N)
        ins = [st.snapshot[k] for k in (ks, kr, ko, kn)]
        ref64, ref32 = (sr.complex_ref(*ins, N, D, LR, EPS, dt) for dt in (torch.float64, torch.float32))
        loss = st.server.raw.kge_step_fused(ks, kr, ko, kn, N, D, LR, EPS)
        st.check({"s": ks, "r": kr, "o": ko, "neg": kn}, loss, ref64, ref32,
                 f"fused complex B={B} N={N} D={D}", "fused_complex[gpu]")
    finally:
        st.close()


def run_fused_sgns(B, N, D):
    st = FusedStore(B * (2 + N), D, seed=9100 + D)
    try:
        kc, kx, kn = st.take(B), st.take(B), st.take(B * N)
        ins = [st.snapshot[k] for k in (kc, kx, kn)]
        ref64, ref32 = (sr.sgns_ref(*ins, N, D, LR, EPS, dt) for dt in (torch.float64, torch.float32))
        loss = st.server.raw.w2v_step_fused(kc, kx, kn, N, D, LR, EPS)
        st.check({"ctr": kc, "ctx": kx, "neg": kn}, loss, ref64, ref32,
                 f"fused sgns B={B} N={N} D={D}", "fused_sgns[gpu]")
    finally:
        st.close()


def run_fused_mf(B, R):
    st = FusedStore(2 * B, R, seed=9200 + R)
    try:
        kw, kh = st.take(B), st.take(B)
        x = torch.randn(B, generator=torch.Generator().manual_seed(R))
        ref64, ref32 = (sr.mf_ref(st.snapshot[kw], st.snapshot[kh], x, R, LR, LAM, EPS, dt)
                        for dt in (torch.float64, torch.float32))
        loss = st.server.raw.mf_step_fused(kw, kh, x, R, LR, LAM, EPS)
        st.check({"w": kw, "h": kh}, loss, ref64, ref32, f"fused mf B={B} R={R}", "fused_mf[gpu]")
    finally:
        st.close()


@GPU
@pytest.mark.parametrize("D", [130, 514, 2050, 4096])  # 1, 2, 8 and 8 lanes per thread
def test_fused_complex(D):
    run_fused_complex(3, 2, D)


@GPU
@pytest.mark.parametrize("D", [65, 301, 513, 2048])  # D = 301: rows of 602 floats, padded to 604
def test_fused_sgns(D):
    run_fused_sgns(3, 2, D)


@GPU
@pytest.mark.parametrize("R", [33, 257, 600])  # R = 33: rows of 66 floats, padded to 68
def test_fused_mf(R):
    run_fused_mf(3, R)


@GPU
def test_fused_sgns_grid_stride():
    run_fused_sgns(16400, 1, 2)


@GPU
def test_fused_mf_grid_stride():
    run_fused_mf(16400, 1)
