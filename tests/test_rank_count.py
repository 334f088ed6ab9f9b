"""_C.rank_count and _C.pair_scores (k_mfma_rank_count, k_mfma_pair_scores and
their CPU twins) against the fp64 references of tests/rank_refs.py. Each case
runs on the CPU twin and, marked `gpu`, on the HIP kernels.

Exact inputs. Q and C come from {-8..8} / 8, Q as ComplEx-style queries of
two such rows, so every product and partial sum is exact in fp32 (the tests
assert that the fp64 scores survive fp32) and the counts must EQUAL the
reference. Ties with base are common on this grid and test the strict `>`;
the tie cases assert that they hold a tied candidate other than the true one.
Shapes: every (B, E) of B in {1, 15, 16, 17, 33} x E in {1, 255, 256, 257,
515} for every K in {1, 3, 4, 15, 16, 17, 36, 64, 130} and every candidate
stride in {K, 2K, 2K + 4}, always with qstride > K and non-zero starting
counts; E == 0 and B == 0; a split of E; max_blocks 1 and 3.

Consistency. With standard-normal inputs rank_count must return, for every
row, exactly the number of pair_scores strictly above the pair score chosen
as base: the two entry points agree bit for bit, with no tolerance.

Tolerance. N(0, 0.3^2) rows, ComplEx-style queries, S the fp64 scores:
delta = 2 * 16 * max(e32, 2^-23) * max|S|, e32 the relative error of the fp32
evaluation of the reference (the rule of test_kernel_reference, doubled
because score and base both carry error). lo[b] <= counts[b] <= hi[b], lo
counting S > base + delta and hi S > base - delta, the true candidate in
neither. Before looking at the kernel the test asserts that at most a quarter
of the rows have lo != hi and none has hi - lo > 2.

Observed (every case prints its figures before it asserts):

    (B, E, K)          e32        rows lo != hi   largest |got - nearest bound|
                                                  CPU twin   MI355X
    (33, 1000, 64)     3.12e-07   1 of 33            0          0
    (17, 515, 36)      2.31e-07   0 of 17            0          0
    (40, 2000, 128)    3.36e-07   3 of 40            1          1

(the largest hi - lo is 2, in the last case). Tie cases: 10, 2 and 10
candidates tied with base other than the true one at (17, 300, 4),
(17, 300, 8) and (33, 515, 36).
"""
import functools

import numpy as np
import pytest
import torch

import rank_refs as rr
from adapm_amd import _C

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda:0", id="gpu", marks=pytest.mark.gpu)]

BS = [1, 15, 16, 17, 33]
ES = [1, 255, 256, 257, 515]
KS = [1, 3, 4, 15, 16, 17, 36, 64, 130]
CSTRIDES = {"K": lambda K: K, "2K": lambda K: 2 * K, "2K+4": lambda K: 2 * K + 4}
QPAD = 3  # qstride = query length + QPAD > K


def _dev(x, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(device)


def _strided(mat, stride, device, fill=np.nan):
    """[n][stride] device tensor holding mat in its first columns and `fill`
    behind them: the kernel must not read past K."""
    n, k = mat.shape
    full = np.full((n, stride), fill, dtype=np.float32)
    full[:, :k] = mat
    return _dev(full, device)


def _rank_count(Q, C, base, counts0, K, device, qstride=None, cstride=None, max_blocks=0):
    """Run rank_count on fp32 copies of Q[:, :K], C[:, :K] laid out with the
    given strides; returns the counts as numpy."""
    q = _strided(np.asarray(Q, np.float32)[:, :K], qstride or K + QPAD, device)
    c = _strided(np.asarray(C, np.float32)[:, :K], cstride or K, device)
    counts = _dev(counts0, device, torch.int32)
    _C.rank_count(q, c, _dev(base, device, torch.float32), counts, K, max_blocks)
    return counts.cpu().numpy()


def _pair_scores(Q, C, owner, K, device, qstride=None, cstride=None):
    q = _strided(np.asarray(Q, np.float32)[:, :K], qstride or K + QPAD, device)
    c = _strided(np.asarray(C, np.float32)[:, :K], cstride or K, device)
    out = torch.full((len(owner),), float("nan"), dtype=torch.float32, device=device)
    _C.pair_scores(q, c, torch.as_tensor(np.asarray(owner), dtype=torch.int32), out, K)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def exact_case(K, seed=0, B=max(BS), E=max(ES)):
    """Grid queries (ComplEx-style, first K floats of an even-length query),
    grid candidates, their fp64 scores; shared by every sub-shape."""
    rng = np.random.default_rng(7000 + 13 * K + seed)
    L = K + (K & 1)
    Q = rr.complex_query(rr.grid(rng, (B, L)), rr.grid(rng, (B, L)), "o")[:, :K]
    C = rr.grid(rng, (E, K))
    S = rr.scores(Q, C, K)
    assert rr.exact_in_fp32(Q) and rr.exact_in_fp32(S)
    for a in (Q, C, S):
        a.setflags(write=False)
    return Q, C, S


def _true_of(B, E):
    return (5 * np.arange(B) + 1) % E


def _start_counts(B):
    return (3 * np.arange(B) + 1).astype(np.int32)


# ------------------------------------------------------------ exact inputs

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("cs", list(CSTRIDES))
@pytest.mark.parametrize("K", KS)
def test_exact_counts_every_shape(K, cs, device):
    Q, C, S = exact_case(K)
    for B in BS:
        for E in ES:
            t = _true_of(B, E)
            base = S[np.arange(B), t]
            ref = _start_counts(B) + rr.count_above(S[:B, :E], base)
            got = _rank_count(Q[:B], C[:E], base, _start_counts(B), K, device,
                              cstride=CSTRIDES[cs](K))
            assert np.array_equal(got, ref), (B, E, K, cs, got.tolist(), ref.tolist())


TIE_CASES = [(17, 300, 4), (17, 300, 8), (33, 515, 36)]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("B,E,K", TIE_CASES)
def test_exact_counts_ties(B, E, K, device):
    Q, C, S = exact_case(K, seed=1, B=B, E=E)
    t = _true_of(B, E)
    base = S[np.arange(B), t]
    tied = S == base[:, None]
    tied[np.arange(B), t] = False
    print(f"ties[{B},{E},{K}]: {int(tied.sum())} candidates tied with base, not the true one")
    assert tied.any()
    ref = rr.count_above(S, base)
    got = _rank_count(Q, C, base, np.zeros(B, np.int32), K, device, cstride=2 * K)
    assert np.array_equal(got, ref), (got.tolist(), ref.tolist())
    # a tied candidate counted by mistake would show as got > ref: the
    # comparison is strict
    assert (ref < E).all()


@pytest.mark.parametrize("device", DEVICES)
def test_empty_sides_leave_counts(device):
    Q, C, S = exact_case(36)
    start = _start_counts(17)
    got = _rank_count(Q[:17], C[:0], S[:17, 0], start, 36, device)
    assert np.array_equal(got, start)
    got = _rank_count(Q[:0], C[:300], np.zeros(0), np.zeros(0, np.int32), 36, device)
    assert got.shape == (0,)
    assert _pair_scores(Q[:17], C[:0], np.zeros(0, np.int32), 36, device).shape == (0,)


@pytest.mark.parametrize("device", DEVICES)
def test_split_of_candidates_adds_up(device):
    B, E, K = 33, 515, 36
    Q, C, S = exact_case(K)
    base = S[np.arange(B), _true_of(B, E)]
    whole = _rank_count(Q, C, base, _start_counts(B), K, device, cstride=2 * K)
    part = _rank_count(Q, C[:259], base, _start_counts(B), K, device, cstride=2 * K)
    part = _rank_count(Q, C[259:], base, part, K, device, cstride=2 * K)
    assert np.array_equal(part, whole)
    assert np.array_equal(whole, _start_counts(B) + rr.count_above(S, base))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("max_blocks", [1, 3])
def test_one_workgroup_walks_many_tiles(max_blocks, device):
    B, E, K = 33, 515, 36
    Q, C, S = exact_case(K)
    base = S[np.arange(B), _true_of(B, E)]
    got = _rank_count(Q, C, base, _start_counts(B), K, device, cstride=2 * K + 4,
                      max_blocks=max_blocks)
    assert np.array_equal(got, _start_counts(B) + rr.count_above(S, base))


# ------------------------------------------------------------ NaN and infinities

@pytest.mark.parametrize("device", DEVICES)
def test_nan_and_infinities(device):
    B, E, K = 17, 300, 4
    rng = np.random.default_rng(11)
    Q = 0.5 + np.abs(rr.grid(rng, (B, K))) / 2  # positive: inf * q keeps its sign
    C = rr.grid(rng, (E, K))
    S0 = rr.scores(Q, C, K)
    plain = rr.count_above(S0, np.zeros(B))
    C[3] = np.inf       # +inf score for every row
    C[290, 0] = -np.inf  # -inf score
    C[297, 1] = np.nan   # NaN score
    S = rr.scores(Q, C, K)
    assert np.isposinf(S[:, 3]).all() and np.isneginf(S[:, 290]).all() and \
        np.isnan(S[:, 297]).all()
    base = np.zeros(B)
    base[1] = np.inf     # counts only the NaN
    base[2] = -np.inf    # counts everything but the -inf score
    ref = rr.count_above(S, base)
    assert ref[1] == 1 and ref[2] == E - 1
    got = _rank_count(Q, C, base, np.zeros(B, np.int32), K, device, cstride=2 * K)
    assert np.array_equal(got, ref), (got.tolist(), ref.tolist())
    # against the same case without the three special rows: the NaN row adds
    # one to every row's count, the +inf row counts, the -inf row does not
    was = (S0[:, [3, 290, 297]] > 0).sum(1)
    assert np.array_equal(got[3:], (plain - was + 2)[3:])


# ------------------------------------------------------------ the two entry points

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("B,E,K", [(33, 515, 36), (17, 257, 130)])
def test_pair_scores_are_the_scores_rank_count_compares(B, E, K, device):
    rng = np.random.default_rng(500 + K)
    Q = rng.standard_normal((B, K)).astype(np.float32)
    C = rng.standard_normal((E, K)).astype(np.float32)
    owner = np.repeat(np.arange(B), E)
    P = _pair_scores(Q, np.tile(C, (B, 1)), owner, K, device, cstride=K + 1).reshape(B, E)
    assert np.isfinite(P).all()
    assert rr.rel_err(P, rr.scores(Q, C, K)) < 1e-5  # it is the score at all
    t = _true_of(B, E)
    base = P[np.arange(B), t]
    expect = (P > base[:, None]).sum(1)
    got = _rank_count(Q, C, base, np.zeros(B, np.int32), K, device, cstride=2 * K)
    assert np.array_equal(got, expect), (got.tolist(), expect.tolist())
    # and with the candidates walked by one workgroup, in another tile order
    got = _rank_count(Q, C, base, np.zeros(B, np.int32), K, device, cstride=K, max_blocks=1)
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("device", DEVICES)
def test_pair_scores_exact(device):
    B, E, K = 33, 515, 36
    Q, C, S = exact_case(K)
    owner = (7 * np.arange(E) + 2) % B
    got = _pair_scores(Q, C, owner, K, device, cstride=2 * K + 4)
    assert np.array_equal(got.astype(np.float64), S[owner, np.arange(E)])


# ------------------------------------------------------------ fp64 with a tolerance

@functools.lru_cache(maxsize=None)
def tolerance_case(B, E, K):
    rng = np.random.default_rng(900 + K)
    rows = lambda n: (rng.standard_normal((n, K)) * 0.3).astype(np.float32)
    Q = rr.complex_query(rows(B), rows(B), "o")  # fp32, as the model builds it
    C = rows(E)
    S = rr.scores(Q, C, K)
    e32 = rr.rel_err(Q @ C.T, S)
    delta = 2 * 16 * max(e32, 2.0 ** -23) * np.abs(S).max()
    t = _true_of(B, E)
    base = S[np.arange(B), t]
    others = np.ones_like(S, dtype=bool)
    others[np.arange(B), t] = False
    lo = ((S > base[:, None] + delta) & others).sum(1)
    hi = ((S > base[:, None] - delta) & others).sum(1)
    return Q, C, t, lo, hi, e32


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("B,E,K", [(33, 1000, 64), (17, 515, 36), (40, 2000, 128)])
def test_counts_within_fp64_bounds(B, E, K, device):
    Q, C, t, lo, hi, e32 = tolerance_case(B, E, K)
    ambiguous = int((lo != hi).sum())
    print(f"bounds[{B},{E},{K}]: e32 {e32:.3g}, rows lo != hi {ambiguous} of {B}, "
          f"max hi - lo {int((hi - lo).max())}")
    assert 4 * ambiguous <= B and (hi - lo).max() <= 2  # on the reference alone
    base = _pair_scores(Q, C[t], np.arange(B), K, device, cstride=2 * K)
    got = _rank_count(Q, C, base, np.zeros(B, np.int32), K, device, cstride=2 * K)
    off = np.minimum(np.abs(got - lo), np.abs(got - hi))
    print(f"bounds[{B},{E},{K}][{device}]: largest |got - nearest bound| {int(off.max())}")
    assert (lo <= got).all() and (got <= hi).all(), (got.tolist(), lo.tolist(), hi.tolist())


# ------------------------------------------------------------ argument checks

def test_argument_checks():
    q = torch.zeros(4, 8)
    c = torch.zeros(6, 8)
    base = torch.zeros(4)
    counts = torch.zeros(4, dtype=torch.int32)
    own = torch.zeros(6, dtype=torch.int32)
    out = torch.zeros(6)
    for bad in (lambda: _C.rank_count(q, c, base, counts, 0),
                lambda: _C.rank_count(q, c, base, counts, 9),
                lambda: _C.rank_count(q, c, base[:3], counts, 8),
                lambda: _C.rank_count(q, c, base, counts.float(), 8),
                lambda: _C.rank_count(q.double(), c, base, counts, 8),
                lambda: _C.rank_count(q.t().contiguous().t(), c, base, counts, 4),
                lambda: _C.pair_scores(q, c, own[:5], out, 8),
                lambda: _C.pair_scores(q, c, own + 4, out, 8),
                lambda: _C.pair_scores(q, c, own - 1, out, 8),
                lambda: _C.pair_scores(q, c, own.long(), out, 8)):
        with pytest.raises(RuntimeError):
            bad()
    _C.rank_count(q[:, :4], c[:, 2:7], base, counts, 4)  # row views are fine
