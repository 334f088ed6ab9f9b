"""fp64 references for the rank kernels and the three-sided KGE evaluation,
written from the definitions:

  rank_count   counts[b] = #{ e : S[b][e] > base[b] or S[b][e] is NaN },
               S = Q[:, :K] @ C[:, :K]^T
  pair_scores  out[p] = Q[owner[p], :K] . C[p, :K]
  ComplEx      psi(s, r, o) = sum_k (s_re r_re - s_im r_im) o_re
                                  + (s_im r_re + s_re r_im) o_im,
               rows [re(D/2) | im(D/2)]
  RESCAL       psi(s, R, o) = s^T R o, R row-major D x D
  ranks        raw rank = 1 + #{candidates scoring above the true triple,
               or NaN}; the filtered rank also leaves out the OTHER known
               subjects of (r, o) / objects of (s, r) that score strictly
               above it (a NaN one stays counted); a NaN true score makes
               all five ranks NaN.

Everything here is numpy in float64 and loops where a loop is clearest.
"""
import numpy as np

KINDS = ("s", "r", "o", "s_raw", "o_raw")


def grid(rng, shape):
    """Values from {-8..8} / 8: products and sums of a few thousand of them
    are exact in fp32."""
    return rng.integers(-8, 9, size=shape).astype(np.float64) / 8.0


def complex_query(a, b, side):
    """The ComplEx query of `side` from the two other rows ([re | im] each):
    side "o": a = s, b = r; side "s": a = r, b = o; side "r": a = s, b = o."""
    dc = a.shape[-1] // 2
    a_re, a_im, b_re, b_im = a[..., :dc], a[..., dc:], b[..., :dc], b[..., dc:]
    if side == "o":
        return np.concatenate([a_re * b_re - a_im * b_im, a_im * b_re + a_re * b_im], axis=-1)
    return np.concatenate([a_re * b_re + a_im * b_im, a_re * b_im - a_im * b_re], axis=-1)


def scores(Q, C, K):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(Q, np.float64)[:, :K] @ np.asarray(C, np.float64)[:, :K].T


def count_above(S, base):
    with np.errstate(invalid="ignore"):
        return ((S > np.asarray(base, np.float64)[:, None]) | np.isnan(S)).sum(1)


def exact_in_fp32(x):
    x = np.asarray(x, np.float64)
    return np.array_equal(x.astype(np.float32).astype(np.float64), x)


def rel_err(got, ref):
    """max|got - ref| / max|ref|, the error measure of test_kernel_reference."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------ scorers

def complex_score(s, r, o):
    """psi of rows s, r, o ([..., D] each, broadcast against each other)."""
    dc = s.shape[-1] // 2
    s_re, s_im, r_re, r_im = s[..., :dc], s[..., dc:], r[..., :dc], r[..., dc:]
    o_re, o_im = o[..., :dc], o[..., dc:]
    return ((s_re * r_re - s_im * r_im) * o_re + (s_im * r_re + s_re * r_im) * o_im).sum(-1)


def rescal_score(s, r, o):
    """s^T R o; r is [..., D*D] row-major."""
    D = s.shape[-1]
    Rm = r.reshape(r.shape[:-1] + (D, D))
    return np.einsum("...i,...ij,...j->...", s, Rm, o)


def brute_ranks(score, ent, rel, triples, filter_triples=None):
    """All five rank kinds of every triple by scoring every candidate in
    fp64. ent [E][D], rel [R][*] hold the embedding parts only."""
    known = set() if filter_triples is None else {tuple(int(x) for x in t)
                                                  for t in filter_triples}
    out = {k: np.zeros(len(triples)) for k in KINDS}
    with np.errstate(invalid="ignore"):
        for i, (s, r, o) in enumerate(np.asarray(triples).tolist()):
            base = score(ent[s], rel[r], ent[o])
            if np.isnan(base):
                for k in KINDS:
                    out[k][i] = np.nan
                continue
            S_s = score(ent, rel[r][None], ent[o][None])
            S_r = score(ent[s][None], rel, ent[o][None])
            S_o = score(ent[s][None], rel[r][None], ent)
            raw = {x: 1 + int(((S > base) | np.isnan(S)).sum())
                   for x, S in (("s", S_s), ("r", S_r), ("o", S_o))}
            other_s = {fs for (fs, fr, fo) in known if fr == r and fo == o and fs != s}
            other_o = {fo for (fs, fr, fo) in known if fs == s and fr == r and fo != o}
            out["s_raw"][i], out["o_raw"][i], out["r"][i] = raw["s"], raw["o"], raw["r"]
            out["s"][i] = raw["s"] - sum(1 for e in other_s if S_s[e] > base)
            out["o"][i] = raw["o"] - sum(1 for e in other_o if S_o[e] > base)
    return out
