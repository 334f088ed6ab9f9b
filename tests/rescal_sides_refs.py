"""High-precision reference of the RESCAL sides step, in the manner of
sides_refs.complex_sides_ref and step_refs._rescal: the objective is written
down, torch autograd differentiates it, and the AdaGrad transform is applied
per role. Nothing is shared with the kernels or their CPU twins.

One sample is a positive (s, R, o) with N object-side negatives (s, R, o'_j)
and NS subject-side negatives (s'_j, R, o), psi(s, R, o) = s^T R o with R
row-major D x D. The objective adds the L2 terms
0.5 * gamma_e * (|s|^2 + |o|^2) + 0.5 * gamma_r * |R|^2 of the positive's rows
to the 1 + N + NS logistic terms; the loss the step reports leaves them out.

Triple b scores with relation row rmat[gid[b]], so one function serves the
per-triple form (gid = 0..B-1) and the grouped form, where the gradient of a
matrix is summed over the triples that name it, each of them adding its own
gamma_r * R.
"""
import numpy as np
import torch

from step_refs import _f32, _halves, _leaf, _softplus


def _rescal_sides(s, rmat, gid, o, neg_o, neg_s, N, NS, D, lr, eps, gamma_e, gamma_r, dtype):
    lr, eps, gamma_e, gamma_r = (_f32(x) for x in (lr, eps, gamma_e, gamma_r))
    B = s.shape[0]
    se, oe, noe, nse = (_leaf(t, D, dtype) for t in (s, o, neg_o, neg_s))
    Re = _leaf(rmat, D * D, dtype)
    Rb = Re.view(-1, D, D)[gid]                                   # [B][D][D]
    objs = torch.cat([oe[:, None, :], noe.view(B, N, D)], dim=1)  # [B][1+N][D]
    psi_o = torch.einsum("bi,bik,bjk->bj", se, Rb, objs)
    psi_s = torch.einsum("bji,bik,bk->bj", nse.view(B, NS, D), Rb, oe)
    loss = _softplus(-psi_o[:, 0]) + _softplus(psi_o[:, 1:]).sum(1) + _softplus(psi_s).sum(1)
    reg = (0.5 * gamma_e * ((se * se).sum(1) + (oe * oe).sum(1))
           + 0.5 * gamma_r * (Rb * Rb).sum((1, 2)))
    (loss + reg).sum().backward()
    return {"loss": loss.detach(), "psi": torch.cat([psi_o, psi_s], dim=1).detach(),
            "s": _halves(s, se, D, lr, eps, dtype),
            "r": _halves(rmat, Re, D * D, lr, eps, dtype),
            "o": _halves(o, oe, D, lr, eps, dtype),
            "neg_o": _halves(neg_o, noe, D, lr, eps, dtype),
            "neg_s": _halves(neg_s, nse, D, lr, eps, dtype)}


def rescal_sides_ref(s, r, o, neg_o, neg_s, N, NS, D, lr, eps, gamma_e, gamma_r, dtype):
    """Per triple: r is [B][2 D^2], one relation row per triple."""
    return _rescal_sides(s, r, torch.arange(s.shape[0]), o, neg_o, neg_s, N, NS, D, lr, eps,
                         gamma_e, gamma_r, dtype)


def rescal_sides_grouped_ref(s, rm, starts, o, neg_o, neg_s, N, NS, D, lr, eps, gamma_e, gamma_r,
                             dtype):
    """Grouped: rm is [G][2 D^2]; triples [starts[g], starts[g+1]) use matrix
    g, and dR is the AdaGrad transform of the group-summed gradient."""
    counts = np.diff(np.asarray(starts, dtype=np.int64))
    gid = torch.from_numpy(np.repeat(np.arange(len(counts)), counts))
    return _rescal_sides(s, rm, gid, o, neg_o, neg_s, N, NS, D, lr, eps, gamma_e, gamma_r, dtype)
