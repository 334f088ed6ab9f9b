"""High-precision reference of the ComplEx sides step, in the manner of
step_refs.complex_ref: the objective is written down, torch autograd
differentiates it, and the AdaGrad transform is applied per role. Nothing is
shared with the kernels or their CPU twins.

One sample is a positive (s, r, o) with N object-side negatives (s, r, o'_j)
and NS subject-side negatives (s'_j, r, o). The objective adds the L2 terms
0.5 * gamma_e * (|s|^2 + |o|^2) + 0.5 * gamma_r * |r|^2 of the positive's rows
to the 1 + N + NS logistic terms; the loss the step reports leaves them out.
"""
import torch

from step_refs import _f32, _halves, _leaf, _softplus, complex_psi


def subject_psi(xe, re_, oe, dc):
    """psi[b][j] = psi(x[b][j], r[b], o[b]) for subjects xe [B][J][D]."""
    xre, xim = xe[..., :dc], xe[..., dc:]
    rre, rim = re_[:, None, :dc], re_[:, None, dc:]
    ure = xre * rre - xim * rim
    uim = xim * rre + xre * rim
    return (ure * oe[:, None, :dc] + uim * oe[:, None, dc:]).sum(-1)


def complex_sides_ref(s, r, o, neg_o, neg_s, N, NS, D, lr, eps, gamma_e, gamma_r, dtype):
    lr, eps, gamma_e, gamma_r = (_f32(x) for x in (lr, eps, gamma_e, gamma_r))
    B = s.shape[0]
    se, re_, oe, noe, nse = (_leaf(t, D, dtype) for t in (s, r, o, neg_o, neg_s))
    objs = torch.cat([oe[:, None, :], noe.view(B, N, D)], dim=1)
    psi_o = complex_psi(se, re_, objs, D // 2)
    psi_s = subject_psi(nse.view(B, NS, D), re_, oe, D // 2)
    loss = _softplus(-psi_o[:, 0]) + _softplus(psi_o[:, 1:]).sum(1) + _softplus(psi_s).sum(1)
    reg = (0.5 * gamma_e * ((se * se).sum(1) + (oe * oe).sum(1))
           + 0.5 * gamma_r * (re_ * re_).sum(1))
    (loss + reg).sum().backward()
    return {"loss": loss.detach(), "psi": torch.cat([psi_o, psi_s], dim=1).detach(),
            "s": _halves(s, se, D, lr, eps, dtype), "r": _halves(r, re_, D, lr, eps, dtype),
            "o": _halves(o, oe, D, lr, eps, dtype),
            "neg_o": _halves(neg_o, noe, D, lr, eps, dtype),
            "neg_s": _halves(neg_s, nse, D, lr, eps, dtype)}
