"""High-precision reference of the ComplEx sides step with dropout, in the
manner of sides_refs.complex_sides_ref: three explicit mask tensors multiply
the leaves before psi, torch autograd differentiates the objective, and the
AdaGrad transform is applied per role. The masks come from a numpy model of
the counter hash written from the contract in csrc/kernels.h (not from the
C++). Nothing is shared with the kernels or their CPU twins.
"""
import numpy as np
import torch

from step_refs import _f32, _halves, _leaf, _softplus


def thresholds(p_e, p_r):
    return tuple(int(np.floor(p * 1024 + 0.5)) for p in (p_e, p_r))


def drop_masks(seed, B, N, NS, D, p_e, p_r):
    """(m_s, m_r, m_o), each [B][T][D] float64 of 0 or scale, T = 1 + N + NS:
    the masks of the subject, relation and object ROLE of scored triple t."""
    dc, T = D // 2, 1 + N + NS
    thr_e, thr_r = thresholds(p_e, p_r)
    with np.errstate(over="ignore"):
        idx = np.arange(B * T * dc, dtype=np.uint64)  # (b * T + t) * dc + k
        h = np.uint64(seed) ^ (idx * np.uint64(0x9E3779B97F4A7C15))
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    h = h.reshape(B, T, dc)
    out = []
    for f, thr in ((0, thr_e), (2, thr_r), (4, thr_e)):  # re field; im is the next one
        keep = np.concatenate([(h >> np.uint64(10 * g)) & np.uint64(1023) for g in (f, f + 1)],
                              axis=2) >= np.uint64(thr)
        out.append(torch.from_numpy(keep * _f32(1024 / (1024 - thr))))
    return tuple(out)


def _psi(x, r, y, dc):
    ure = x[..., :dc] * r[..., :dc] - x[..., dc:] * r[..., dc:]
    uim = x[..., dc:] * r[..., :dc] + x[..., :dc] * r[..., dc:]
    return (ure * y[..., :dc] + uim * y[..., dc:]).sum(-1)


def complex_drop_ref(s, r, o, neg_o, neg_s, N, NS, D, lr, eps, gamma_e, gamma_r, masks, dtype):
    lr, eps, gamma_e, gamma_r = (_f32(x) for x in (lr, eps, gamma_e, gamma_r))
    m_s, m_r, m_o = (m.to(dtype) for m in masks)
    B = s.shape[0]
    se, re_, oe, noe, nse = (_leaf(t, D, dtype) for t in (s, r, o, neg_o, neg_s))
    subj = torch.cat([se[:, None, :].expand(B, 1 + N, D), nse.view(B, NS, D)], dim=1)
    obj = torch.cat([oe[:, None, :], noe.view(B, N, D), oe[:, None, :].expand(B, NS, D)], dim=1)
    psi = _psi(m_s * subj, m_r * re_[:, None, :], m_o * obj, D // 2)  # [B][T]
    loss = _softplus(-psi[:, 0]) + _softplus(psi[:, 1:]).sum(1)
    reg = (0.5 * gamma_e * ((se * se).sum(1) + (oe * oe).sum(1))
           + 0.5 * gamma_r * (re_ * re_).sum(1))
    (loss + reg).sum().backward()
    return {"loss": loss.detach(), "psi": psi.detach(),
            "s": _halves(s, se, D, lr, eps, dtype), "r": _halves(r, re_, D, lr, eps, dtype),
            "o": _halves(o, oe, D, lr, eps, dtype),
            "neg_o": _halves(neg_o, noe, D, lr, eps, dtype),
            "neg_s": _halves(neg_s, nse, D, lr, eps, dtype)}
