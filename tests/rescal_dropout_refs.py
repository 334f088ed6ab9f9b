"""High-precision reference of the RESCAL sides step with dropout: the
objective of rescal_sides_refs._rescal_sides with three explicit mask tensors
multiplied into the leaves before psi; torch autograd differentiates it and the
AdaGrad transform is applied per role. The masks come from a numpy model of the
two counter hashes written from the contract in csrc/kernels.h (not from the
C++). Nothing is shared with the kernels or their CPU twins.
"""
import numpy as np
import torch

from step_refs import _f32, _halves, _leaf, _softplus

GOLD = np.uint64(0x9E3779B97F4A7C15)


def _hash(seed, n):
    """pcg_hash64(seed ^ idx * GOLD) for idx < n."""
    with np.errstate(over="ignore"):
        h = np.uint64(seed) ^ (np.arange(n, dtype=np.uint64) * GOLD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    return h


def _mask(h, field, p):
    thr = int(np.floor(p * 1024 + 0.5))
    keep = ((h >> (np.uint64(10) * field)) & np.uint64(1023)) >= np.uint64(thr)
    return torch.from_numpy(keep * _f32(1024 / (1024 - thr)))


def drop_masks(seed, B, N, NS, D, p_e, p_r):
    """(m_s [B][T][D], m_r [B][T][D*D], m_o [B][T][D]) float64 of 0 or scale,
    T = 1 + N + NS: the masks of the subject role, of R and of the object role
    of scored triple t of sample b, q = b * T + t."""
    T, Q = 1 + N + NS, (D * D + 3) // 4
    he = _hash(seed, B * T * D).reshape(B, T, D)                      # idx = q * D + k
    hr = _hash(seed ^ 0xFFFFFFFFFFFFFFFF, B * T * Q).reshape(B, T, Q)  # idx = q * Q + (e >> 2)
    e = np.arange(D * D)
    return (_mask(he, np.uint64(0), p_e), _mask(hr[:, :, e >> 2], (e & 3).astype(np.uint64), p_r),
            _mask(he, np.uint64(1), p_e))


def rescal_drop_ref(s, rm, starts, o, neg_o, neg_s, N, NS, D, lr, eps, gamma_e, gamma_r, masks,
                    dtype):
    """Grouped: rm is [G][2 D^2]; samples [starts[g], starts[g+1]) use matrix g
    and dR is the AdaGrad transform of the group-summed gradient."""
    lr, eps, gamma_e, gamma_r = (_f32(x) for x in (lr, eps, gamma_e, gamma_r))
    m_s, m_r, m_o = (m.to(dtype) for m in masks)
    B, T = s.shape[0], 1 + N + NS
    counts = np.diff(np.asarray(starts, dtype=np.int64))
    gid = torch.from_numpy(np.repeat(np.arange(len(counts)), counts))
    se, oe, noe, nse = (_leaf(t, D, dtype) for t in (s, o, neg_o, neg_s))
    Re = _leaf(rm, D * D, dtype)
    Rb = Re.view(-1, D, D)[gid]                                                   # [B][D][D]
    subj = torch.cat([se[:, None, :].expand(B, 1 + N, D), nse.view(B, NS, D)], dim=1)
    obj = torch.cat([oe[:, None, :], noe.view(B, N, D), oe[:, None, :].expand(B, NS, D)], dim=1)
    psi = torch.einsum("bti,btij,btj->bt", m_s * subj, m_r.view(B, T, D, D) * Rb[:, None],
                       m_o * obj)
    loss = _softplus(-psi[:, 0]) + _softplus(psi[:, 1:]).sum(1)
    reg = (0.5 * gamma_e * ((se * se).sum(1) + (oe * oe).sum(1))
           + 0.5 * gamma_r * (Rb * Rb).sum((1, 2)))
    (loss + reg).sum().backward()
    return {"loss": loss.detach(), "psi": psi.detach(),
            "s": _halves(s, se, D, lr, eps, dtype), "r": _halves(rm, Re, D * D, lr, eps, dtype),
            "o": _halves(o, oe, D, lr, eps, dtype),
            "neg_o": _halves(neg_o, noe, D, lr, eps, dtype),
            "neg_s": _halves(neg_s, nse, D, lr, eps, dtype)}
