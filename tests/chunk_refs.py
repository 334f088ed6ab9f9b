"""fp64 reference of the ComplEx step with chunk-shared negatives
(csrc/kernels.h, kge_complex_step_chunk), in the manner of step_refs.py: the
loss is written down, autograd differentiates it, AdaGrad is applied to the
gradient. One leaf row per occurrence."""
import torch

from step_refs import _f32, _halves, _leaf, _softplus, complex_psi


def complex_chunk_ref(s, r, o, neg, C, M, D, lr, eps, dtype):
    """Chunks of C positives; chunk c scores every positive of its own against
    neg[cM .. cM + M). s, r, o [B][2D], neg [ceil(B/C) * M][2D]."""
    lr, eps = _f32(lr), _f32(eps)
    B = s.shape[0]
    se, re_, oe, ne = (_leaf(t, D, dtype) for t in (s, r, o, neg))
    chunk = torch.arange(B) // C
    objs = torch.cat([oe[:, None, :], ne.view(-1, M, D)[chunk]], dim=1)
    psi = complex_psi(se, re_, objs, D // 2)
    loss = _softplus(-psi[:, 0]) + _softplus(psi[:, 1:]).sum(1)
    loss.sum().backward()
    return {"loss": loss.detach(),
            "s": _halves(s, se, D, lr, eps, dtype), "r": _halves(r, re_, D, lr, eps, dtype),
            "o": _halves(o, oe, D, lr, eps, dtype), "neg": _halves(neg, ne, D, lr, eps, dtype)}
