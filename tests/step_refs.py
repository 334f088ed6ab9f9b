"""Shared high-precision references for the step, scoring and loss kernels.

Every reference here is the plain definition of the operation, evaluated on
the CPU in the dtype it is asked for: the loss is written down, torch autograd
differentiates it, and the AdaGrad transform is applied to the gradient.
Nothing is shared with the kernels or their CPU twins. Called with
``torch.float64`` a reference is the truth a kernel is compared with; called
with ``torch.float32`` it is the yardstick for how much error fp32 arithmetic
alone puts into that very case (see ``assert_half_close``).

Rows follow the store's layout ``[emb(L) | accum(L)]``. A step reference
returns ``{"loss": [B], name: (delta, g2), ...}``: for every output tensor the
delta half and the g^2 half separately, and the per-sample loss.
"""
import numpy as np
import torch

K_MARGIN = 16.0
EPS_F32 = 2.0 ** -23


# ------------------------------------------------------------ comparison

def rel_err(x, ref64):
    """max|x - ref64| / max|ref64| over one half of one output tensor."""
    scale = ref64.abs().max().item()
    return ((x.detach().cpu().double() - ref64).abs().max() / scale).item()


def assert_half_close(got, ref64, ref32, what, family=None):
    """`got` (fp32, any device) against the fp64 reference of the same half.

    error = max|got - ref64| / max|ref64|; bound = K * max(e32, 2^-23) with
    e32 the same error measure of `ref32`, the fp32 evaluation of the
    reference for this very case. An identically zero reference demands an
    exactly zero result. Prints one RATIO line per call (`family` only
    labels it) and returns err / max(e32, 2^-23).
    """
    got = got.detach().cpu()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    assert ref64.dtype == torch.float64 and ref32.dtype == torch.float32
    if ref64.numel() == 0:
        return 0.0
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} values left unwritten (NaN)"
    if not ref64.any():
        assert not got.any(), f"{what}: reference is exactly zero, got max |{got.abs().max().item():g}|"
        return 0.0
    err = rel_err(got, ref64)
    e32 = rel_err(ref32, ref64)
    floor = max(e32, EPS_F32)
    ratio = err / floor
    print(f"RATIO {family or '-'} {what}: err={err:.3e} e32={e32:.3e} "
          f"err/e32={(err / e32 if e32 else float('inf')):.3g} err/max(e32,2^-23)={ratio:.3g}")
    assert err <= K_MARGIN * floor, (
        f"{what}: err {err:.3e} > {K_MARGIN:g} * max(e32 {e32:.3e}, 2^-23) = {K_MARGIN * floor:.3e}")
    return ratio


def assert_step_close(got, ref64, ref32, what, family=None):
    """All halves and the loss of one step: `got` maps a name to the
    kernel's [rows][2L] output (or "loss" to its [B] loss)."""
    for name, g in got.items():
        if name == "loss":
            assert_half_close(g, ref64["loss"], ref32["loss"], f"{what} loss", family)
            continue
        L = g.shape[1] // 2
        g = g.detach().cpu()
        for half, part in ((0, "delta"), (1, "g2")):
            assert_half_close(g[:, half * L:(half + 1) * L], ref64[name][half], ref32[name][half],
                              f"{what} {name}.{part}", family)


# ------------------------------------------------------------ output buffers

SENTINEL = -12345.6789


class Guarded:
    """An output buffer prefilled with NaN, with one extra trailing row of a
    sentinel: a lane the kernel skips stays NaN and fails the comparison, a
    write past the end changes the sentinel row."""

    def __init__(self, rows, cols, device):
        self.full = torch.full((rows + 1, cols), float("nan"), dtype=torch.float32, device=device)
        self.full[rows] = SENTINEL
        self.out = self.full[:rows]  # contiguous view the kernel writes
        self.rows = rows

    def check(self, what):
        tail = self.full[self.rows].cpu()
        want = torch.full_like(tail, SENTINEL)
        assert torch.equal(tail.view(torch.int32), want.view(torch.int32)), \
            f"{what}: wrote past the end of the buffer"


def guarded_vec(n, device):
    """[n] output (a loss) with the same NaN prefill and sentinel."""
    g = Guarded(n, 1, device)
    g.out = g.full[:n, 0]
    return g


# ------------------------------------------------------------ helpers

def _f32(x):
    """Scalars reach the kernels as fp32."""
    return float(np.float32(x))


def _leaf(rows, L, dtype):
    return rows[:, :L].to(dtype).clone().requires_grad_(True)


def _grad(leaf):
    return leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)


def adagrad_halves(g, acc, lr, eps):
    """([-lr g / sqrt(acc + g^2 + eps)], [g^2]) for gradient g."""
    g2 = g * g
    return (-lr * g / torch.sqrt(acc + g2 + eps)).detach(), g2.detach()


def _softplus(z):
    # log(1 + exp(z)) without a branch; its derivative is sigmoid(z)
    return torch.logaddexp(z, torch.zeros_like(z))


def _halves(rows, leaf, L, lr, eps, dtype):
    return adagrad_halves(_grad(leaf).reshape(rows.shape[0], L), rows[:, L:].to(dtype), lr, eps)


# ------------------------------------------------------------ ComplEx

def complex_psi(se, re_, oe, dc):
    """psi[b][j] for s, r [B][D] and objects oe [B][J][D]."""
    sre, sim = se[:, :dc], se[:, dc:]
    rre, rim = re_[:, :dc], re_[:, dc:]
    ure = (sre * rre - sim * rim)[:, None, :]
    uim = (sim * rre + sre * rim)[:, None, :]
    return (ure * oe[..., :dc] + uim * oe[..., dc:]).sum(-1)


def complex_ref(s, r, o, neg, N, D, lr, eps, dtype):
    """ComplEx logistic loss with N o-side negatives per positive."""
    lr, eps = _f32(lr), _f32(eps)
    B = s.shape[0]
    se, re_, oe, ne = (_leaf(t, D, dtype) for t in (s, r, o, neg))
    objs = torch.cat([oe[:, None, :], ne.view(B, N, D)], dim=1)
    psi = complex_psi(se, re_, objs, D // 2)
    loss = _softplus(-psi[:, 0]) + _softplus(psi[:, 1:]).sum(1)
    loss.sum().backward()
    return {"loss": loss.detach(), "psi": psi.detach(),
            "s": _halves(s, se, D, lr, eps, dtype), "r": _halves(r, re_, D, lr, eps, dtype),
            "o": _halves(o, oe, D, lr, eps, dtype), "neg": _halves(neg, ne, D, lr, eps, dtype)}


def complex_score_ref(s, r, cand, D, dtype):
    """scores[b][e] = psi(s_b, r_b, cand_e)."""
    dc = D // 2
    s, r, c = (t[:, :D].to(dtype) for t in (s, r, cand))
    ure = s[:, :dc] * r[:, :dc] - s[:, dc:] * r[:, dc:]
    uim = s[:, dc:] * r[:, :dc] + s[:, :dc] * r[:, dc:]
    return ure @ c[:, :dc].T + uim @ c[:, dc:].T


# ------------------------------------------------------------ SGNS

def sgns_ref(ctr, ctx, neg, N, D, lr, eps, dtype):
    lr, eps = _f32(lr), _f32(eps)
    B = ctr.shape[0]
    ce, xe, ne = (_leaf(t, D, dtype) for t in (ctr, ctx, neg))
    objs = torch.cat([xe[:, None, :], ne.view(B, N, D)], dim=1)
    psi = (ce[:, None, :] * objs).sum(-1)
    loss = _softplus(-psi[:, 0]) + _softplus(psi[:, 1:]).sum(1)
    loss.sum().backward()
    return {"loss": loss.detach(), "psi": psi.detach(),
            "ctr": _halves(ctr, ce, D, lr, eps, dtype), "ctx": _halves(ctx, xe, D, lr, eps, dtype),
            "neg": _halves(neg, ne, D, lr, eps, dtype)}


# ------------------------------------------------------------ MF

def mf_ref(w, h, x, R, lr, lam, eps, dtype):
    """NZSL + L2: gradients of (x - w.h)^2 + lam (|w|^2 + |h|^2); the
    per-sample loss the step reports is the squared error alone."""
    lr, lam, eps = _f32(lr), _f32(lam), _f32(eps)
    we, he = _leaf(w, R, dtype), _leaf(h, R, dtype)
    e = x.to(dtype) - (we * he).sum(1)
    obj = e * e + lam * ((we * we).sum(1) + (he * he).sum(1))
    obj.sum().backward()
    return {"loss": (e * e).detach(),
            "w": _halves(w, we, R, lr, eps, dtype), "h": _halves(h, he, R, lr, eps, dtype)}


def mf_loss_ref(w, h, x, R, lam, dtype):
    """(squared-error sum, regulariser sum) over all nonzeros, as a [2] tensor."""
    lam = _f32(lam)
    wv, hv = w[:, :R].to(dtype), h[:, :R].to(dtype)
    e = x.to(dtype) - (wv * hv).sum(1)
    return torch.stack([(e * e).sum(), lam * ((wv * wv).sum() + (hv * hv).sum())])


# ------------------------------------------------------------ RESCAL

def _rescal(s, rmat, gid, o, neg, N, D, lr, eps, dtype):
    """Shared body: triple b scores with relation matrix rmat[gid[b]], so the
    gradient of a matrix is summed over the triples that name it."""
    lr, eps = _f32(lr), _f32(eps)
    B = s.shape[0]
    se, oe, ne = (_leaf(t, D, dtype) for t in (s, o, neg))
    Re = _leaf(rmat, D * D, dtype)
    Rb = Re.view(-1, D, D)[gid]
    u = torch.einsum("bi,bij->bj", se, Rb)
    objs = torch.cat([oe[:, None, :], ne.view(B, N, D)], dim=1)
    psi = (u[:, None, :] * objs).sum(-1)
    loss = _softplus(-psi[:, 0]) + _softplus(psi[:, 1:]).sum(1)
    loss.sum().backward()
    return {"loss": loss.detach(), "psi": psi.detach(),
            "s": _halves(s, se, D, lr, eps, dtype), "r": _halves(rmat, Re, D * D, lr, eps, dtype),
            "o": _halves(o, oe, D, lr, eps, dtype), "neg": _halves(neg, ne, D, lr, eps, dtype)}


def rescal_ref(s, r, o, neg, N, D, lr, eps, dtype):
    """Per triple: r is [B][2 D^2], one relation row per triple."""
    return _rescal(s, r, torch.arange(s.shape[0]), o, neg, N, D, lr, eps, dtype)


def rescal_grouped_ref(s, rm, starts, o, neg, N, D, lr, eps, dtype):
    """Grouped: rm is [G][2 D^2]; triples [starts[g], starts[g+1]) use matrix
    g, and dR is the AdaGrad transform of the group-summed gradient."""
    counts = np.diff(np.asarray(starts, dtype=np.int64))
    gid = torch.from_numpy(np.repeat(np.arange(len(counts)), counts))
    return _rescal(s, rm, gid, o, neg, N, D, lr, eps, dtype)


# ------------------------------------------------------------ alias draw

def alias_draw_ref(prob, alias, seed, N):
    """The counter hash of alias_draw in numpy uint64 arithmetic."""
    n = np.uint64(prob.numel())
    p, a = prob.numpy(), alias.numpy()
    with np.errstate(over="ignore"):
        h = np.uint64(seed) ^ (np.arange(N, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15))
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
        h *= np.uint64(0xC4CEB9FE1A85EC53)
        h ^= h >> np.uint64(33)
    slot = (h % n).astype(np.int64)
    u = ((h >> np.uint64(40)) & np.uint64(0xFFFFFF)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return torch.from_numpy(np.where(u < p[slot], slot, a[slot].astype(np.int64)))
