"""The ComplEx sides step with dropout (csrc/kernels.h, kge_complex_step_drop)
through every layer: the classic kernel and its CPU twin, the fused slab-direct
kernel on the identity, device-sampled and general paths, and the model.

The reference is tests/dropout_refs.py: the sides objective with three explicit
mask tensors from a numpy model of the contract's counter hash, in fp64.
Comparison as in tests/test_kge_sides.py: one half of one output at a time,
err = max|got - ref64| / max|ref64| <= 16 * max(e32, 2^-23)
(step_refs.assert_half_close), outputs prefilled with NaN and followed by a
sentinel row, the shared-row case with lr = 0.
"""
import functools

import numpy as np
import pytest
import torch

import dropout_refs
import step_refs as sr
from adapm_amd import _C
from test_kge_sides import (DEVICES, EPS, GE, GPU, GR, LR, ROLES, Store, _check_store, _fam,
                            _rows, _shared_batch, _sync)

P_E, P_R = 0.25, 0.5
SEED = 0x5EEDD20B0C0FFEE5  # above 2^62: the whole 64-bit range reaches the kernels


def _refs(ins, N, NS, D, p_e, p_r, seed, lr=LR):
    masks = dropout_refs.drop_masks(seed, ins[0].shape[0], N, NS, D, p_e, p_r)
    return masks, tuple(dropout_refs.complex_drop_ref(*ins, N, NS, D, lr, EPS, GE, GR, masks, dt)
                        for dt in (torch.float64, torch.float32))


# A case is built once and shared by the CPU and GPU twins of a test.
@functools.lru_cache(maxsize=8)
def drop_case(B, N, NS, L, p_e=P_E, p_r=P_R, seed=SEED):
    D = 2 * L
    g = torch.Generator().manual_seed(21000 + L + 7 * N + 13 * NS)
    ins = tuple(_rows(g, n, D) for n in (B, B, B, B * N, B * NS))
    masks, (ref64, ref32) = _refs(ins, N, NS, D, p_e, p_r, seed)
    return ins, masks, ref64, ref32


def _call_drop(device, ins, N, NS, D, p_e, p_r, seed, guarded=True):
    """_C.kge_complex_step_drop -> ({role: out, "loss": out}, guards)."""
    B = ins[0].shape[0]
    bufs = {n: sr.Guarded(t.shape[0], t.shape[1], device) for n, t in zip(ROLES, ins)}
    loss = sr.guarded_vec(B, device)
    _C.kge_complex_step_drop(*[t.to(device) for t in ins], *[b.out for b in bufs.values()],
                             loss.out, N, NS, D, LR, EPS, GE, GR, p_e, p_r, seed)
    _sync(device)
    got = {n: b.out for n, b in bufs.items()}
    got["loss"] = loss.out
    return got, {**bufs, "loss": loss}


def run_drop(device, B, N, NS, L, p_e=P_E, p_r=P_R, seed=SEED):
    ins, masks, ref64, ref32 = drop_case(B, N, NS, L, p_e, p_r, seed)
    what = f"drop B={B} N={N} NS={NS} L={L} p=({p_e:g},{p_r:g})"
    got, guards = _call_drop(device, ins, N, NS, 2 * L, p_e, p_r, seed)
    sr.assert_step_close(got, ref64, ref32, what, _fam("complex_drop", device))
    for n, b in guards.items():
        b.check(f"{what} {n}")
    return masks


# ------------------------------------------------------------ classic step

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("L", [1, 65, 256, 257, 513, 1025, 2048])
def test_drop_step_lanes(device, L):
    """Every lanes-per-thread instantiation and its edges."""
    run_drop(device, 3, 2, 2, L)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("N,NS", [(0, 0), (0, 3), (3, 0), (1, 2)])
def test_drop_step_negatives(device, N, NS):
    run_drop(device, 3, N, NS, 65)


# the seed of each case is one at which every masked role has a kept and a
# dropped component (checked below, on the masks of the numpy model)
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("p_e,p_r,seed", [(0.25, 0.0, SEED), (0.0, 0.5, SEED),
                                          (1 / 1024, 1023 / 1024, SEED),
                                          (1023 / 1024, 1 / 1024, SEED)])
def test_drop_step_thresholds(device, p_e, p_r, seed):
    m_s, m_r, m_o = run_drop(device, 3, 2, 2, 65, p_e, p_r, seed)
    if device == "cpu":
        for name, m, p in (("s", m_s, p_e), ("r", m_r, p_r), ("o", m_o, p_e)):
            if p:
                assert (m == 0).any() and (m != 0).any(), f"role {name}: take another seed"
            else:
                assert (m == 1).all()


@pytest.mark.parametrize("device", DEVICES)
def test_drop_step_grid_stride(device):
    """More samples than the launch has workgroups: idx for b beyond the grid."""
    run_drop(device, 16400, 1, 1, 1)


@pytest.mark.parametrize("device", DEVICES)
def test_drop_seed_decides_the_masks(device):
    ins = drop_case(3, 2, 2, 65)[0]
    a, b, c = (_call_drop(device, ins, 2, 2, 130, P_E, P_R, s)[0] for s in (SEED, SEED, SEED + 1))
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    assert all(not torch.equal(a[n], c[n]) for n in a)


@pytest.mark.parametrize("device", DEVICES)
def test_drop_p0_is_the_sides_step(device):
    ins = [t.to(device) for t in drop_case(3, 2, 2, 65)[0]]
    got, want = ([torch.full_like(t, float("nan")) for t in ins] + [torch.empty(3, device=device)]
                 for _ in range(2))
    _C.kge_complex_step_drop(*ins, *got, 2, 2, 130, LR, EPS, GE, GR, 0.0, 0.0, SEED)
    _C.kge_complex_step_sides(*ins, *want, 2, 2, 130, LR, EPS, GE, GR)
    _sync(device)
    for a, b in zip(got, want):
        assert not torch.isnan(b).any() and torch.equal(a, b)


# ------------------------------------------------------------ fused

E_F, R_F, B_F, N_F, NS_F, NEG_SEED = 512, 4, 3, 2, 2, 31


def run_fused_drop(path, L, device="cuda:0"):
    """Store after one step against the reference, all keys different. The
    negatives are the host stream's next draw, so that the sampled path steps
    on the same keys as the other two."""
    D, B, N, NS = 2 * L, B_F, N_F, NS_F
    neg = np.random.default_rng(NEG_SEED).integers(0, E_F, size=B * (N + NS), dtype=np.int64)
    assert len(np.unique(neg)) == len(neg)
    free = np.setdiff1d(np.arange(E_F, dtype=np.int64), neg)
    keys = dict(zip(ROLES, map(torch.from_numpy, (
        free[:B].copy(), E_F + np.arange(B, dtype=np.int64), free[B:2 * B].copy(),
        neg[:B * N].copy(), neg[B * N:].copy()))))
    st = Store(E_F + R_F, D, seed=22000 + L, device=device)
    try:
        raw = st.server.raw
        ins = tuple(st.snapshot[keys[n]].contiguous() for n in ROLES)
        _, (ref64, ref32) = _refs(ins, N, NS, D, P_E, P_R, SEED)
        tail = (N, NS, D, LR, EPS, GE, GR, P_E, P_R, SEED)
        if path == "identity":
            loss = raw.kge_step_drop_fused(*[keys[n] for n in ROLES], *tail)
        elif path == "sampled":
            from adapm_amd.sampling import Uniform

            us = Uniform(0, E_F, NEG_SEED).native_stream(device)
            loss, drawn = raw.kge_step_drop_fused_sampled(*[keys[n] for n in ROLES[:3]], us, *tail)
            assert np.array_equal(drawn.cpu().numpy(), neg)
        else:
            loss, missed = raw.kge_step_drop_fused_general(*[keys[n] for n in ROLES], *tail)
            assert missed.numel() == 0
        _sync(device)
        what, fam = f"fused drop {path} L={L}", _fam("fused_drop", device)
        sr.assert_half_close(loss, ref64["loss"], ref32["loss"], f"{what} loss", fam)
        _check_store(st, st.pull_all(), keys, ref64, ref32, what, fam)
    finally:
        st.close()


@GPU
@pytest.mark.parametrize("L", [65, 513])
@pytest.mark.parametrize("path", ["identity", "sampled", "general"])
def test_fused_drop(path, L):
    run_fused_drop(path, L)


def test_fused_drop_general_cpu_store():
    run_fused_drop("general", 65, device="cpu")


@GPU
def test_fused_drop_shared_rows():
    """The UNIQ kernel's atomic branch beside its plain one, and the all-atomic
    general path on a twin store; lr = 0 (tests/test_kge_sides.py says why)."""
    E, R, B, D, N, NS = 512, 8, 64, 8, 2, 2
    keys = _shared_batch(E, R, B, N, NS)
    args = (*[keys[n] for n in ROLES], N, NS, D, 0.0, EPS, GE, GR, P_E, P_R, SEED)
    for path in ("identity", "general"):
        st = Store(E + R, D, seed=23000)
        try:
            ins = tuple(st.snapshot[keys[n]] for n in ROLES)
            _, (ref64, ref32) = _refs(ins, N, NS, D, P_E, P_R, SEED, lr=0.0)
            if path == "identity":
                loss = st.server.raw.kge_step_drop_fused(*args)
            else:
                loss, missed = st.server.raw.kge_step_drop_fused_general(*args)
                assert missed.numel() == 0
            torch.cuda.synchronize()
            what = f"fused drop shared rows, {path}"
            sr.assert_half_close(loss, ref64["loss"], ref32["loss"], f"{what} loss",
                                 "fused_drop[gpu]")
            after = st.pull_all()
            _check_store(st, after, keys, ref64, ref32, what, "fused_drop[gpu]")
            assert torch.equal(after[:, :D], st.snapshot[:, :D])
        finally:
            st.close()


# ------------------------------------------------------------ guards

def test_drop_guards():
    """Bad p, bad D and a wrong row count are refused before anything runs."""
    D = 4
    st = Store(16, D, seed=24000, device="cpu")
    try:
        raw = st.server.raw
        k = torch.arange(2, dtype=torch.int64)
        neg = torch.arange(4, dtype=torch.int64) + 4
        keys, tail = (k, k + 2, k + 4, neg, neg + 4), (LR, EPS, GE, GR)
        for fn in (raw.kge_step_drop_fused, raw.kge_step_drop_fused_general):
            for p_e, p_r in ((1.0, 0.5), (0.5, -0.1), (0.9999, 0.0), (float("nan"), 0.0)):
                with pytest.raises(RuntimeError, match="dropout p_e"):
                    fn(*keys, 2, 2, D, *tail, p_e, p_r, SEED)
        with pytest.raises(RuntimeError, match="D/2 = 2050 exceeds .* limit of 2048"):
            raw.kge_step_drop_fused(*keys, 2, 2, 4100, *tail, P_E, P_R, SEED)
        with pytest.raises(RuntimeError, match="disagree on the batch"):
            raw.kge_step_drop_fused_general(*keys[:3], neg[:3], neg + 4, 2, 2, D, *tail, P_E, P_R,
                                            SEED)
        assert torch.equal(st.pull_all(), st.snapshot)
    finally:
        st.close()
    rows = lambda n: torch.zeros(n, 2 * D)
    ok = [rows(2), rows(2), rows(2), rows(4), rows(4)]
    with pytest.raises(RuntimeError, match="dropout p_e"):
        _C.kge_complex_step_drop(*ok, *ok, torch.zeros(2), 2, 2, D, *tail, 1.0, 0.0, SEED)
    with pytest.raises(RuntimeError, match=r"neg_s and dneg_s must be \[B\*NS\]\[2D\]"):
        _C.kge_complex_step_drop(*ok[:4], rows(3), *ok, torch.zeros(2), 2, 2, D, *tail, P_E, P_R,
                                 SEED)


# ------------------------------------------------------------ model

def test_model_dropout_is_reproducible():
    """Same seeds, same stores after three classic steps; dropout 0 differs."""
    from adapm_amd.models import kge

    E, R, D, B = 40, 3, 8, 6
    triples = kge.make_synthetic_triples(3 * B, E, R, seed=5)
    after = []
    for p in (0.2, 0.2, 0.0):
        st = Store(E + R, D, seed=25000, device="cpu")
        try:
            cfg = kge.ComplExConfig(num_entities=E, num_relations=R, dim=D, neg_samples=2,
                                    neg_samples_subject=1, batch_size=B, seed=9, dropout_entity=p)
            model = kge.ComplEx(cfg, st.server, st.worker)
            for i in range(3):
                assert np.isfinite(model.train_batch(triples[i * B:(i + 1) * B]))
            model.drain()
            after.append(st.pull_all())
        finally:
            st.close()
    assert not torch.equal(after[0], st.snapshot)
    assert torch.equal(after[0].view(torch.int32), after[1].view(torch.int32))
    assert not torch.equal(after[0], after[2])
