"""The RESCAL sides step with dropout (csrc/kernels.h, rescal_step_drop) through
every layer: the classic kernels and their CPU twin, the fused slab-direct
kernels on a GPU and a CPU store, and the model.

The reference is tests/rescal_dropout_refs.py: the sides objective with three
explicit mask tensors from a numpy model of the contract's counter hashes, in
fp64. Comparison as in tests/test_rescal_sides.py and test_rescal_sides_fused.py:
one half of one output at a time, err = max|got - ref64| / max|ref64| <=
16 * max(e32, 2^-23) (step_refs.assert_half_close), outputs prefilled with NaN
and followed by a sentinel row, unnamed rows of a store bit-identical, the
shared-row case with lr = 0.
"""
import functools

import numpy as np
import pytest
import torch

import rescal_dropout_refs as rd
import step_refs as sr
from adapm_amd import _C
from test_rescal_fused import DEVICES, EPS, GPU, LR, SPARE_ROWS, Store, _rows
from test_rescal_sides_fused import SidesStore, batch

ROLES = ("s", "r", "o", "neg_o", "neg_s")
DTS = (torch.float64, torch.float32)
GE, GR = 0.01, 0.02
P_E, P_R = 0.25, 0.5
SEED = 0x5EEDD20B0C0FFEE5  # above 2^62: the whole 64-bit range reaches the kernels
MAX_D = _C.RESCAL_DROP_MAX_DIM


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _refs(ins, starts, N, NS, D, p_e, p_r, seed, lr=LR):
    masks = rd.drop_masks(seed, ins[0].shape[0], N, NS, D, p_e, p_r)
    return masks, tuple(rd.rescal_drop_ref(ins[0], ins[1], starts, *ins[2:], N, NS, D, lr, EPS, GE,
                                           GR, masks, dt) for dt in DTS)


# A case is built once and shared by the CPU and GPU twins of a test.
@functools.lru_cache(maxsize=8)
def drop_case(D, sizes, N, NS, p_e=P_E, p_r=P_R, seed=SEED):
    B = sum(sizes)
    g = torch.Generator().manual_seed(51000 + D + 7 * N + 13 * NS)
    ins = (_rows(g, B, D, 0.3), _rows(g, len(sizes), D * D, 0.3 / D ** 0.5), _rows(g, B, D, 0.3),
           _rows(g, B * N, D, 0.3), _rows(g, B * NS, D, 0.3))
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    masks, (ref64, ref32) = _refs(ins, starts, N, NS, D, p_e, p_r, seed)
    return ins, starts, masks, ref64, ref32


def _call_drop(device, ins, starts, N, NS, D, p_e, p_r, seed):
    """_C.rescal_step_drop -> ({role: out, "loss": loss}, guards)."""
    bufs = {n: sr.Guarded(t.shape[0], t.shape[1], device) for n, t in zip(ROLES, ins)}
    loss = _C.rescal_step_drop(*[t.to(device) for t in ins], *[b.out for b in bufs.values()],
                               torch.from_numpy(starts), N, NS, D, LR, EPS, GE, GR, p_e, p_r, seed)
    _sync(device)
    return {**{n: b.out for n, b in bufs.items()}, "loss": loss}, bufs


def run_drop(device, D, sizes, N=1, NS=2, p_e=P_E, p_r=P_R, seed=SEED):
    ins, starts, masks, ref64, ref32 = drop_case(D, tuple(sizes), N, NS, p_e, p_r, seed)
    what = f"drop D={D} sizes={list(sizes)} N={N} NS={NS} p=({p_e:g},{p_r:g})"
    got, guards = _call_drop(device, ins, starts, N, NS, D, p_e, p_r, seed)
    sr.assert_step_close(got, ref64, ref32, what,
                         f"rescal_drop[{'cpu' if device == 'cpu' else 'gpu'}]")
    for n, b in guards.items():
        b.check(f"{what} {n}")
    return masks


# ------------------------------------------------------------ classic step

@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D", [1, 5, 63, 64, 65, 128, 129, MAX_D])
def test_drop_step_dims(device, D):
    """Every accumulator extent and its edges, rows that start on 16 bytes and not."""
    run_drop(device, D, (3,))


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("sizes", [(33, 1, 5), (15, 16, 17)])
def test_drop_step_tiles(device, sizes):
    """Tile edges, a group joined from three partials, groups of one."""
    run_drop(device, 20, sizes)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("N,NS", [(0, 0), (0, 3), (3, 0), (1, 2)])
def test_drop_step_negatives(device, N, NS):
    run_drop(device, 20, (3,), N, NS)


# the seed of each case is one at which every masked role has a kept and a
# dropped component (checked below, on the masks of the numpy model)
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("p_e,p_r,seed", [(0.25, 0.0, SEED), (0.0, 0.5, SEED),
                                          (1 / 1024, 1023 / 1024, SEED),
                                          (1023 / 1024, 1 / 1024, SEED)])
def test_drop_step_thresholds(device, p_e, p_r, seed):
    masks = run_drop(device, 64, (3,), 1, 2, p_e, p_r, seed)
    if device == "cpu":
        for name, m, p in zip("sro", masks, (p_e, p_r, p_e)):
            if p:
                assert (m == 0).any() and (m != 0).any(), f"role {name}: take another seed"
            else:
                assert (m == 1).all()


@pytest.mark.parametrize("device", DEVICES)
def test_drop_seed_decides_the_masks(device):
    ins, starts = drop_case(20, (3,), 1, 2)[:2]
    a, b, c = (_call_drop(device, ins, starts, 1, 2, 20, P_E, P_R, s)[0]
               for s in (SEED, SEED, SEED + 1))
    for n in a:
        assert torch.equal(a[n].view(torch.int32), b[n].view(torch.int32)), n
    assert all(not torch.equal(a[n], c[n]) for n in a)


# ------------------------------------------------------------ fused

def run_fused(device, D, sizes, N=2, NS=2, lr=LR, share=False):
    """One step on a store: distinct keys unless `share`; -> the store after it."""
    B = sum(sizes)
    st = SidesStore(device, B * (2 + N + NS) + SPARE_ROWS, len(sizes) + 2, D, seed=52000 + D)
    try:
        ekeys, rel, kr = batch(st, sizes, N, NS)
        ks, ko, kno, kns = ekeys
        if share:  # X: s of samples 0 and 1, o of 2, an o' of 3, an s' of 4
            ks[1] = ko[2] = kno[3 * N + 1] = kns[4 * NS] = ks[0]
        ent, rels = st.snapshot
        starts = np.concatenate([[0], np.cumsum(sizes)])
        _, refs = _refs((ent[ks], rels[rel], ent[ko], ent[kno], ent[kns]), starts, N, NS, D, P_E,
                        P_R, SEED, lr)
        loss, missed = st.raw.rescal_step_drop_fused_general(ks, kr, ko, kno, kns, N, NS, D, lr,
                                                             EPS, GE, GR, P_E, P_R, SEED)
        assert missed.numel() == 0
        what = f"fused drop D={D} sizes={sizes}"
        fam = st.check(ekeys, rel, refs, what, emb_fixed=lr == 0.0)
        sr.assert_half_close(loss, refs[0]["loss"], refs[1]["loss"], f"{what} loss", fam)
        return st.pull_all() + (loss.cpu(),)
    finally:
        st.close()


@pytest.mark.parametrize("device,D,sizes", [
    pytest.param("cuda:0", 8, [33, 1, 5], marks=GPU),
    pytest.param("cuda:0", 64, [15, 16, 17], marks=GPU),
    pytest.param("cuda:0", 132, [17], marks=GPU), ("cpu", 8, [33, 1, 5])])
def test_fused_drop_unique_keys(device, D, sizes):
    run_fused(device, D, sizes)


@pytest.mark.parametrize("device", DEVICES)
def test_fused_drop_shared_rows(device):
    run_fused(device, 8, [40, 24], lr=0.0, share=True)


@pytest.mark.parametrize("device", DEVICES)
def test_fused_drop_is_reproducible(device):
    """No atomic on a partial: two steps from one state agree bit for bit."""
    a, b = (run_fused(device, 8, [33, 1, 5]) for _ in range(2))
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------ guards

_K = lambda *ks: torch.tensor(ks, dtype=torch.int64)


def _classic_args(device, D, B=1, ns_rows=1):
    rows = lambda n, L: torch.zeros(n, 2 * L, device=device)
    t = [rows(B, D), rows(1, D * D), rows(B, D), rows(B, D), rows(ns_rows, D)]
    return (*t, *[torch.empty_like(x) for x in t], torch.tensor([0, B], dtype=torch.int32), 1, 1, D,
            LR, EPS, GE, GR)


@pytest.mark.parametrize("device,D,kw,match", [
    ("cpu", 4, dict(p_e=1.0), "dropout p_e"), ("cpu", 4, dict(p_r=-0.1), "dropout p_e"),
    ("cpu", 4, dict(ns_rows=2), r"neg_s and dneg_s must be \[B\*NS\]\[2D\]"),
    pytest.param("cuda:0", MAX_D + 1, {}, f"D = {MAX_D + 1} exceeds", marks=GPU)])
def test_classic_guards(device, D, kw, match):
    args = _classic_args(device, D, ns_rows=kw.pop("ns_rows", 1))
    with pytest.raises(RuntimeError, match=match):
        _C.rescal_step_drop(*args, kw.get("p_e", P_E), kw.get("p_r", P_R), SEED)


@pytest.mark.parametrize("device,kns,D,p_e,match", [
    ("cpu", [3], 4, 1.0, "dropout p_e"), ("cpu", [3], 4, float("nan"), "dropout p_e"),
    ("cpu", [3], 6, P_E, "D = 6 must be a positive multiple of 4"),
    ("cpu", [3, 4], 4, P_E, "disagree on the batch"),
    pytest.param("cuda:0", [3], MAX_D + 4, P_E, f"D = {MAX_D + 4} exceeds", marks=GPU)])
def test_fused_guards(device, kns, D, p_e, match):
    st = Store(device, 16, 3, 4, seed=53000)
    try:
        with pytest.raises(RuntimeError, match=match):
            st.raw.rescal_step_drop_fused_general(_K(0), _K(16), _K(1), _K(2), _K(*kns), 1, 1, D, LR,
                                                  EPS, GE, GR, p_e, P_R, SEED)
        for got, snap in zip(st.pull_all(), st.snapshot):
            assert torch.equal(got.view(torch.int32), snap.view(torch.int32))
    finally:
        st.close()


# ------------------------------------------------------------ model

def test_model_dropout_is_reproducible():
    """Same seeds, same stores after three classic steps; dropout 0 differs."""
    from adapm_amd.models.kge import make_synthetic_triples

    E, R, D, B = 40, 3, 8, 6
    triples = make_synthetic_triples(3 * B, E, R, seed=5)
    after = []
    for p in (0.2, 0.2, 0.0):
        st = Store("cpu", E, R, D, seed=54000, neg_samples=2, neg_samples_subject=1, batch_size=B,
                   dropout_entity=p)
        try:
            for i in range(3):
                assert np.isfinite(st.model.train_batch(triples[i * B:(i + 1) * B]))
            st.model.drain()
            st.worker.wait_sync()
            after.append(st.pull_all())
        finally:
            st.close()
    assert not torch.equal(after[0][0], st.snapshot[0])
    for a, b in zip(after[0], after[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(after[0][0], after[2][0])
