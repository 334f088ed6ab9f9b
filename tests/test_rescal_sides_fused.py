"""The fused slab-direct RESCAL step of the two-sided objective
(Server.rescal_step_sides_fused_general, Rescal.train_batch_fused(fuse_sides=
True)) against rescal_sides_refs.rescal_sides_grouped_ref on the whole store,
by the method of tests/test_rescal_fused.py, whose store helper this file
extends by the fifth key role: after a step the store is the snapshot plus the
reference deltas summed by key, one half of one value length at a time within
16 * max(e32, 2^-23) (step_refs.assert_half_close, which prints a RATIO line),
and every row that the batch does not name is bit-identical.

The shared-row case steps with lr = 0; tests/test_kge_sides.py says why.
"""
import numpy as np
import pytest
import torch

import rescal_sides_refs as rr
import step_refs as sr
from test_rescal_fused import (B_M, D_M, DEVICES, E_M, EPS, GPU, LR, N_M, R_M, SPARE_ROWS, Store,
                               _model_batch)

DTS = (torch.float64, torch.float32)
NAMES = ("s", "o", "neg_o", "neg_s")
NS_M, GE_M, GR_M = 2, 0.01, 0.02


class SidesStore(Store):
    def refs(self, ks, rel, starts, ko, kno, kns, N, NS, ge, gr, lr=LR):
        ent, rels = self.snapshot
        return tuple(rr.rescal_sides_grouped_ref(ent[ks], rels[rel], starts, ent[ko], ent[kno],
                                                 ent[kns], N, NS, self.D, lr, EPS, ge, gr, dt)
                     for dt in DTS)

    def check(self, ekeys, rel, refs, what, emb_fixed=False):
        """ekeys: the entity keys role by role, in the order of NAMES."""
        fam = f"rescal_step_sides_fused[{'cpu' if self.device == 'cpu' else 'gpu'}]"
        after = self.pull_all()
        for snap, got, L, keys, names, spare in (
                (self.snapshot[0], after[0], self.D, torch.cat(ekeys), NAMES, SPARE_ROWS),
                (self.snapshot[1], after[1], self.D * self.D, rel, ("r",), 1)):
            exp = [snap.clone().to(dt).index_add_(
                0, keys, torch.cat([torch.cat(ref[n], dim=1) for n in names]).to(dt))
                for ref, dt in zip(refs, DTS)]
            named = torch.unique(keys)
            for half, part in ((0, "emb"), (1, "acc")):
                cols = slice(half * L, (half + 1) * L)
                sr.assert_half_close(got[named][:, cols], exp[0][named][:, cols],
                                     exp[1][named][:, cols], f"{what} L={L} {part}", fam)
            rest = torch.ones(snap.shape[0], dtype=torch.bool)
            rest[named] = False
            assert int(rest.sum()) >= spare
            assert torch.equal(got[rest].view(torch.int32), snap[rest].view(torch.int32)), \
                f"{what}: a row that the batch does not name changed"
            if emb_fixed:
                assert torch.equal(got[:, :L].view(torch.int32), snap[:, :L].view(torch.int32))
        return fam


def batch(st, sizes, N, NS):
    """Distinct keys for every role, groups of `sizes` not in key order."""
    B = sum(sizes)
    cuts = np.cumsum([0, B, B, B * N, B * NS])
    perm = torch.randperm(st.E, generator=st.g)
    ekeys = [perm[a:b].clone() for a, b in zip(cuts[:-1], cuts[1:])]
    rel = torch.randperm(st.R, generator=st.g)[:len(sizes)]
    return ekeys, rel, st.E + rel.repeat_interleave(torch.tensor(sizes))


def run_step(device, D, sizes, N, NS, ge, gr, lr=LR, share=False):
    B = sum(sizes)
    st = SidesStore(device, B * (2 + N + NS) + SPARE_ROWS, len(sizes) + 2, D, seed=41000 + D + N)
    try:
        ekeys, rel, kr = batch(st, sizes, N, NS)
        ks, ko, kno, kns = ekeys
        if share:  # X: s of samples 0 and 1, o of 2, an o' of 3, an s' of 4
            ks[1] = ko[2] = kno[3 * N + 1] = kns[4 * NS] = ks[0]
        starts = np.concatenate([[0], np.cumsum(sizes)])
        refs = st.refs(ks, rel, starts, ko, kno, kns, N, NS, ge, gr, lr)
        loss, missed = st.raw.rescal_step_sides_fused_general(ks, kr, ko, kno, kns, N, NS, D, lr,
                                                              EPS, ge, gr)
        assert missed.numel() == 0
        what = f"D={D} sizes={sizes} N={N} NS={NS}"
        fam = st.check(ekeys, rel, refs, what, emb_fixed=lr == 0.0)
        sr.assert_half_close(loss, refs[0]["loss"], refs[1]["loss"], f"{what} loss", fam)
    finally:
        st.close()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D,sizes,N,NS,ge,gr", [
    (4, [33, 1, 5], 1, 1, 0.0, 0.0), (20, [15, 16, 17], 3, 2, 0.01, 0.02),
    (64, [32], 0, 2, 0.01, 0.02), (68, [15, 16, 17], 1, 0, 0.01, 0.02),
    (132, [33, 1, 5], 2, 3, 0.01, 0.0), (256, [1], 1, 1, 0.0, 0.02)])
def test_step_unique_keys(device, D, sizes, N, NS, ge, gr):
    run_step(device, D, sizes, N, NS, ge, gr)


@GPU
def test_step_grid_stride():
    """The mid kernel's grid is capped at 8192 workgroups of 4 triples."""
    run_step("cuda:0", 4, [33000], 1, 1, 0.0, 0.0)


@pytest.mark.parametrize("device", DEVICES)
def test_step_shared_rows(device):
    run_step(device, 8, [40, 24], 2, 2, 0.01, 0.02, lr=0.0, share=True)


@pytest.mark.parametrize("device", DEVICES)
def test_one_sided_case_is_the_one_sided_step(device):
    D, sizes, N, after = 20, [15, 16, 17], 3, []
    for sides in (True, False):
        st = SidesStore(device, sum(sizes) * (2 + N) + SPARE_ROWS, 5, D, seed=42000)
        try:
            (ks, ko, kno, kns), _, kr = batch(st, sizes, N, 0)
            if sides:
                loss, _ = st.raw.rescal_step_sides_fused_general(ks, kr, ko, kno, kns, N, 0, D, LR,
                                                                 EPS, 0.0, 0.0)
            else:
                loss, _ = st.raw.rescal_step_fused_general(ks, kr, ko, kno, N, D, LR, EPS)
            after.append(st.pull_all() + (loss.cpu(),))
            assert not torch.equal(after[-1][0], st.snapshot[0])
        finally:
            st.close()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*after))


# ------------------------------------------------------------ model

def _model_store(device, seed):
    return SidesStore(device, E_M, R_M, D_M, seed=seed, neg_samples=N_M, batch_size=B_M,
                      neg_samples_subject=NS_M, gamma_entity=GE_M, gamma_relation=GR_M)


@pytest.mark.parametrize("device", DEVICES)
def test_model_sorts_and_maps_back(device):
    st = _model_store(device, 43000)
    try:
        triples, neg = _model_batch(st.g, N_M + NS_M)
        order = np.argsort(triples[:, 1], kind="stable")
        ts = torch.from_numpy(triples[order])
        kno, kns = (torch.from_numpy(part.reshape(B_M, n)[order].reshape(-1))
                    for part, n in ((neg[:B_M * N_M], N_M), (neg[B_M * N_M:], NS_M)))
        rel, counts = torch.unique(ts[:, 1], return_counts=True)
        starts = np.concatenate([[0], np.cumsum(counts.numpy())])
        refs = st.refs(ts[:, 0], rel, starts, ts[:, 2], kno, kns, N_M, NS_M, GE_M, GR_M)
        loss = st.model.train_batch_fused(triples, force_general=True, neg_keys=neg,
                                          fuse_sides=True)
        fam = st.check([ts[:, 0], ts[:, 2], kno, kns], rel, refs, "model")
        sr.assert_half_close(loss, refs[0]["loss"], refs[1]["loss"], "model loss", fam)
    finally:
        st.close()


@pytest.mark.parametrize("device", DEVICES)
def test_model_without_fuse_sides_is_train_batch(device):
    after = []
    for fused in (True, False):
        st = _model_store(device, 44000)
        try:
            triples, neg = _model_batch(st.g, N_M + NS_M)
            if fused:
                st.model.train_batch_fused(triples, force_general=True, neg_keys=neg,
                                           fuse_sides=False)
            else:
                st.model.train_batch(triples, sync_loss=False, neg_keys=neg)
            st.model.drain()
            st.worker.wait_sync()
            after.append(st.pull_all())
            assert not torch.equal(after[-1][0], st.snapshot[0])
        finally:
            st.close()
    assert torch.equal(after[0][0], after[1][0]) and torch.equal(after[0][1], after[1][1])


# ------------------------------------------------------------ guards

@pytest.mark.parametrize("kns,NS,ge,match", [
    ([2], -1, 0.0, "NS = -1 must be >= 0"),
    ([2], 1, -0.5, "gamma_e = -0.5 and gamma_r = 0 must be finite and >= 0"),
    ([17], 1, 0.0, "keys_neg_s: key 17 has a row of 32 floats, an entity row has 8"),
], ids=["NS-1", "gamma<0", "relation-as-neg_s"])
def test_guards(kns, NS, ge, match):
    st = SidesStore("cpu", 16, 3, 4, seed=45000)
    try:
        k = lambda *ks: torch.tensor(ks, dtype=torch.int64)
        with pytest.raises(RuntimeError, match=match):
            st.raw.rescal_step_sides_fused_general(k(0), k(16), k(1), k(3), k(*kns), 1, NS, 4, LR,
                                                   EPS, ge, 0.0)
        for got, snap in zip(st.pull_all(), st.snapshot):
            assert torch.equal(got.view(torch.int32), snap.view(torch.int32))
    finally:
        st.close()
