"""The fused slab-direct RESCAL step (Server.rescal_step_fused_general,
Rescal.train_batch_fused) against step_refs.rescal_grouped_ref on the whole
store: after a step the store is the snapshot plus the reference deltas summed
by key, one half of one value length at a time within
16 * max(e32, 2^-23) (step_refs.assert_half_close, which prints a RATIO line),
and every row that the batch does not name is bit-identical.

The shared-row case steps with lr = 0; tests/test_kge_sides.py says why.
"""
import numpy as np
import pytest
import torch

import step_refs as sr
from adapm_amd.models.kge import ComplExConfig, Rescal

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda:0", id="gpu", marks=pytest.mark.gpu)]
GPU = pytest.mark.gpu
LR, EPS = 0.05, 1e-6
SPARE_ROWS = 7


def _rows(g, n, L, scale):
    """[n][2L] store rows: N(0, scale^2) values | U(0, 0.1) accumulators."""
    return torch.cat([torch.randn(n, L, generator=g) * scale, torch.rand(n, L, generator=g) * 0.1],
                     dim=1)


class Store:
    """A world-1 store of known rows with RESCAL's two value lengths."""

    def __init__(self, device, E, R, D, seed, **cfg_kw):
        import adapm_amd

        adapm_amd._SETUP.clear()
        adapm_amd.runtime._RUNTIME = None
        self.device, self.E, self.R, self.D = device, E, R, D
        adapm_amd.setup(num_keys=E + R, num_threads=1, device=device)
        self.server = adapm_amd.Server(torch.from_numpy(Rescal.value_lengths(E, R, D)))
        self.worker = adapm_amd.Worker(0, self.server)
        self.raw = self.server.raw
        self.g = torch.Generator().manual_seed(seed)
        self.ekeys = np.arange(E, dtype=np.int64)
        self.rkeys = E + np.arange(R, dtype=np.int64)
        self.worker.set(self.ekeys, _rows(self.g, E, D, 0.3).to(device))
        self.worker.set(self.rkeys, _rows(self.g, R, D * D, 0.3 / D ** 0.5).to(device))
        self.worker.wait_sync()
        self.snapshot = self.pull_all()
        cfg = ComplExConfig(num_entities=E, num_relations=R, dim=D, lr=LR, eps=EPS, **cfg_kw)
        self.model = Rescal(cfg, self.server, self.worker)

    def pull_all(self):
        """(entity rows [E][2D], relation rows [R][2D^2])"""
        ent = torch.empty(self.E, 2 * self.D, device=self.device)
        rel = torch.empty(self.R, 2 * self.D * self.D, device=self.device)
        self.worker.pull(self.ekeys, ent)
        self.worker.pull(self.rkeys, rel)
        if self.device != "cpu":
            torch.cuda.synchronize()
        return ent.cpu(), rel.cpu()

    def close(self):
        self.worker.finalize()
        self.server.shutdown()

    def refs(self, ks, rel, starts, ko, kn, N, lr=LR):
        """fp64 and fp32 reference of the step over samples sorted by relation:
        group g = samples [starts[g], starts[g+1]) of relation rel[g]."""
        ent, rels = self.snapshot
        return tuple(sr.rescal_grouped_ref(ent[ks], rels[rel], starts, ent[ko], ent[kn], N, self.D,
                                           lr, EPS, dt) for dt in (torch.float64, torch.float32))

    def check(self, ks, rel, ko, kn, refs, what, emb_fixed=False):
        fam = f"rescal_step_fused[{'cpu' if self.device == 'cpu' else 'gpu'}]"
        after = self.pull_all()
        for snap, got, L, keys, names, spare in (
                (self.snapshot[0], after[0], self.D, torch.cat([ks, ko, kn]), ("s", "o", "neg"),
                 SPARE_ROWS),
                (self.snapshot[1], after[1], self.D * self.D, rel, ("r",), 1)):
            exp = [snap.clone().to(dt).index_add_(
                0, keys, torch.cat([torch.cat(ref[n], dim=1) for n in names]).to(dt))
                for ref, dt in zip(refs, (torch.float64, torch.float32))]
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


def run_step(device, D, sizes, N, lr=LR, share=False):
    """One step over groups of `sizes` samples, every key different unless
    `share`, and the whole store compared."""
    B, G = sum(sizes), len(sizes)
    st = Store(device, B * (2 + N) + SPARE_ROWS, G + 2, D, seed=31000 + D + N)
    try:
        perm = torch.randperm(st.E, generator=st.g)
        ks, ko, kn = perm[:B].clone(), perm[B:2 * B].clone(), perm[2 * B:B * (2 + N)].clone()
        if share:  # X: s of samples 0 and 1, o of sample 2, a negative of sample 3
            ks[1] = ko[2] = kn[3 * N + 1] = ks[0]
        rel = torch.randperm(st.R, generator=st.g)[:G]  # groups not in key order
        starts = np.concatenate([[0], np.cumsum(sizes)])
        kr = st.E + rel.repeat_interleave(torch.tensor(sizes))
        refs = st.refs(ks, rel, starts, ko, kn, N, lr)
        before = st.raw.stats()
        loss, missed = st.raw.rescal_step_fused_general(ks, kr, ko, kn, N, D, lr, EPS)
        assert missed.numel() == 0
        # counted as ONE pull and ONE push of all its keys; a real pull or push
        # would add to these
        stats = st.raw.stats()
        for name, by in (("pulls", 1), ("pushes", 1), ("pull_keys", B * (3 + N)),
                         ("push_keys", B * (3 + N))):
            assert stats[name] - before[name] == by, name
        what = f"D={D} sizes={sizes} N={N}"
        fam = st.check(ks, rel, ko, kn, refs, what, emb_fixed=lr == 0.0)
        sr.assert_half_close(loss, refs[0]["loss"], refs[1]["loss"], f"{what} loss", fam)
    finally:
        st.close()


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("D,sizes,N", [
    (4, [33, 1, 5], 1), (20, [15, 16, 17], 3), (64, [33, 1, 5], 0), (68, [15, 16, 17], 1),
    (132, [33, 1, 5], 3), (256, [1], 1)])
def test_step_unique_keys(device, D, sizes, N):
    run_step(device, D, sizes, N)


@GPU
def test_step_grid_stride():
    """The mid kernel's grid is capped at 8192 workgroups of 4 triples."""
    run_step("cuda:0", 4, [40000], 1)


@pytest.mark.parametrize("device", DEVICES)
def test_step_shared_rows(device):
    run_step(device, 8, [40, 24], 2, lr=0.0, share=True)


# ------------------------------------------------------------ model

E_M, R_M, D_M, B_M, N_M = 200, 5, 8, 32, 2


def _model_batch(g, n_neg):
    perm = torch.randperm(E_M, generator=g)
    rel = torch.randint(0, R_M - 1, (B_M,), generator=g)  # relation R_M - 1 stays unnamed
    triples = torch.stack([perm[:B_M], rel, perm[B_M:2 * B_M]], dim=1).numpy().astype(np.int64)
    return triples, perm[2 * B_M:B_M * (2 + n_neg)].numpy().astype(np.int64)


@pytest.mark.parametrize("device", DEVICES)
def test_model_sorts_and_maps_back(device):
    st = Store(device, E_M, R_M, D_M, seed=32000, neg_samples=N_M, batch_size=B_M)
    try:
        triples, neg = _model_batch(st.g, N_M)
        order = np.argsort(triples[:, 1], kind="stable")
        ts = torch.from_numpy(triples[order])
        kn = torch.from_numpy(neg.reshape(B_M, N_M)[order].reshape(-1))
        rel, counts = torch.unique(ts[:, 1], return_counts=True)
        starts = np.concatenate([[0], np.cumsum(counts.numpy())])
        refs = st.refs(ts[:, 0], rel, starts, ts[:, 2], kn, N_M)
        loss = st.model.train_batch_fused(triples, force_general=True, neg_keys=neg)
        fam = st.check(ts[:, 0], rel, ts[:, 2], kn, refs, "model")
        sr.assert_half_close(loss, refs[0]["loss"], refs[1]["loss"], "model loss", fam)
    finally:
        st.close()


@pytest.mark.parametrize("device", DEVICES)
def test_model_sides_take_the_classic_step(device):
    after = []
    for fused in (True, False):
        st = Store(device, E_M, R_M, D_M, seed=33000, neg_samples=N_M, batch_size=B_M,
                   neg_samples_subject=1)
        try:
            triples, neg = _model_batch(st.g, N_M + 1)
            if fused:
                st.model.train_batch_fused(triples, force_general=True, neg_keys=neg)
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

E_G, D_G = 16, 4
_K = lambda *ks: torch.tensor(ks, dtype=torch.int64)


@pytest.mark.parametrize("device,s,r,o,neg,N,D,match", [
    ("cpu", _K(0), _K(E_G), _K(1), _K(2), 1, 6, "D = 6 must be a positive multiple of 4"),
    pytest.param("cuda:0", _K(0), _K(E_G), _K(1), _K(2), 1, 260, "D = 260 exceeds", marks=GPU),
    ("cpu", _K(0, 1, 2), _K(E_G, E_G + 1, E_G), _K(3, 4, 5), _K(6, 7, 8), 1, D_G,
     "reappears at position 2"),
    ("cpu", _K(0), _K(3), _K(1), _K(2), 1, D_G, "key 3 has a row of 8 floats, a relation row has 32"),
    ("cpu", _K(0), _K(E_G), _K(E_G + 1), _K(2), 1, D_G,
     "key 17 has a row of 32 floats, an entity row has 8"),
    ("cpu", _K(0), _K(E_G), _K(1), _K(2), -1, D_G, "N = -1 must be >= 0"),
], ids=["D6", "D260", "runs", "entity-as-r", "relation-as-o", "N-1"])
def test_guards(device, s, r, o, neg, N, D, match):
    st = Store(device, E_G, 3, D_G, seed=34000)
    try:
        with pytest.raises(RuntimeError, match=match):
            st.raw.rescal_step_fused_general(s, r, o, neg, N, D, LR, EPS)
        for got, snap in zip(st.pull_all(), st.snapshot):
            assert torch.equal(got.view(torch.int32), snap.view(torch.int32))
    finally:
        st.close()
