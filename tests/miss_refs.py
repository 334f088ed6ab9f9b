"""Helpers of tests/test_fused_general_misses.py: stores in which a chosen
sample misses, the eight general entries as one table, and the comparison of a
whole store with the fp64 references of step_refs, sides_refs, dropout_refs,
rescal_sides_refs and rescal_dropout_refs evaluated on the HIT samples only.

A lone rank 0 of a two-rank world owns the even keys: a sample misses exactly
when it names an odd key. Every set and pull here names even keys only, a
remote key would wait for a peer that does not exist.
"""
import numpy as np
import torch

import dropout_refs
import rescal_dropout_refs
import rescal_sides_refs
import sides_refs
import step_refs as sr

LR, EPS, LAM = 0.05, 1e-6, 0.05
GE, GR = 0.01, 0.02
P_E = P_R = 0.25
DTS = (torch.float64, torch.float32)


def torch_device(device):
    return "cuda:0" if device == "cuda" else device


def rows(g, n, L, scale):
    """[n][2L] store rows: N(0, scale^2) values | U(0.01, 0.11) accumulators."""
    return torch.cat([torch.randn(n, L, generator=g) * scale,
                      torch.rand(n, L, generator=g) * 0.1 + 0.01], dim=1)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class LoneStore:
    """Rank 0 of a two-rank world, alone. `tables` are (rows, L, scale): table
    t holds the keys after those of table t - 1, rows of [emb(L) | acc(L)].
    Only the even keys exist here; `init` has a row for every key so that a
    key indexes it, the odd ones are never stored or compared."""

    def __init__(self, device, tables, seed):
        from adapm_amd import _C

        self.device = torch_device(device)
        self.tables = tables
        self.base = np.concatenate([[0], np.cumsum([n for n, _, _ in tables])]).astype(np.int64)
        lens = np.concatenate([np.full(n, 2 * L, dtype=np.int64) for n, L, _ in tables])
        if len(tables) == 1:
            lens = lens[:1]
        self.raw = _C.Server(num_keys=int(self.base[-1]), value_lengths=torch.from_numpy(lens),
                             rank=0, world=2, num_channels=2, num_workers=1, device=self.device,
                             capacity_factor=2.0, techniques=0, location_caches=True,
                             device_cap_floats=0, host_spill_floats=0, sync_threshold=0.0)
        g = torch.Generator().manual_seed(seed)
        self.init = [rows(g, n, L, scale) for n, L, scale in tables]
        for t, init in enumerate(self.init):
            own = self.owned(t)
            assert self.raw.push(0, own, init[own - int(self.base[t])].to(self.device), True) == -1

    def owned(self, t):
        """The keys of table t that this rank owns."""
        k = torch.arange(int(self.base[t]), int(self.base[t + 1]), dtype=torch.int64)
        return k[k % 2 == 0]

    def pull(self, t):
        """Table t as [rows][2L]: the owned rows as stored, the others as init."""
        own = self.owned(t)
        buf = torch.empty(len(own), self.init[t].shape[1], device=self.device)
        assert self.raw.pull(0, own, buf) == -1
        if self.device != "cpu":
            torch.cuda.synchronize()
        out = self.init[t].clone()
        out[own - int(self.base[t])] = buf.cpu()
        return out

    def key_state(self, keys):
        return [self.raw.debug_key_state(int(k)) for k in keys]


def check_table(store, t, hit_keys, refs, names, what, fam, rest_keys=(), emb_fixed=False):
    """Table t after a step against init + the reference deltas summed by key.
    `hit_keys` are the keys of the hit samples, role by role as `names` orders
    the reference's outputs; the rows they name are compared half by half, every
    other owned row, `rest_keys` among them, must have kept its bits."""
    L, base = store.tables[t][1], int(store.base[t])
    init, got = store.init[t], store.pull(t)
    idx = torch.cat(list(hit_keys)) - base
    exp = [init.to(dt).index_add_(0, idx, torch.cat([torch.cat(ref[n], dim=1) for n in names]).to(dt))
           for ref, dt in zip(refs, DTS)]
    named = torch.unique(idx)
    for half, part in ((0, "emb"), (1, "acc")):
        cols = slice(half * L, (half + 1) * L)
        sr.assert_half_close(got[named][:, cols], exp[0][named][:, cols], exp[1][named][:, cols],
                             f"{what} L={L} {part}", fam)
    own = store.owned(t) - base
    rest = torch.zeros(init.shape[0], dtype=torch.bool)
    rest[own] = True
    rest[named] = False
    for k in rest_keys:
        assert rest[int(k) - base], f"{what}: key {int(k)} is not a row of missed samples only"
    assert bits_equal(got[rest], init[rest]), f"{what}: a row that no hit sample names changed"
    if emb_fixed:
        assert bits_equal(got[own][:, :L], init[own][:, :L]), f"{what}: lr = 0 moved an embedding"
    return int(rest.sum())


# ------------------------------------------------------------ the entries

class Entry:
    """One general entry: its key roles, the call and the fp64 reference."""

    def __init__(self, name, roles, per, call, ref, drop=None):
        self.name, self.roles, self.per, self.call, self.ref, self.drop = (
            name, roles, per, call, ref, drop)


def _tail(N, NS, D, lr):
    return (N, NS, D, lr, EPS, GE, GR)


UNIFORM = {e.name: e for e in (
    Entry("kge", ("s", "r", "o", "neg"), lambda N, NS: (1, 1, 1, N),
          lambda raw, k, x, N, NS, D, lr, seed: raw.kge_step_fused_general(*k, N, D, lr, EPS),
          lambda r, x, N, NS, D, lr, masks, dt: sr.complex_ref(*r, N, D, lr, EPS, dt)),
    Entry("kge_sides", ("s", "r", "o", "neg_o", "neg_s"), lambda N, NS: (1, 1, 1, N, NS),
          lambda raw, k, x, N, NS, D, lr, seed: raw.kge_step_sides_fused_general(
              *k, *_tail(N, NS, D, lr)),
          lambda r, x, N, NS, D, lr, masks, dt: sides_refs.complex_sides_ref(
              *r, *_tail(N, NS, D, lr), dt)),
    Entry("kge_drop", ("s", "r", "o", "neg_o", "neg_s"), lambda N, NS: (1, 1, 1, N, NS),
          lambda raw, k, x, N, NS, D, lr, seed: raw.kge_step_drop_fused_general(
              *k, *_tail(N, NS, D, lr), P_E, P_R, seed),
          lambda r, x, N, NS, D, lr, masks, dt: dropout_refs.complex_drop_ref(
              *r, *_tail(N, NS, D, lr), masks, dt),
          drop=dropout_refs.drop_masks),
    Entry("w2v", ("ctr", "ctx", "neg"), lambda N, NS: (1, 1, N),
          lambda raw, k, x, N, NS, D, lr, seed: raw.w2v_step_fused_general(*k, N, D, lr, EPS),
          lambda r, x, N, NS, D, lr, masks, dt: sr.sgns_ref(*r, N, D, lr, EPS, dt)),
    Entry("mf", ("w", "h"), lambda N, NS: (1, 1),
          lambda raw, k, x, N, NS, D, lr, seed: raw.mf_step_fused_general(*k, x, D, lr, LAM, EPS),
          lambda r, x, N, NS, D, lr, masks, dt: sr.mf_ref(*r, x, D, lr, LAM, EPS, dt)),
)}

# RESCAL: the entity roles; the relation key array goes second in the call
RESCAL = {e.name: e for e in (
    Entry("rescal", ("s", "o", "neg"), lambda N, NS: (1, 1, N),
          lambda raw, k, x, N, NS, D, lr, seed: raw.rescal_step_fused_general(*k, N, D, lr, EPS),
          lambda r, starts, N, NS, D, lr, masks, dt: sr.rescal_grouped_ref(
              r[0], r[1], starts, *r[2:], N, D, lr, EPS, dt)),
    Entry("rescal_sides", ("s", "o", "neg_o", "neg_s"), lambda N, NS: (1, 1, N, NS),
          lambda raw, k, x, N, NS, D, lr, seed: raw.rescal_step_sides_fused_general(
              *k, *_tail(N, NS, D, lr)),
          lambda r, starts, N, NS, D, lr, masks, dt: rescal_sides_refs.rescal_sides_grouped_ref(
              r[0], r[1], starts, *r[2:], *_tail(N, NS, D, lr), dt)),
    Entry("rescal_drop", ("s", "o", "neg_o", "neg_s"), lambda N, NS: (1, 1, N, NS),
          lambda raw, k, x, N, NS, D, lr, seed: raw.rescal_step_drop_fused_general(
              *k, *_tail(N, NS, D, lr), P_E, P_R, seed),
          lambda r, starts, N, NS, D, lr, masks, dt: rescal_dropout_refs.rescal_drop_ref(
              r[0], r[1], starts, *r[2:], *_tail(N, NS, D, lr), masks, dt),
          drop=rescal_dropout_refs.drop_masks),
)}


# ------------------------------------------------------------ batches

def chunk_pattern(B):
    """The missed samples of the compaction case, ascending: the first and the
    last sample, both sides of the chunk boundary at 1024, a run of 40 and
    every 7th sample."""
    return np.array(sorted({0, 1023, 1024, 1025, B - 1} | set(range(300, 340))
                           | set(range(3, B, 7))), dtype=np.int64)


def unique_keys(B, per, misses):
    """[B][S] keys, S = sum(per): slot j of the batch gets key 2j, and 2j + 1
    where `misses` = {sample: column} puts the one odd key of a missed sample."""
    S = sum(per)
    keys = 2 * np.arange(B * S, dtype=np.int64).reshape(B, S)
    for b, col in misses.items():
        keys[b, col] += 1
    return keys


def split_roles(keys, per):
    """[B][S] keys -> one flat int64 tensor per role."""
    cuts = np.concatenate([[0], np.cumsum(per)])
    return [torch.from_numpy(np.ascontiguousarray(keys[:, a:b]).reshape(-1))
            for a, b in zip(cuts[:-1], cuts[1:])]


def hit_rows(role_keys, per, hit):
    """The key arrays of the hit samples, compacted in order."""
    hit = torch.as_tensor(hit)
    return [k.view(-1, n)[hit].reshape(-1) if n else k for k, n in zip(role_keys, per)]


def relation_runs(group_of, r_missed):
    """Relation keys (relative to the first one) of samples sorted by relation:
    a run is a stretch of one group with one r_missed flag, run j gets key 2j,
    or 2j + 1 where its samples miss through the relation. Returns (keys [B],
    number of relation keys)."""
    kr, j = np.empty(len(group_of), dtype=np.int64), -1
    for b in range(len(group_of)):
        if b == 0 or group_of[b] != group_of[b - 1] or r_missed[b] != r_missed[b - 1]:
            j += 1
        kr[b] = 2 * j + int(r_missed[b])
    return kr, 2 * (j + 1)


# ------------------------------------------------------------ tiered world-1 store

def mix64(x):
    """pcg_hash64 of the kernels' contract (csrc/kernels.h) on Python ints."""
    m = (1 << 64) - 1
    x &= m
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & m
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & m
    return x ^ (x >> 33)


def launch_seed(cfg_seed, n):
    """The seed of a model's n-th drop launch on rank 0 (models/kge.py)."""
    return mix64(mix64(mix64(cfg_seed)) ^ n)


class TieredStore:
    """A world-1 store whose device tier holds `cap_floats` floats; the keys
    after it, in key order, are in the host-spill tier. Tables as LoneStore's;
    `tier[k]` is Server.key_tier(k) as read after the rows are set."""

    def __init__(self, device, tables, cap_floats, seed):
        import adapm_amd

        adapm_amd._SETUP.clear()
        adapm_amd.runtime._RUNTIME = None
        self.device = torch_device(device)
        self.tables = tables
        self.base = np.concatenate([[0], np.cumsum([n for n, _, _ in tables])]).astype(np.int64)
        nk = int(self.base[-1])
        adapm_amd.setup(num_keys=nk, num_threads=1, device=self.device,
                        device_cap_gb=cap_floats * 4 / 2 ** 30, host_spill_gb=0.01)
        lens = np.concatenate([np.full(n, 2 * L, dtype=np.int64) for n, L, _ in tables])
        self.server = adapm_amd.Server(int(lens[0]) if (lens == lens[0]).all() else lens)
        self.worker = adapm_amd.Worker(0, self.server)
        g = torch.Generator().manual_seed(seed)
        self.init = [rows(g, n, L, scale) for n, L, scale in tables]
        for t, init in enumerate(self.init):
            self.worker.set(self.keys(t), init.to(self.device))
        self.worker.wait_sync()
        self.tier = np.array([self.server.raw.key_tier(k) for k in range(nk)])
        assert (self.tier == 0).any() and (self.tier == 1).any(), "both tiers must hold keys"

    def keys(self, t):
        return np.arange(self.base[t], self.base[t + 1], dtype=np.int64)

    def pull(self, t):
        out = torch.empty(self.init[t].shape, device=self.device)
        self.worker.pull(self.keys(t), out)
        if self.device != "cpu":
            torch.cuda.synchronize()
        return out.cpu()

    def close(self):
        self.worker.finalize()
        self.server.shutdown()


def check_rows(init, got, idx, deltas, L, what, fam):
    """`got` against init + deltas summed at rows idx, half by half; every
    other row must have kept its bits. deltas: the (fp64, fp32) [len(idx)][2L]."""
    exp = [init.to(dt).index_add_(0, idx, d.to(dt)) for d, dt in zip(deltas, DTS)]
    named = torch.unique(idx)
    for half, part in ((0, "emb"), (1, "acc")):
        cols = slice(half * L, (half + 1) * L)
        sr.assert_half_close(got[named][:, cols], exp[0][named][:, cols], exp[1][named][:, cols],
                             f"{what} L={L} {part}", fam)
    rest = torch.ones(init.shape[0], dtype=torch.bool)
    rest[named] = False
    assert rest.any() and bits_equal(got[rest], init[rest]), \
        f"{what}: a row that no sample names changed"
