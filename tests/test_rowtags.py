"""Row tags of the world==1 fused ComplEx step (kernels.h): one word per key,
a tag pass (occurrence i stores i at its row), a flag pass (occurrence i
stores SHARED unless it reads its own i) and a bits pass (each occurrence
rewrites its row's bitmap word from the 32 tags behind it), all with plain
stores on memory that is never cleaned. The result must be exact, not
conservative: a row comes out shared if and only if two or more occurrences
of the batch name it.

Mask tests run the three passes through the test-only binding
`_C.rowtag_shared_mask`, which asks the bitmap what the step kernel asks it,
and compare the bool mask with numpy's counts for equality. Step tests compare the store after a fused step with
    snapshot + index_add(classic per-occurrence deltas, by key)
and the per-sample loss with the classic kernel's, at atol = 1e-4 (values are
O(0.1), multiplicities <= 32), and the step's count of shared occurrences
with numpy's. Wherever keys repeat the step runs with lr = 0: embeddings stay
put and the accumulators become the exact sum of g^2 over occurrences, so the
result does not depend on the order in which the blocks run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ATOL = 1e-4
EPS = 1e-6


# ------------------------------------------------------------------ masks

def _want_mask(parts):
    keys = np.concatenate(parts)
    _, inverse, counts = np.unique(keys, return_inverse=True, return_counts=True)
    return counts[inverse] > 1


def _mask(parts, num_keys):
    from adapm_amd import _C

    tensors = [torch.from_numpy(np.ascontiguousarray(p, dtype=np.int64)) for p in parts]
    got = _C.rowtag_shared_mask(tensors, num_keys)
    assert got.is_cuda and got.dtype == torch.bool
    return got.cpu().numpy()


def _split(keys, arrays):
    """Unequal parts, one of them empty when there is more than one."""
    n = len(keys)
    if arrays == 1:
        cuts = []
    elif arrays == 2:
        cuts = [n]                         # second array empty
    else:
        a = n // 7
        cuts = [a, a, a + (n - a) // 3]    # second array empty, the rest unequal
    return np.split(keys, cuts)


# 1. block edges: totals around one and several 256-thread blocks
@pytest.mark.parametrize("arrays", [1, 2, 4])
@pytest.mark.parametrize("total", [1, 255, 256, 257, 1025])
def test_mask_block_edges(total, arrays):
    num_keys = 4096
    rng = np.random.default_rng(1000 * arrays + total)
    # a pool of about 0.7 * total rows leaves about half the rows repeated;
    # rows 0 and num_keys - 1 are not in it
    pool = rng.choice(np.arange(1, num_keys - 1), max(1, (7 * total) // 10), replace=False)
    keys = rng.choice(pool, total).astype(np.int64)
    if total >= 255:
        keys[0] = keys[total // 2] = 0  # the first row twice,
        keys[total - 1] = num_keys - 1  # the last row once
    else:
        keys[0] = num_keys - 1
    parts = _split(keys, arrays)
    assert len(parts) == arrays and sum(len(p) for p in parts) == total
    assert arrays == 1 or any(len(p) == 0 for p in parts)
    want = _want_mask(parts)
    assert not want[total - 1]
    if total >= 255:
        _, counts = np.unique(keys, return_counts=True)
        frac = (counts > 1).mean()
        assert 0.4 < frac < 0.7, frac
        assert want[0] and want[total // 2]
    got = _mask(parts, num_keys)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]


# 2. extreme multiplicities: every occurrence shared
@pytest.mark.parametrize("rows", [1, 8])
def test_mask_extreme_multiplicity(rows):
    num_keys, total = 64, 4096
    rng = np.random.default_rng(rows)
    pool = rng.choice(num_keys, rows, replace=False)
    keys = pool[np.arange(total) % rows].astype(np.int64)
    rng.shuffle(keys)
    got = _mask([keys[:1000], keys[1000:]], num_keys)
    assert got.shape == (total,) and got.all()


# 3. all unique: no occurrence shared
def test_mask_all_unique():
    num_keys = 4096
    keys = np.random.default_rng(3).permutation(num_keys).astype(np.int64)
    got = _mask([keys[:100], keys[100:3000], keys[3000:]], num_keys)
    assert got.shape == (num_keys,) and not got.any()


# 4a. back-to-back calls of the binding (same num_keys, so the allocator
#     usually hands the second call the first call's words): each is exact
@pytest.mark.parametrize("dup_first", [True, False])
def test_mask_calls_do_not_see_each_other(dup_first):
    num_keys = 500  # not a multiple of the 32 rows of a bitmap word
    rng = np.random.default_rng(4)
    rows = rng.permutation(num_keys)[:300].astype(np.int64)
    dup = rng.choice(rows[:20], 300).astype(np.int64)  # 300 occurrences over 20 rows
    uniq = rows                                        # the same rows and 280 more, once each
    order = [dup, uniq] if dup_first else [uniq, dup]
    for keys in order * 2:
        got = _mask([keys], num_keys)
        assert np.array_equal(got, _want_mask([keys]))


# ------------------------------------------------------------------ steps

def _store(num_keys, D, seed=0):
    import adapm_amd

    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    adapm_amd.setup(num_keys=num_keys, num_threads=1, device="cuda:0")
    server = adapm_amd.Server(2 * D)
    worker = adapm_amd.Worker(0, server)
    g = torch.Generator().manual_seed(seed)
    init = torch.cat([torch.randn(num_keys, D, generator=g) * 0.2,
                      torch.rand(num_keys, D, generator=g) * 0.1], dim=1)
    worker.set(np.arange(num_keys, dtype=np.int64), init.cuda())
    return server, worker


def _pull_all(worker, num_keys, D):
    out = torch.empty(num_keys, 2 * D, device="cuda")
    worker.pull(np.arange(num_keys, dtype=np.int64), out)
    torch.cuda.synchronize()
    return out


def _expected(snapshot, s_k, r_k, o_k, n_k, N, D, lr):
    """Classic kernel on the snapshot's rows -> (store after the step, loss)."""
    from adapm_amd import _C

    keys = torch.from_numpy(np.concatenate([s_k, r_k, o_k, n_k])).cuda()
    B = len(s_k)
    rows = snapshot[keys].contiguous()
    sv, rv, ov, nv = rows[:B], rows[B:2 * B], rows[2 * B:3 * B], rows[3 * B:]
    deltas = torch.empty_like(rows)
    ds, dr, do, dn = deltas[:B], deltas[B:2 * B], deltas[2 * B:3 * B], deltas[3 * B:]
    loss = torch.empty(B, device="cuda")
    _C.kge_complex_step(sv, rv, ov, nv, ds, dr, do, dn, loss, N, D, lr, EPS)
    return snapshot.clone().index_add_(0, keys, deltas), loss


def _shared_occurrences(*parts):
    return int(_want_mask([np.asarray(p, dtype=np.int64) for p in parts]).sum())


def _check_step(server, worker, num_keys, s_k, r_k, o_k, N, D, lr, n_k=None, us=None):
    """One fused step (host negatives n_k, or device negatives from us)
    against the classic reference; returns the negative keys it used."""
    s_k, r_k, o_k = (np.ascontiguousarray(a, dtype=np.int64) for a in (s_k, r_k, o_k))
    snapshot = _pull_all(worker, num_keys, D)
    before = server.raw.stats()
    pos = [torch.from_numpy(a) for a in (s_k, r_k, o_k)]
    if us is not None:
        loss, neg = server.raw.kge_step_fused_sampled(*pos, us, N, D, lr, EPS)
        torch.cuda.synchronize()
        n_k = neg.cpu().numpy()
    else:
        n_k = np.ascontiguousarray(n_k, dtype=np.int64)
        loss = server.raw.kge_step_fused(*pos, torch.from_numpy(n_k), N, D, lr, EPS)
        torch.cuda.synchronize()
    assert n_k.shape == (len(s_k) * N,)
    after = server.raw.stats()
    assert after["fused_plain_steps"] == before["fused_plain_steps"] + 1, (before, after)
    assert after["fused_atomic_steps"] == before["fused_atomic_steps"]
    want, want_loss = _expected(snapshot, s_k, r_k, o_k, n_k, N, D, lr)
    got = _pull_all(worker, num_keys, D)
    loss_err = (loss - want_loss).abs().max().item()
    err = (got - want).abs().max().item()
    shared = after["fused_shared_occurrences"] - before.get("fused_shared_occurrences", 0)
    want_shared = _shared_occurrences(s_k, r_k, o_k, n_k)
    print(f"loss err {loss_err:.3g}  store err {err:.3g}  shared {shared} (numpy {want_shared})")
    assert loss_err < ATOL, f"loss mismatch: {loss_err}"
    assert err < ATOL, f"store mismatch: {err}"
    assert shared == want_shared
    return n_k


# 4b. no memory between steps on the server's one tag array, by count and by
#     value: duplicated then unique on the same rows, and the reverse
@pytest.mark.parametrize("dup_first", [True, False])
def test_steps_do_not_see_each_others_tags(monkeypatch, dup_first):
    monkeypatch.setenv("ADAPM_FUSED_STATS", "1")  # read on the first fused step
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    rng = np.random.default_rng(40)
    pool = rng.permutation(E)[:B * (2 + N)].astype(np.int64)
    d_s, d_o, d_n = rng.choice(pool[:6], B), rng.choice(pool[:6], B), rng.choice(pool[:6], B * N)
    d_r = (E + np.arange(B) % 2).astype(np.int64)
    u_s, u_o, u_n = pool[:B], pool[B:2 * B], pool[2 * B:]
    u_r = (E + rng.permutation(R)[:B]).astype(np.int64)
    dup = (d_s, d_r, d_o, d_n, 0.0)
    uniq = (u_s, u_r, u_o, u_n, 0.05)
    assert _shared_occurrences(*uniq[:4]) == 0
    assert _shared_occurrences(*dup[:4]) == B * (3 + N)
    for s_k, r_k, o_k, n_k, lr in ([dup, uniq] if dup_first else [uniq, dup]) * 2:
        _check_step(server, worker, E + R, s_k, r_k, o_k, N, D, lr, n_k=n_k)
    server.shutdown()


# 5. sampled step: device negatives that collide with each other and with s, o
def test_sampled_step_with_colliding_negatives(monkeypatch):
    from adapm_amd import _C
    from adapm_amd.sampling import Uniform

    monkeypatch.setenv("ADAPM_FUSED_STATS", "1")
    E, R, B, N, D = 40, 4, 8, 3, 64
    assert _C.UniformStream.supported(0, E)
    server, worker = _store(E + R, D)
    us = Uniform(0, E, 50).native_stream("cuda:0")
    rng = np.random.default_rng(5)
    collided = 0
    for _ in range(2):  # back to back on one tag array
        s_k, o_k = rng.integers(0, E, B), rng.integers(0, E, B)
        r_k = E + rng.integers(0, R, B)
        n_k = _check_step(server, worker, E + R, s_k, r_k, o_k, N, D, 0.0, us=us)
        _, counts = np.unique(n_k, return_counts=True)
        collided += int((counts > 1).sum()) + len(np.intersect1d(n_k, np.concatenate([s_k, o_k])))
    assert collided > 0  # 24 draws from 40 entities per step
    server.shutdown()


# 6. host-negatives step without negatives: the fourth key array is empty
def test_host_step_without_negatives(monkeypatch):
    monkeypatch.setenv("ADAPM_FUSED_STATS", "1")
    E, R, B, N, D = 64, 8, 8, 0, 64
    server, worker = _store(E + R, D)
    rng = np.random.default_rng(6)
    ents = rng.permutation(E)[:2 * B].astype(np.int64)
    s_k, o_k = ents[:B], ents[B:].copy()
    r_k = (E + np.arange(B)).astype(np.int64)
    empty = np.zeros(0, dtype=np.int64)
    _check_step(server, worker, E + R, s_k, r_k, o_k, N, D, 0.05, n_k=empty)  # all unique
    o_k[3] = s_k[3]
    r_k[5] = r_k[4]
    _check_step(server, worker, E + R, s_k, r_k, o_k, N, D, 0.0, n_k=empty)   # 4 shared
    server.shutdown()


# 7. more occurrences than one block of the tag and flag passes, duplicates
#    drawn as test_kge_fused_unique.test_grid_stride draws them
def test_many_occurrences(monkeypatch):
    monkeypatch.setenv("ADAPM_FUSED_STATS", "1")
    E, R, B, N, D = 1200, 64, 300, 3, 8
    server, worker = _store(E + R, D)
    rng = np.random.default_rng(7)
    s_k, o_k, n_k = rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, E, B * N)
    r_k = E + np.arange(B) % R  # <= 5 samples per relation
    assert 3 * B + len(n_k) == 1800
    _, counts = np.unique(np.concatenate([s_k, o_k, n_k]), return_counts=True)
    assert counts.max() <= 32 and (counts > 1).sum() > 100 and (counts == 1).sum() > 100
    _check_step(server, worker, E + R, s_k, r_k, o_k, N, D, 0.0, n_k=n_k)
    server.shutdown()
