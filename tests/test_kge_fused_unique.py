"""World==1 fused ComplEx step (Server.kge_step_fused): rows that are unique
in the batch are written with plain stores, shared rows with atomics. Every
case compares the store after the step with
    snapshot + index_add(classic per-occurrence deltas, by key)
and the per-sample loss with the classic kernel's, at atol=1e-4 (values are
O(0.1), multiplicities <= 32).

Cases with duplicate keys step with lr = 0: embeddings stay put and the
accumulators become the exact sum of g^2 over occurrences, so the result
does not depend on the order in which the blocks run. All-unique cases use
lr = 0.05."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ATOL = 1e-4
EPS = 1e-6


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


def _step(server, s_k, r_k, o_k, n_k, N, D, lr):
    loss = server.raw.kge_step_fused(torch.from_numpy(s_k), torch.from_numpy(r_k),
                                     torch.from_numpy(o_k), torch.from_numpy(n_k),
                                     N, D, lr, EPS)
    torch.cuda.synchronize()
    return loss


def _check(server, worker, num_keys, s_k, r_k, o_k, n_k, N, D, lr, expect_plain=True):
    s_k, r_k, o_k, n_k = (np.ascontiguousarray(a, dtype=np.int64) for a in (s_k, r_k, o_k, n_k))
    snapshot = _pull_all(worker, num_keys, D)
    want, want_loss = _expected(snapshot, s_k, r_k, o_k, n_k, N, D, lr)
    before = server.raw.stats()
    loss = _step(server, s_k, r_k, o_k, n_k, N, D, lr)
    after = server.raw.stats()
    path = "fused_plain_steps" if expect_plain else "fused_atomic_steps"
    assert after[path] == before[path] + 1, (before, after)
    got = _pull_all(worker, num_keys, D)
    loss_err = (loss - want_loss).abs().max().item()
    err = (got - want).abs().max().item()
    print(f"loss err {loss_err:.3g}  store err {err:.3g}")
    assert loss_err < ATOL, f"loss mismatch: {loss_err}"
    assert err < ATOL, f"store mismatch: {err}"
    return got


def _unique_batch(rng, E, R, B, N, pool=None):
    """B samples whose 3B + BN keys are all different; relations are E..E+R."""
    ents = rng.permutation(E if pool is None else pool)[: B * (2 + N)].astype(np.int64)
    assert len(ents) == B * (2 + N)
    s_k, o_k, n_k = ents[:B], ents[B:2 * B], ents[2 * B:]
    r_k = (E + rng.choice(R, B, replace=False)).astype(np.int64)
    return s_k, r_k, o_k, n_k


# 1. all unique: KPT 1 full block, partial block, KPT 2, KPT 4, KPT 8
@pytest.mark.parametrize("D", [512, 64, 1024, 2048, 4096])
def test_all_unique(D):
    E, R, B, N = (64, 8, 8, 3) if D <= 1024 else (32, 4, 4, 1)
    server, worker = _store(E + R, D)
    s_k, r_k, o_k, n_k = _unique_batch(np.random.default_rng(D), E, R, B, N)
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.05)
    server.shutdown()


# 2. one relation shared by all samples, entities unique
def test_shared_relation():
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    s_k, r_k, o_k, n_k = _unique_batch(np.random.default_rng(2), E, R, B, N)
    r_k[:] = E + 5
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.0)
    server.shutdown()


# 3. an entity that is s of one sample and a negative of another
def test_subject_also_negative_elsewhere():
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    s_k, r_k, o_k, n_k = _unique_batch(np.random.default_rng(3), E, R, B, N)
    n_k[5 * N + 1] = s_k[2]
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.0)
    server.shutdown()


# 4. the same entity twice among one sample's negatives
def test_negative_twice_in_one_sample():
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    s_k, r_k, o_k, n_k = _unique_batch(np.random.default_rng(4), E, R, B, N)
    n_k[3 * N + 2] = n_k[3 * N + 0]
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.0)
    server.shutdown()


# 5. a sample with o == s
def test_object_equals_subject():
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    s_k, r_k, o_k, n_k = _unique_batch(np.random.default_rng(5), E, R, B, N)
    o_k[6] = s_k[6]
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.0)
    server.shutdown()


# 6. unique and shared entity rows in one launch, both kinds checked
def test_mixed_unique_and_shared():
    E, R, B, N, D = 128, 16, 16, 3, 64
    server, worker = _store(E + R, D)
    s_k, r_k, o_k, n_k = _unique_batch(np.random.default_rng(6), E, R, B, N)
    shared = np.array([s_k[0], o_k[1], n_k[2]])
    o_k[8:12] = shared[0]          # s of sample 0 is o of four others
    n_k[10 * N:11 * N] = shared[1]  # o of sample 1 fills one sample's negatives
    s_k[13] = shared[2]            # a negative of sample 0 is s of sample 13
    r_k[4:8] = r_k[4]              # a relation shared by four samples
    snap = _pull_all(worker, E + R, D)[:, D:]
    got = _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.0)
    # both kinds were really there, and both moved their accumulators
    keys, counts = np.unique(np.concatenate([s_k, r_k, o_k, n_k]), return_counts=True)
    assert (counts == 1).sum() > 20 and (counts > 1).sum() >= 4
    moved = (got[:, D:] - snap).abs().sum(dim=1).cpu().numpy()
    assert (moved[keys] > 0).all()
    untouched = np.setdiff1d(np.arange(E + R), keys)
    assert (moved[untouched] == 0).all()
    server.shutdown()


def _heavy_then_unique(repeat_b):
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    rng = np.random.default_rng(7)
    # step A: every key drawn from a pool of 40 entities / 2 relations
    pool = rng.permutation(E)[:40].astype(np.int64)
    a_s, a_o = rng.choice(pool, B), rng.choice(pool, B)
    a_n = rng.choice(pool, B * N)
    a_r = (E + rng.choice(2, B)).astype(np.int64)
    _check(server, worker, E + R, a_s, a_r, a_o, a_n, N, D, 0.0)
    dup = np.unique(np.concatenate([a_s, a_o, a_n]))
    _, cnt = np.unique(np.concatenate([a_s, a_o, a_n]), return_counts=True)
    assert (cnt > 1).sum() >= 4
    # step B: all unique, on exactly the rows A had marked
    assert len(pool) == B * (2 + N)
    b_s, b_r, b_o, b_n = _unique_batch(rng, E, R, B, N, pool=pool)
    assert set(dup) <= set(np.concatenate([b_s, b_o, b_n]))
    for _ in range(repeat_b):
        _check(server, worker, E + R, b_s, b_r, b_o, b_n, N, D, 0.05)
    server.shutdown()


# 7. scratch hygiene: right after a heavily duplicated step, an all-unique
#    step on the rows that step had marked must match classic as in case 1
def test_marks_cleared_after_duplicated_step():
    _heavy_then_unique(1)


# 8. same, with the all-unique step run twice in a row
def test_marks_cleared_between_unique_steps():
    _heavy_then_unique(2)


def test_marks_are_zero_between_steps(monkeypatch):
    """Cases 7/8 by count: a stale mark can only turn a unique row shared,
    which costs time and never a wrong value, so it is invisible in the
    store. With the debug counter on, a step that uses rows once each
    right after a step that used them many times must flag none."""
    monkeypatch.setenv("ADAPM_FUSED_STATS", "1")  # read on the first fused step
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    z = np.zeros(B, dtype=np.int64)
    _step(server, z, z + E, z + 1, np.full(B * N, 2, dtype=np.int64), N, D, 0.0)
    after_a = server.raw.stats()["fused_shared_occurrences"]
    assert after_a == B * (3 + N)
    e = np.arange(B * (2 + N), dtype=np.int64)
    for _ in range(2):
        _step(server, e[:B], E + np.arange(B, dtype=np.int64), e[B:2 * B], e[2 * B:], N, D, 0.0)
        assert server.raw.stats()["fused_shared_occurrences"] == after_a
    server.shutdown()


# 9. grid-stride: more samples than the grid cap of 16384 blocks
def test_grid_stride():
    E, R, B, N, D = 20000, 1024, 16400, 1, 8
    server, worker = _store(E + R, D)
    rng = np.random.default_rng(9)
    s_k, o_k, n_k = rng.integers(0, E, B), rng.integers(0, E, B), rng.integers(0, E, B * N)
    r_k = E + np.arange(B) % R  # <= 17 samples per relation
    _, counts = np.unique(np.concatenate([s_k, o_k, n_k]), return_counts=True)
    assert counts.max() <= 32 and (counts > 1).sum() > 1000 and (counts == 1).sum() > 1000
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.0)
    server.shutdown()


# 10. fallback: a fused step on a stream other than the one that owns the
#     row marks runs the all-atomic kernel, and so does every step after it
def test_other_stream_falls_back_to_atomic():
    E, R, B, N, D = 64, 8, 8, 3, 64
    server, worker = _store(E + R, D)
    rng = np.random.default_rng(10)
    s_k, r_k, o_k, n_k = _unique_batch(rng, E, R, B, N)
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.05)  # owner: default stream
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.05, expect_plain=False)
    torch.cuda.synchronize()
    _check(server, worker, E + R, s_k, r_k, o_k, n_k, N, D, 0.05, expect_plain=False)
    server.shutdown()
