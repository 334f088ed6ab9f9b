"""What the fused steps refuse on a GPU store, before anything is enqueued:
keys outside the store, and rows longer than the step kernels can hold in
registers (STEP_MAX_LANES = 2048 lanes: D/2 for ComplEx, D for SGNS)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6


def _store(num_keys, D):
    import adapm_amd

    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    adapm_amd.setup(num_keys=num_keys, num_threads=1, device="cuda:0")
    server = adapm_amd.Server(2 * D)
    worker = adapm_amd.Worker(0, server)
    g = torch.Generator().manual_seed(11)
    init = torch.cat([torch.randn(num_keys, D, generator=g) * 0.2,
                      torch.rand(num_keys, D, generator=g) * 0.1], dim=1)
    worker.set(np.arange(num_keys, dtype=np.int64), init.cuda())
    return server, worker


def _pull_all(worker, num_keys, D):
    out = torch.empty(num_keys, 2 * D, device="cuda")
    worker.pull(np.arange(num_keys, dtype=np.int64), out)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("bad", [64, -1])
def test_out_of_range_key_launches_nothing(bad):
    K, D, B, N = 64, 16, 4, 2
    server, worker = _store(K, D)
    before = _pull_all(worker, K, D)
    ok = torch.arange(B, dtype=torch.int64)
    neg = torch.arange(B * N, dtype=torch.int64) + 8
    bad_neg = neg.clone()
    bad_neg[3] = bad
    bad_b = ok.clone()
    bad_b[2] = bad
    x = torch.ones(B)
    msg = rf"key out of range: {bad}\b"
    with pytest.raises(RuntimeError, match=msg):
        server.raw.w2v_step_fused(ok, ok + 4, bad_neg, N, D, 0.05, EPS)
    with pytest.raises(RuntimeError, match=msg):
        server.raw.w2v_step_fused(bad_b, ok + 4, neg, N, D, 0.05, EPS)
    with pytest.raises(RuntimeError, match=msg):
        server.raw.mf_step_fused(ok, bad_b, x, D, 0.05, 0.01, EPS)
    with pytest.raises(RuntimeError, match=msg):
        server.raw.mf_step_fused(bad_b, ok + 4, x, D, 0.05, 0.01, EPS)
    assert torch.equal(_pull_all(worker, K, D), before)
    server.shutdown()


def _rows(n, D, device):
    g = torch.Generator().manual_seed(12)
    return torch.cat([torch.randn(n, D, generator=g) * 0.2,
                      torch.rand(n, D, generator=g) * 0.1], dim=1).to(device)


def _classic_kge(D, device):
    from adapm_amd import _C

    s, r, o, n = (_rows(1, D, device) for _ in range(4))
    ds, dr, do, dn = (torch.full_like(t, 7.0) for t in (s, r, o, n))
    loss = torch.empty(1, device=device)
    _C.kge_complex_step(s, r, o, n, ds, dr, do, dn, loss, 1, D, 0.05, EPS)
    return loss, (ds, dr, do, dn)


def _classic_w2v(D, device):
    from adapm_amd import _C

    c, x, n = (_rows(1, D, device) for _ in range(3))
    dc, dx, dn = (torch.full_like(t, 7.0) for t in (c, x, n))
    loss = torch.empty(1, device=device)
    _C.w2v_sgns_step(c, x, n, dc, dx, dn, loss, 1, D, 0.05, EPS)
    return loss, (dc, dx, dn)


@pytest.mark.parametrize("classic,D,lanes", [(_classic_kge, 4100, 2050), (_classic_w2v, 2052, 2052)])
def test_classic_step_dimension_limit(classic, D, lanes):
    with pytest.raises(RuntimeError, match=f"{lanes} exceeds .* limit of 2048"):
        classic(D, "cuda")
    torch.cuda.synchronize()
    # the CPU twins have no limit: every lane of every delta row is written
    loss, deltas = classic(D, "cpu")
    assert torch.isfinite(loss).all()
    for d in deltas:
        assert torch.isfinite(d).all() and not (d == 7.0).any()


def test_kge_step_fused_dimension_limit():
    K, D = 8, 4100
    server, worker = _store(K, D)
    before = _pull_all(worker, K, D)
    k = torch.arange(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="kge_step_fused: D/2 = 2050 exceeds .* limit of 2048"):
        server.raw.kge_step_fused(k, k + 1, k + 2, k + 3, 1, D, 0.05, EPS)
    with pytest.raises(RuntimeError, match="kge_step_fused: D/2 = 2050 exceeds .* limit of 2048"):
        server.raw.kge_step_fused_general(k, k + 1, k + 2, k + 3, 1, D, 0.05, EPS)
    assert torch.equal(_pull_all(worker, K, D), before)
    server.shutdown()


def test_w2v_step_fused_dimension_limit():
    K, D = 8, 2052
    server, worker = _store(K, D)
    before = _pull_all(worker, K, D)
    k = torch.arange(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="w2v_step_fused: D = 2052 exceeds .* limit of 2048"):
        server.raw.w2v_step_fused(k, k + 1, k + 2, 1, D, 0.05, EPS)
    with pytest.raises(RuntimeError, match="w2v_step_fused: D = 2052 exceeds .* limit of 2048"):
        server.raw.w2v_step_fused_general(k, k + 1, k + 2, 1, D, 0.05, EPS)
    assert torch.equal(_pull_all(worker, K, D), before)
    server.shutdown()
