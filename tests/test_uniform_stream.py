"""Native uniform key stream (_C.UniformStream, sampling.Uniform.draw_native,
Server.kge_step_fused_sampled): the keys and the generator state are those of
numpy's Generator(PCG64).integers(lo, hi, size=n, dtype=int64), bit for bit,
whichever side serves a call. Integer results are compared exactly; the store
after a sampled step is compared with the store after the host-key step at
test_kge_fused_unique's ATOL (accumulators differ by atomic summation order
only)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ATOL = 1e-4
EPS = 1e-6
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CPU_NS = [1, 2, 3, 7, 4096, 100001]  # odd n flip the has_uint32 parity between calls
CPU_RANGES = [(0, 10_000_000), (5, 1000), (0, 2 ** 31 + 1), (0, 2 ** 32 - 1)]
HALF = (0, 2 ** 31 + 1)  # about 50 % rejection


def _uniform(lo, hi, seed):
    from adapm_amd.sampling import Uniform

    return Uniform(lo, hi, seed)


def _np_draw(ref, lo, hi, n):
    return ref.integers(lo, hi, size=n, dtype=np.int64)


def _assert_state_equal(u, ref):
    """Exported native state == numpy's state after the same draws."""
    w = u.native_stream(u._native_dev).export_state()
    st = ref.bit_generator.state
    assert (w[0] << 64) | w[1] == st["state"]["state"]
    assert (w[2] << 64) | w[3] == st["state"]["inc"]
    assert w[4] == st["has_uint32"]
    if st["has_uint32"]:
        assert w[5] == st["uinteger"]


# ------------------------------------------------------------------ CPU twin

@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("lo,hi", CPU_RANGES)
def test_twin_equals_numpy_over_consecutive_calls(lo, hi, seed):
    u, ref = _uniform(lo, hi, seed), np.random.default_rng(seed)
    assert u.native_supported()
    for n in CPU_NS:
        got = u.draw_native(n, "cpu")
        assert got.dtype == torch.int64 and got.shape == (n,)
        assert np.array_equal(got.numpy(), _np_draw(ref, lo, hi, n)), (lo, hi, seed, n)
        _assert_state_equal(u, ref)
    # and the host side picks the stream up where the native side left it
    assert np.array_equal(u.draw(5), _np_draw(ref, lo, hi, 5))
    assert u.rng.bit_generator.state["state"] == ref.bit_generator.state["state"]


def test_interleaving_host_and_native():
    lo, hi = 0, 10_000_000
    u, ref = _uniform(lo, hi, 3), np.random.default_rng(3)
    got = [u.draw(7), u.draw_native(1001, "cpu").numpy(), u.draw(4096),
           u.draw_native(3, "cpu").numpy()]
    want = [_np_draw(ref, lo, hi, n) for n in (7, 1001, 4096, 3)]
    assert np.array_equal(np.concatenate(got), np.concatenate(want))


def test_twin_forced_shortfall():
    lo, hi = HALF
    u, ref = _uniform(lo, hi, 11), np.random.default_rng(11)
    for n in (4097, 5):
        got = u.native_stream("cpu").draw(n, 0)  # slack 0: sequential continuation
        assert np.array_equal(got.numpy(), _np_draw(ref, lo, hi, n))
        _assert_state_equal(u, ref)


@pytest.mark.parametrize("lo,hi", [(3, 4), (0, 2 ** 32), (-5, 2 ** 32 + 9), (0, 2 ** 40)])
def test_fallback_ranges_take_the_host_path(lo, hi):
    from adapm_amd import _C

    assert not _C.UniformStream.supported(lo, hi)
    u, ref = _uniform(lo, hi, 5), np.random.default_rng(5)
    assert not u.native_supported()
    for n in (1, 3, 1000):
        got = u.draw_native(n, "cpu")
        assert np.array_equal(got.numpy(), _np_draw(ref, lo, hi, n))
    assert u._native is None
    with pytest.raises(RuntimeError):
        _C.UniformStream(lo, hi, "cpu")


# ------------------------------------------------------------------ device

GPU_NS = [1, 63, 64, 65, 4097, 100001]


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(0, 10_000_000), HALF])
def test_device_draw_equals_numpy(lo, hi):
    for n in GPU_NS:
        u, ref = _uniform(lo, hi, n), np.random.default_rng(n)
        for _ in range(2):
            got = u.draw_native(n, "cuda:0")
            assert got.is_cuda and got.dtype == torch.int64
            assert np.array_equal(got.cpu().numpy(), _np_draw(ref, lo, hi, n)), (lo, hi, n)
        _assert_state_equal(u, ref)


@pytest.mark.gpu
def test_device_forced_shortfall():
    lo, hi = HALF
    u, ref = _uniform(lo, hi, 13), np.random.default_rng(13)
    got = u.native_stream("cuda:0").draw(4097, 0)
    assert np.array_equal(got.cpu().numpy(), _np_draw(ref, lo, hi, 4097))
    _assert_state_equal(u, ref)


@pytest.mark.gpu
def test_device_draw_on_second_stream():
    lo, hi = 0, 10_000_000
    u, ref = _uniform(lo, hi, 17), np.random.default_rng(17)
    a = u.draw_native(4097, "cuda:0")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        b = u.draw_native(4097, "cuda:0")
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), _np_draw(ref, lo, hi, 4097))
    assert np.array_equal(b.cpu().numpy(), _np_draw(ref, lo, hi, 4097))


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


STAT_KEYS = ["fused_plain_steps", "fused_atomic_steps", "pull_keys", "push_keys", "pulls",
             "pushes"]


def _sampled_vs_host(s_k, r_k, o_k, lo, hi, E, R, D, N, lr, seed):
    """One sampled step on one store, one host-key step on its twin."""
    B = len(s_k)
    keys = [torch.from_numpy(np.ascontiguousarray(k, dtype=np.int64)) for k in (s_k, r_k, o_k)]
    results = []
    for sampled in (True, False):
        server, worker = _store(E + R, D)
        before = server.raw.stats()
        if sampled:
            us = _uniform(lo, hi, seed).native_stream("cuda:0")
            loss, neg = server.raw.kge_step_fused_sampled(*keys, us, N, D, lr, EPS)
            neg = neg.cpu().numpy()
        else:
            neg = _np_draw(np.random.default_rng(seed), lo, hi, B * N)
            loss = server.raw.kge_step_fused(*keys, torch.from_numpy(neg), N, D, lr, EPS)
        torch.cuda.synchronize()
        after = server.raw.stats()
        moved = {k: after[k] - before[k] for k in STAT_KEYS if k in after}
        results.append((neg, loss.cpu(), _pull_all(worker, E + R, D).cpu(), moved))
        server.shutdown()
    (neg_a, loss_a, store_a, stat_a), (neg_b, loss_b, store_b, stat_b) = results
    assert np.array_equal(neg_a, neg_b)
    assert torch.equal(loss_a, loss_b)
    err = (store_a - store_b).abs().max().item()
    print(f"store err {err:.3g}")
    assert err < ATOL
    assert stat_a == stat_b and stat_a["fused_plain_steps"] == 1
    return neg_a


@pytest.mark.gpu
def test_sampled_step_equals_host_key_step():
    E, R, D, B, N = 5000, 16, 32, 64, 4
    rng = np.random.default_rng(21)
    s_k, o_k = rng.integers(0, E, B), rng.integers(0, E, B)
    r_k = E + rng.integers(0, R, B)
    _sampled_vs_host(s_k, r_k, o_k, 0, E, E, R, D, N, 0.0, seed=22)


@pytest.mark.gpu
def test_sampled_step_all_unique_batch():
    E, R, D, B, N = 5000, 16, 32, 8, 4
    # the negatives seed 24 draws are known beforehand: pick s, o around them
    neg = _np_draw(np.random.default_rng(24), 0, E, B * N)
    assert len(np.unique(neg)) == B * N
    free = np.setdiff1d(np.arange(E, dtype=np.int64), neg)
    s_k, o_k = free[:B], free[B:2 * B]
    r_k = E + np.arange(B, dtype=np.int64)
    got = _sampled_vs_host(s_k, r_k, o_k, 0, E, E, R, D, N, 0.05, seed=24)
    assert len(np.unique(np.concatenate([s_k, r_k, o_k, got]))) == B * (3 + N)


@pytest.mark.gpu
def test_sampled_step_rejects_a_stream_wider_than_the_store():
    E, R, D, B, N = 64, 8, 32, 8, 2
    server, worker = _store(E + R, D)
    z = torch.zeros(B, dtype=torch.int64)
    us = _uniform(0, E + R + 1, 1).native_stream("cuda:0")
    with pytest.raises(RuntimeError, match="exceeds the store"):
        server.raw.kge_step_fused_sampled(z, z + E, z + 1, us, N, D, 0.0, EPS)
    server.shutdown()


_MODEL_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import adapm_amd
from adapm_amd.models.kge import ComplEx, ComplExConfig, make_synthetic_triples
E, R, D, B, N = 5000, 16, 32, 64, 4
adapm_amd.setup(num_keys=E + R, num_threads=1, device="cuda:0")
server = adapm_amd.Server(2 * D)
server.enable_sampling_support("local", True, "uniform", 0, E)
worker = adapm_amd.Worker(0, server)
cfg = ComplExConfig(num_entities=E, num_relations=R, dim=D, neg_samples=N, batch_size=B, lr=0.0)
model = ComplEx(cfg, server, worker)
torch.manual_seed(0)  # init_embeddings draws from torch's generator
model.init_embeddings()
triples = make_synthetic_triples(3 * B, E, R, seed=100)
losses = [model.train_batch_fused(triples[i * B:(i + 1) * B]).cpu().numpy() for i in range(3)]
np.save(sys.argv[2], np.stack(losses))
print("native_live", server.sampling.dist._native_live)
server.shutdown()
"""


@pytest.mark.gpu
def test_model_device_negatives_equal_host_negatives(tmp_path):
    out = {}
    for host in ("1", "0"):
        env = dict(os.environ, ADAPM_HOST_NEGATIVES=host)
        path = str(tmp_path / f"loss_{host}.npy")
        r = subprocess.run([sys.executable, "-c", _MODEL_CHILD, REPO, path], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        out[host] = np.load(path)
        # the device draw really served the run that should use it, and only that one
        assert f"native_live {host == '0'}" in r.stdout, r.stdout
    assert out["0"].shape == (3, 64)
    assert np.array_equal(out["0"], out["1"])
