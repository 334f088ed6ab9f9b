"""Fused CTR embedding step (Server.ctr_lookup_fused / ctr_update_fused,
models.ctr.FusedEmbedding, WideAndDeep.train_batch_fused).

Reference: numpy fp64, np.add.at of the gradients by key, then AdaGrad on an
fp64 copy of the whole store. Criterion (docs/PARITY.md, "Kernels against
fp64 references"), one half of the whole store at a time:
    err = max|got - ref64| / max|ref64| <= 16 * max(e32, 2^-23)
e32: the same error of the reference in fp32, each key's occurrences summed
in sorted order. Rows the batch does not name keep their bits."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
NK, LR, EPS = 3000, 0.05, 1e-6
DIMS = [1, 3, 4, 64, 68, 1024]  # the last is _C.CTR_MAX_DIM (test_guards)
RUNS = {  # run lengths over distinct keys, C = _C.CTR_SEG_CHUNK
    "unique": lambda C: [1] * (C + 1),
    "end-before-edge": lambda C: [C - 1, 1],
    "end-at-edge": lambda C: [C, 1],
    "end-after-edge": lambda C: [C + 1, 1],
    "begin-at-edge": lambda C: [1, C],
    "two-chunks": lambda C: [C, C],
    "one-key": lambda C: [3 * C + 5],
    "mix": lambda C: [2, 2 * C + 1, 1, 1, C - 3, 4 * C],
    "n1": lambda C: [1],
    "n0": lambda C: [],
}
_LAST = {}


def _c():
    from adapm_amd import _C

    return _C


def _store(D, threads=1, fresh=False):
    """A store of NK rows [emb | accum], accumulators at 0 and around 0.1; the
    last one made is kept for the next case of the same shape."""
    import adapm_amd
    if fresh or _LAST.get("shape") != (D, threads):
        adapm_amd._SETUP.clear()
        adapm_amd.runtime._RUNTIME = None
        adapm_amd.setup(num_keys=NK, num_threads=threads, device="cuda:0")
        server = adapm_amd.Server(2 * D)
        worker = adapm_amd.Worker(0, server)
        g = torch.Generator().manual_seed(D)
        acc = (0.05 + 0.1 * torch.rand(NK, D, generator=g)) * (torch.rand(NK, 1, generator=g) < 0.5)
        init = torch.cat([torch.randn(NK, D, generator=g) * 0.2, acc], dim=1)
        worker.set(np.arange(NK, dtype=np.int64), init.cuda())
        _LAST.update(shape=(D, threads), val=(server, worker))
    return _LAST["val"]


def _pull_all(worker, D):
    out = torch.empty(NK, 2 * D, device="cuda")
    worker.pull(np.arange(NK, dtype=np.int64), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _batch(runs, D, seed=1):
    rng = np.random.default_rng(seed)
    keys = np.repeat(rng.choice(NK, len(runs), replace=False), np.array(runs, dtype=np.int64))
    keys = keys[rng.permutation(len(keys))]
    return keys, (rng.standard_normal((len(keys), D)) * 0.1).astype(np.float32)


def _reference(store, keys, grad, D, dt):
    ref, g = store.astype(dt), np.zeros((NK, D), dt)
    order = np.argsort(keys, kind="stable")
    np.add.at(g, keys[order], grad[order].astype(dt))
    u = np.unique(keys)
    acc = ref[u, D:] + g[u] * g[u]
    ref[u, :D] += -dt(LR) * g[u] / np.sqrt(acc + dt(EPS))
    ref[u, D:] = acc
    return ref


def _check(got, store, keys, grad, D):
    ref64 = _reference(store, keys, grad, D, np.float64)
    ref32 = _reference(store, keys, grad, D, np.float32)
    for name, h in (("emb", slice(0, D)), ("acc", slice(D, 2 * D))):
        scale = np.abs(ref64[:, h]).max()
        floor = max(np.abs(ref32[:, h] - ref64[:, h]).max() / scale, 2.0 ** -23)
        err = np.abs(got[:, h] - ref64[:, h]).max() / scale
        print(f"{name}: err {err:.3g} floor {floor:.3g} ratio {err / floor:.3g}")
        assert err <= 16 * floor, (name, err, floor)
    rest = np.setdiff1d(np.arange(NK), keys)
    assert np.array_equal(got[rest].view(np.int32), store[rest].view(np.int32))


def _update(server, keys, grad, D):
    _, batch = server.raw.ctr_lookup_fused(torch.from_numpy(keys), D)
    server.raw.ctr_update_fused(batch, torch.from_numpy(grad).cuda(), D, LR, EPS)


@gpu
@pytest.mark.parametrize("runs", list(RUNS))
@pytest.mark.parametrize("D", DIMS)
def test_update(D, runs):
    server, worker = _store(D)
    keys, grad = _batch(RUNS[runs](_c().CTR_SEG_CHUNK), D)
    store = _pull_all(worker, D)
    _update(server, keys, grad, D)
    _check(_pull_all(worker, D), store, keys, grad, D)


@gpu
def test_update_deterministic():
    keys, grad = _batch(RUNS["mix"](_c().CTR_SEG_CHUNK), 64)
    got = []
    for _ in range(2):
        server, worker = _store(64, fresh=True)
        _update(server, keys, grad, 64)
        got.append(torch.from_numpy(_pull_all(worker, 64)))
    assert torch.equal(got[0], got[1])


@gpu
@pytest.mark.parametrize("n", [1, 77, 300])
@pytest.mark.parametrize("D", DIMS)
def test_gather(D, n):
    server, worker = _store(D)
    keys = np.random.default_rng(n).integers(0, NK, n)
    keys[-1] = keys[0]  # a duplicate wherever n > 1
    x, _ = server.raw.ctr_lookup_fused(torch.from_numpy(keys), D)
    want = torch.from_numpy(_pull_all(worker, D))[keys][:, :D]
    assert torch.equal(x.cpu(), want)


@gpu
def test_function():
    from adapm_amd.models.ctr import FusedEmbedding, make_synthetic_ctr
    D, F, B = 16, 4, 37
    server, worker = _store(D)
    keys = make_synthetic_ctr(B, NK, F, seed=3)[0].reshape(-1)
    W = torch.randn(B * F, D, generator=torch.Generator().manual_seed(4)) * 0.1
    store = _pull_all(worker, D)
    x = FusedEmbedding.lookup(server.raw, torch.from_numpy(keys), D, LR, EPS)
    (x * W.cuda()).sum().backward()
    _check(_pull_all(worker, D), store, keys, W.numpy(), D)


def _train(device, fused):
    """tests/test_apps.py's _ctr configuration -> (losses, stats)."""
    import adapm_amd
    from adapm_amd.models.ctr import CTRConfig, WideAndDeep, make_synthetic_ctr
    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    _LAST.clear()
    cfg = CTRConfig(num_features=2000, dim=16, fields=4, hidden=32, batch_size=512)
    adapm_amd.setup(num_keys=cfg.num_features, num_threads=1, device=device)
    server = adapm_amd.Server(cfg.row)
    worker = adapm_amd.Worker(0, server)
    model = WideAndDeep(cfg, server, worker)
    model.init_embeddings()
    feats, labels = make_synthetic_ctr(4096, cfg.num_features, cfg.fields, seed=6)
    step = model.train_batch_fused if fused else model.train_batch
    losses = [step(feats[i:i + 512], labels[i:i + 512])
              for _ in range(6) for i in range(0, len(feats), 512)]
    model.drain()
    stats = server.raw.stats()
    worker.finalize()
    server.shutdown()
    return losses, stats


@gpu
def test_model_gpu():
    losses, stats = _train("cuda:0", True)
    assert losses[-1] < 0.98 * losses[0], f"no learning: {losses[0]} -> {losses[-1]}"
    assert stats["ctr_fused_steps"] == len(losses)


def test_model_cpu_falls_back():
    losses, stats = _train("cpu", True)
    assert losses == _train("cpu", False)[0]
    assert stats["ctr_fused_steps"] == 0


@gpu
def test_guards():
    from adapm_amd.models.ctr import CTRConfig, WideAndDeep, make_synthetic_ctr
    D = 4
    assert DIMS[-1] == _c().CTR_MAX_DIM
    server, worker = _store(D, fresh=True)
    raw, keys = server.raw, torch.arange(5)
    store = _pull_all(worker, D)
    with pytest.raises(RuntimeError, match="range"):
        raw.ctr_lookup_fused(keys, _c().CTR_MAX_DIM + 1)
    with pytest.raises(Exception):
        raw.ctr_lookup_fused(torch.tensor([1, NK, 2]), D)
    _, batch = raw.ctr_lookup_fused(keys, D)
    for bad in (torch.zeros(5, D + 1), torch.zeros(4, D), torch.zeros(5, D, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="grad"):
            raw.ctr_update_fused(batch, bad.cuda(), D, LR, EPS)
    assert np.array_equal(_pull_all(worker, D), store)

    server, worker = _store(D, threads=2)
    with pytest.raises(RuntimeError, match="one worker thread"):
        server.raw.ctr_lookup_fused(keys, D)
    model = WideAndDeep(CTRConfig(num_features=NK, dim=D, fields=4, hidden=8), server, worker)
    loss = model.train_batch_fused(*make_synthetic_ctr(32, NK, 4))
    model.drain()
    assert np.isfinite(loss) and server.raw.stats()["ctr_fused_steps"] == 0
