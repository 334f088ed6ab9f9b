"""The word2vec window step (kernels.h, w2v_window_step): the pair rules
against their model on Python ints, bit for bit, and the step against the
fp64 model within assert_half_close's bound, CPU twin and GPU kernels."""
import numpy as np
import pytest
import torch

from step_refs import assert_half_close
from w2v_window_refs import window_plan_ref, window_step_ref

DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
EPS = 1e-6
SCAN_BLOCK = 1024  # items per scan workgroup (W2V_SCAN_BLOCK); 256 totals per totals pass


def _store(V, D, device):
    """A fresh single-rank store of 2V rows [emb(D) | acc(D)] and its contents."""
    import adapm_amd

    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    adapm_amd.setup(num_keys=2 * V, num_threads=1, device="cuda:0" if device == "cuda" else "cpu")
    server = adapm_amd.Server(2 * D)
    worker = adapm_amd.Worker(0, server)
    g = torch.Generator().manual_seed(11)
    init = torch.cat([torch.randn(2 * V, D, generator=g) * 0.3,
                      torch.rand(2 * V, D, generator=g) * 0.1 + 0.01], dim=1)
    worker.set(np.arange(2 * V, dtype=np.int64), init.to(device))
    return server, worker, init


def _pull_all(worker, V, D, device):
    out = torch.empty(2 * V, 2 * D, device=device)
    worker.pull(np.arange(2 * V, dtype=np.int64), out)
    return out.cpu()


def _table(V, device, power=0.75):
    from adapm_amd.sampling import Unigram

    p = (1.0 / np.arange(1, V + 1)) ** power
    prob, alias = Unigram._build_alias(p / p.sum())
    return prob.to(device), alias.to(device)


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _stream(T, W, V, seed=5):
    """T tokens in sentences of lengths 0, 1, 2, 3, 2W+1, 40, ...; sentence s
    holds odd words only (s % 3 == 0), one even word and odd ones (1) or any
    words (2), and a sentence ends on the first scan-block boundary."""
    rng = np.random.default_rng(seed)
    lens, starts = [0, 1, 2, 3, 2 * W + 1, 40], [0]
    while starts[-1] < T:
        starts.append(min(T, starts[-1] + lens[(len(starts) - 1) % 6]))
    if T > SCAN_BLOCK:
        starts = sorted(starts + [SCAN_BLOCK])
    tok = rng.integers(0, V, size=T)
    for s in range(len(starts) - 1):
        a, b = starts[s], starts[s + 1]
        if s % 3 < 2:
            tok[a:b] |= 1
        if s % 3 == 1 and b > a:
            tok[a] &= ~1
    return tok.tolist(), starts


def _keep(mode, V, device):
    if mode is None:
        return None
    if mode == "01":  # even words stay: whole sentences vanish, some keep one token
        k = (np.arange(V) % 2 == 0).astype(np.float32)
    else:
        k = np.random.default_rng(3).uniform(0.2, 0.9, V).astype(np.float32)
    return torch.from_numpy(k).to(device)


PV = 64


@pytest.fixture(scope="module", params=DEVS)
def pair_store(request):
    server, worker, _ = _store(PV, 4, request.param)
    yield server.raw, request.param
    server.shutdown()


MIXED = [(230, W, N, k) for W in (1, 2, 5) for N in (0, 1, 5) for k in (None, "01", "mid")]
SIZES = [(T, 2, 1, "mid") for T in (0, 1, 255, 256, 257, 1025, 3 * SCAN_BLOCK + 5)]
SIZES += [(257 * SCAN_BLOCK + 9, 1, 0, "mid")]  # a second pass over the block totals


@pytest.mark.parametrize("T,W,N,mode", MIXED + SIZES)
def test_pairs_equal_the_model(pair_store, T, W, N, mode):
    raw, device = pair_store
    tok, starts = _stream(T, W, PV)
    keep, (prob, alias) = _keep(mode, PV, device), _table(PV, device)
    seed = 0xFEEDFACECAFEBEEF + T + 7 * W + N
    ctok, pairs = window_plan_ref(tok, starts, None if keep is None else keep.cpu().numpy(),
                                  prob.cpu().numpy(), alias.cpu().numpy(), W, N, seed)
    ctr, ctx, neg, counts = raw.w2v_window_pairs(_i32(tok), _i32(starts), keep, prob, alias,
                                                 W, N, seed)
    assert counts.tolist() == [len(ctok), len(pairs)]
    assert ctr.tolist() == [p[1] for p in pairs]
    assert ctx.tolist() == [p[2] for p in pairs]
    assert neg.shape == (len(pairs), N) and neg.tolist() == [p[3] for p in pairs]


def _check_step(device, V, D, tok, starts, keep_mode, W, N, lr, seed, rows_of=None, power=0.75,
                centres=slice(None)):
    """One window step on a fresh store against the fp64 model: counts, the loss
    of `centres`, the emb and acc halves of `rows_of(pairs)` (default: all)."""
    server, worker, init = _store(V, D, device)
    try:
        keep, (prob, alias) = _keep(keep_mode, V, device), _table(V, device, power)
        ctok, pairs = window_plan_ref(tok, starts, None if keep is None else keep.cpu().numpy(),
                                      prob.cpu().numpy(), alias.cpu().numpy(), W, N, seed)
        loss, counts = server.raw.w2v_window_step(_i32(tok), _i32(starts), keep, prob, alias,
                                                  W, N, D, lr, EPS, seed)
        after = _pull_all(worker, V, D, device)
    finally:
        server.shutdown()
    T = len(tok)
    r64, l64 = window_step_ref(init, pairs, T, N, D, lr, EPS, torch.float64)
    r32, l32 = window_step_ref(init, pairs, T, N, D, lr, EPS, torch.float32)
    assert counts.tolist() == [len(ctok), len(pairs)]
    what = f"window {device} D={D} N={N}"
    assert_half_close(loss.cpu()[centres], l64[centres], l32[centres], f"{what} loss", "w2v_window")
    rows = slice(None) if rows_of is None else sorted(rows_of(pairs))
    for h, part in ((slice(0, D), "emb"), (slice(D, 2 * D), "acc")):
        assert_half_close(after[rows, h], r64[rows, h], r32[rows, h], f"{what} {part}", "w2v_window")
    return init, after, pairs, r64


def _distinct_seed(tok, starts, V, W, N):
    """A seed, found here on the CPU, for which the model's draws differ from
    each other and from the words of the stream (near-uniform table)."""
    prob, alias = _table(V, "cpu", power=0.05)
    for seed in range(1, 200):
        _, pairs = window_plan_ref(tok, starts, None, prob.numpy(), alias.numpy(), W, N, seed)
        draws = [w for p in pairs for w in p[3]]
        if len(set(draws)) == len(draws) and not set(draws) & set(tok):
            return seed
    raise AssertionError("no conflict-free seed below 200")


# every D of the issue's two lists; a multiple of 4 takes the float4 lanes
@pytest.mark.parametrize("D", [1, 63, 64, 65, 300, 511, 4, 256, 260, 512])
@pytest.mark.parametrize("N", [0, 3])
@pytest.mark.parametrize("device", DEVS)
def test_step_conflict_free(device, D, N):
    V, S = 1200, 5  # 10 centres: three workgroups
    tok = [7 * i + 3 for i in range(2 * S)]
    starts = list(range(0, 2 * S + 1, 2))
    seed = _distinct_seed(tok, starts, V, 2, N)
    _, _, pairs, _ = _check_step(device, V, D, tok, starts, None, 2, N, 0.1, seed, power=0.05)
    named = [w for p in pairs for w in [p[2]] + p[3]]
    assert len(pairs) == 2 * S and len(set(named)) == len(named)


@pytest.mark.parametrize("device", DEVS)
def test_step_held_centre(device):
    """Sentence (a, b, c), W = 1: b's second pair scores against the centre
    its first pair has moved. On the GPU waves a and c race for syn1[b]; only
    wave b touches the rows, and the loss, compared there."""
    V, N, tok = 400, 2, [11, 23, 37]
    seed = _distinct_seed(tok, [0, 3], V, 1, N)

    def rows_b(pairs):
        mine = [p for p in pairs if p[0] == 1]
        assert len(mine) == 2
        return {2 * 23} | {2 * w + 1 for p in mine for w in [p[2]] + p[3]}

    _check_step(device, V, 20, tok, [0, 3], None, 1, N, 0.5, seed,
                rows_of=None if device == "cpu" else rows_b, power=0.05,
                centres=slice(None) if device == "cpu" else [1])


@pytest.mark.parametrize("D", [20, 7])
@pytest.mark.parametrize("device", DEVS)
def test_step_real_windows_lr0(device, D):
    """Shared rows at lr = 0 (tests/test_kge_sides.py): embeddings keep their
    bits, accumulators are acc0 + sum g^2 whatever the order of the atomics."""
    V, W, N = 30, 5, 5
    rng = np.random.default_rng(8)
    lens = [3, 40, 7, 12, 25]
    starts = np.concatenate([[0], np.cumsum(lens)]).tolist()
    tok = rng.integers(0, V, size=starts[-1]).tolist()
    init, after, pairs, _ = _check_step(device, V, D, tok, starts, "mid", W, N, 0.0, 99)
    assert torch.equal(after[:, :D].view(torch.int32), init[:, :D].view(torch.int32))
    named = {2 * p[1] for p in pairs} | {2 * w + 1 for p in pairs for w in [p[2]] + p[3]}
    rest = sorted(set(range(2 * V)) - named)
    assert len(pairs) > len(tok) and len(named) > V and rest
    assert torch.equal(after[rest].view(torch.int32), init[rest].view(torch.int32))


@pytest.mark.parametrize("device", DEVS)
def test_guards(device):
    from adapm_amd import _C

    V, D = 16, 8
    server, worker, _ = _store(V, D, device)
    before = _pull_all(worker, V, D, device)
    prob, alias = _table(V, device)
    tok, st = _i32([1, 2, 3]), _i32([0, 3])
    step = server.raw.w2v_window_step
    with pytest.raises(RuntimeError, match="D = 516 is outside 1..512"):
        step(tok, st, None, prob, alias, 2, 1, 516, 0.1, EPS, 1)
    with pytest.raises(RuntimeError, match="N = 64 is outside 0..63"):
        step(tok, st, None, prob, alias, 2, 64, D, 0.1, EPS, 1)
    with pytest.raises(RuntimeError, match="starts decreases"):
        step(tok, _i32([0, 2, 1, 3]), None, prob, alias, 2, 1, D, 0.1, EPS, 1)
    with pytest.raises(RuntimeError, match="tok must be a contiguous 1-d int32"):
        step(tok.long(), st, None, prob, alias, 2, 1, D, 0.1, EPS, 1)
    with pytest.raises(RuntimeError, match=r"token id lies outside \[0, 16\)"):
        step(_i32([1, 16, 3]), st, None, prob, alias, 2, 1, D, 0.1, EPS, 1)
    assert torch.equal(_pull_all(worker, V, D, device), before)
    server.shutdown()
    # a rank of a two-rank world: the native server alone, no peers needed
    two = _C.Server(num_keys=2 * V, value_lengths=torch.tensor([2 * D]), rank=0, world=2,
                    num_channels=2, num_workers=1, device="cuda:0" if device == "cuda" else "cpu",
                    capacity_factor=2.0, techniques=0, location_caches=True,
                    device_cap_floats=0, host_spill_floats=0, sync_threshold=0.0)
    with pytest.raises(RuntimeError, match="requires a single rank"):
        two.w2v_window_step(tok, st, None, prob, alias, 2, 1, D, 0.1, EPS, 1)


def _model(seed):
    import adapm_amd
    from adapm_amd.models.word2vec import W2VConfig, Word2Vec

    V = 300
    cfg = W2VConfig(vocab_size=V, dim=16, negative=3, window=3, lr=0.05, seed=seed)
    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    adapm_amd.setup(num_keys=cfg.num_keys, num_threads=1, device="cpu")
    server = adapm_amd.Server(cfg.row)
    counts = np.arange(V, 0, -1)
    server.enable_sampling_support("local", True, "unigram", 0, V, counts=counts)
    model = Word2Vec(cfg, server, adapm_amd.Worker(0, server))
    model.set_vocab_counts(counts, sample=0.05)
    model.init_embeddings()
    return model


def test_model_tokens_fused():
    from adapm_amd.models.word2vec import make_synthetic_sentences, token_chunks

    (tokens, starts), = token_chunks(make_synthetic_sentences(60, 300, seed=2), 10 ** 9)
    runs = []
    for _ in range(2):
        model = _model(seed=21)
        args = model._window_args(tokens, starts)
        model._window_calls = 0  # the call below takes the same seed
        lists = [t.tolist() for t in model.server.raw.w2v_window_pairs(*args)]
        losses = [model.train_tokens_fused(tokens, starts, sync_loss=True) for _ in range(6)]
        runs.append((lists, model.last_counts.tolist()))
        model.server.shutdown()
    assert losses[-1] < losses[0], f"no learning {losses}"
    assert runs[0] == runs[1] and runs[0][1][1] > len(tokens)
