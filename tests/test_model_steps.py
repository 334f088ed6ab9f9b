"""Characterization of the Python half of the training step in
adapm_amd/models: the classic pull/kernel/push step, the negative draw,
the bounded async pushes and the fused dispatch with its one-step miss
deferral, for ComplEx, Word2Vec and MF.

No process group and no store: the model runs on a fake server whose
`*_step_fused_general` answers from a script, and on a fake worker that
logs every pull/push and fills pulled rows from their keys. The real
`_C` CPU twins run the classic kernels."""
import types

import numpy as np
import pytest
import torch

from adapm_amd import _C
from adapm_amd.models.kge import ComplEx, ComplExConfig
from adapm_amd.models.mf import MF, MFConfig
from adapm_amd.models.word2vec import W2VConfig, Word2Vec, syn0, syn1

B = 4
NEG = 2
DIM = 8
ROW = 2 * DIM
ENT = 32
REL = 4
RANK = 1            # process rank of the fake runtime (seeds the model rng)
PULL_TICKET0 = 10_000  # pull tickets start here, push tickets at 0


def fake_rows(keys):
    """What the fake store holds for `keys`: a deterministic function of
    the key, so a swapped or shifted view changes the kernel's output.
    Positive throughout (the upper half is the AdaGrad accumulator)."""
    k = torch.from_numpy(np.asarray(keys, dtype=np.int64))
    col = torch.arange(ROW, dtype=torch.float32)
    return (0.05 + 0.01 * (k % 7).float()[:, None] + 0.001 * col[None, :]).contiguous()


class FakeWorker:
    def __init__(self, push_ticket=None):
        self.log = []      # ("pull", keys) / ("push", keys, deltas)
        self.waits = []
        self.sample_calls = []
        self._pull_ts = PULL_TICKET0
        self._push_ts = 0
        self._fixed_push_ticket = push_ticket

    def pull(self, keys, vals, async_=False):
        keys = np.array(keys, dtype=np.int64)
        self.log.append(("pull", keys))
        vals.view(len(keys), ROW).copy_(fake_rows(keys))
        self._pull_ts += 1
        return self._pull_ts - 1

    def push(self, keys, vals, async_=False):
        self.log.append(("push", np.array(keys, dtype=np.int64), vals.clone()))
        if self._fixed_push_ticket is not None:
            return self._fixed_push_ticket
        self._push_ts += 1
        return self._push_ts - 1

    def wait(self, ts):
        self.waits.append(ts)

    @property
    def push_waits(self):
        return [t for t in self.waits if 0 <= t < PULL_TICKET0]

    def current_clock(self):
        return 0

    def prepare_sample(self, K, start=0, end=0):
        self.sample_calls.append(("prepare", K))
        return 7

    def finish_sample(self, sid):
        self.sample_calls.append(("finish", sid))


class FakeSampling:
    """Sampling manager: hands out consecutive keys, logs on the worker."""

    def __init__(self, num_keys):
        self.num_keys = num_keys
        self.next = 0

    def pull(self, worker, sid, n):
        worker.sample_calls.append(("pull", sid, n))
        out = (self.next + np.arange(n, dtype=np.int64)) % self.num_keys
        self.next += n
        return out


class FakeRaw:
    """Scripted `*_step_fused_general`: records its arguments, returns
    (loss of len B' - len(missed), missed) from the next script entry."""

    def __init__(self, script):
        self.script = list(script)
        self.calls = []
        self.losses = []

    def layout_identity(self):
        return False

    def _general(self, *args):
        self.calls.append([a.numpy().copy() if torch.is_tensor(a) else a for a in args])
        missed = self.script.pop(0)
        n = len(args[0]) - len(missed)
        loss = torch.arange(n, dtype=torch.float32) + 100.0 * len(self.calls)
        self.losses.append(loss)
        return loss, torch.tensor(missed, dtype=torch.int64)

    kge_step_fused_general = _general
    w2v_step_fused_general = _general
    mf_step_fused_general = _general


class Kind:
    """What differs between the three models, for the tests only. A batch
    is described by `rows`: one int64 row of keys per sample, the `fixed`
    per-sample roles first, then its negatives; `extra` is a per-sample
    float array (MF ratings) or None."""

    def __init__(self, name):
        self.name = name
        self.fixed = {"kge": 3, "w2v": 2, "mf": 2}[name]
        self.neg = 0 if name == "mf" else NEG
        self.num_neg_keys = {"kge": ENT, "w2v": ENT, "mf": 0}[name]

    def make(self, script=(), sampling=None, push_ticket=None):
        worker = FakeWorker(push_ticket)
        raw = FakeRaw(script)
        rt = types.SimpleNamespace(device=torch.device("cpu"), rank=RANK, world=2)
        server = types.SimpleNamespace(rt=rt, sampling=sampling, raw=raw)
        if self.name == "kge":
            cfg = ComplExConfig(num_entities=ENT, num_relations=REL, dim=DIM,
                                neg_samples=NEG, batch_size=B, seed=3)
            model = ComplEx(cfg, server, worker)
        elif self.name == "w2v":
            cfg = W2VConfig(vocab_size=ENT, dim=DIM, negative=NEG, seed=3)
            model = Word2Vec(cfg, server, worker)
        else:
            cfg = MFConfig(num_rows=ENT, num_cols=REL, rank=DIM, seed=3)
            model = MF(cfg, server, worker)
        return model, worker, raw

    def batch(self, i):
        """Model-level arguments of batch i (distinct ids per batch)."""
        g = np.random.default_rng(100 + i)
        if self.name == "kge":
            return (np.stack([g.integers(0, ENT, B), g.integers(0, REL, B),
                              g.integers(0, ENT, B)], axis=1).astype(np.int64),)
        if self.name == "w2v":
            return g.integers(0, ENT, B), g.integers(0, ENT, B)
        return (g.integers(0, ENT, B), g.integers(0, REL, B),
                g.normal(size=B).astype(np.float32))

    def fixed_rows(self, batch):
        """[B, fixed] store keys of the per-sample roles."""
        if self.name == "kge":
            t = batch[0]
            return np.stack([t[:, 0], ENT + t[:, 1], t[:, 2]], axis=1)
        if self.name == "w2v":
            return np.stack([syn0(batch[0]), syn1(batch[1])], axis=1)
        return np.stack([batch[0], ENT + batch[1]], axis=1).astype(np.int64)

    def neg_keys(self, draws):
        """Store keys of drawn negative ids, [B, NEG]."""
        d = np.asarray(draws, dtype=np.int64).reshape(-1, NEG)
        return syn1(d) if self.name == "w2v" else d

    def rows(self, batch, draws=None):
        f = self.fixed_rows(batch)
        return f if self.name == "mf" else np.concatenate([f, self.neg_keys(draws)], axis=1)

    def extra(self, batch):
        return batch[2] if self.name == "mf" else None

    def classic(self, model, batch, **kw):
        fn = model.train_pairs if self.name == "w2v" else model.train_batch
        return fn(*batch, **kw)

    def fused(self, model, batch, **kw):
        fn = model.train_pairs_fused if self.name == "w2v" else model.train_batch_fused
        return fn(*batch, force_general=True, **kw)

    def call_rows(self, call):
        """[B', fixed + NEG] key rows (and the ratings) of one recorded
        general-step call."""
        n = len(call[0])
        cols = [call[j].reshape(n, 1) for j in range(self.fixed)]
        if self.name == "mf":
            return np.concatenate(cols, axis=1), call[2]
        assert call[self.fixed + 1] == NEG
        return np.concatenate(cols + [call[self.fixed].reshape(n, NEG)], axis=1), None

    def classic_keys(self, rows):
        """Role-wise concatenation the classic step pulls and pushes:
        [s|r|o|neg], [ctr|ctx|neg], [w|h]."""
        parts = [rows[:, j] for j in range(self.fixed)]
        if self.neg:
            parts.append(rows[:, self.fixed:].reshape(-1))
        return np.concatenate(parts)

    def direct(self, model, rows, extra):
        """Deltas and loss of a direct `_C.*_step` call on the rows the
        fake store holds for `rows`."""
        cfg = model.cfg
        n = len(rows)
        parts = [rows[:, j] for j in range(self.fixed)]
        if self.neg:
            parts.append(rows[:, self.fixed:].reshape(-1))
        v = [fake_rows(p) for p in parts]
        d = [torch.empty_like(t) for t in v]
        loss = torch.empty(n, dtype=torch.float32)
        if self.name == "kge":
            _C.kge_complex_step(*v, *d, loss, NEG, DIM, cfg.lr, cfg.eps)
        elif self.name == "w2v":
            _C.w2v_sgns_step(*v, *d, loss, NEG, DIM, cfg.lr, cfg.eps)
        else:
            _C.mf_update_step(*v, torch.from_numpy(np.asarray(extra, dtype=np.float32)),
                              *d, loss, DIM, cfg.lr, cfg.lam, cfg.eps)
        return torch.cat([t.reshape(-1) for t in d]), loss

    def draws(self, model, n_steps):
        """The negative ids the model's rng will draw over n_steps steps."""
        if not self.neg:
            return [None] * n_steps
        g = np.random.default_rng(model.cfg.seed + RANK)
        return [g.integers(0, self.num_neg_keys, size=B * NEG, dtype=np.int64)
                for _ in range(n_steps)]

    def assert_classic_step(self, model, log, rows, extra):
        """`log` is exactly one classic step over `rows`: one pull and one
        push of the role-wise keys, deltas bit-equal to the direct call."""
        assert [e[0] for e in log] == ["pull", "push"]
        keys = self.classic_keys(rows)
        np.testing.assert_array_equal(log[0][1], keys)
        np.testing.assert_array_equal(log[1][1], keys)
        deltas, loss = self.direct(model, rows, extra)
        assert torch.equal(log[1][2].reshape(-1), deltas)
        return loss


KINDS = [Kind("kge"), Kind("w2v"), Kind("mf")]
NEG_KINDS = KINDS[:2]
ids = lambda k: k.name  # noqa: E731


def _sub(x, idx):
    return None if x is None else x[idx]


def _cat(a, b):
    return None if a is None else np.concatenate([a, b])


# ------------------------------------------------------ deferral schedule


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_deferral_schedule(kind):
    model, worker, raw = kind.make(script=[[1, 3], [0, 4], []])
    draws = kind.draws(model, 3)
    batches = [kind.batch(i) for i in range(3)]
    new = [(kind.rows(b, d), kind.extra(b)) for b, d in zip(batches, draws)]

    # step 1: samples 1 and 3 miss for the first time -> deferred
    out = kind.fused(model, batches[0], sync_loss=False)
    assert out.numel() == 2
    rows1, x1 = kind.call_rows(raw.calls[0])
    np.testing.assert_array_equal(rows1, new[0][0])
    assert worker.log == []
    assert model._deferred is not None

    # step 2: the two deferred samples first, then the four new ones,
    # each with its own negatives
    out = kind.fused(model, batches[1], sync_loss=False)
    rows2, x2 = kind.call_rows(raw.calls[1])
    want2 = np.concatenate([new[0][0][[1, 3]], new[1][0]])
    wantx2 = _cat(_sub(new[0][1], [1, 3]), new[1][1])
    np.testing.assert_array_equal(rows2, want2)
    if x2 is not None:
        np.testing.assert_array_equal(x2, wantx2)
    # index 0 missed twice: classic path now, its own keys and negatives
    closs = kind.assert_classic_step(model, worker.log, want2[[0]], _sub(wantx2, [0]))
    assert out.numel() == 4 + 1
    assert torch.equal(out, torch.cat([raw.losses[1], closs]))
    assert model._deferred is not None

    # step 3: index 4 of step 2 comes back first and hits; nothing is left
    n_log = len(worker.log)
    out = kind.fused(model, batches[2], sync_loss=False)
    rows3, x3 = kind.call_rows(raw.calls[2])
    np.testing.assert_array_equal(rows3, np.concatenate([want2[[4]], new[2][0]]))
    if x3 is not None:
        np.testing.assert_array_equal(x3, _cat(wantx2[[4]], new[2][1]))
    assert out.numel() == 5
    assert model._deferred is None
    assert len(worker.log) == n_log
    assert len(raw.calls) == 3


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_drain_flushes_deferred_through_classic(kind):
    model, worker, raw = kind.make(script=[[2]])
    batch = kind.batch(0)
    rows = kind.rows(batch, kind.draws(model, 1)[0])
    kind.fused(model, batch, sync_loss=False)
    assert worker.log == [] and model._deferred is not None
    model.drain()
    kind.assert_classic_step(model, worker.log, rows[[2]], _sub(kind.extra(batch), [2]))
    assert model._deferred is None
    assert len(raw.calls) == 1
    assert model._pending == [] and worker.push_waits == [0]


# ------------------------------------------------------ return-value rules


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_all_missed_first_step_returns_zero_or_empty(kind):
    model, _, _ = kind.make(script=[[0, 1, 2, 3]])
    out = kind.fused(model, kind.batch(0), sync_loss=True)
    assert isinstance(out, float) and out == 0.0

    model, worker, _ = kind.make(script=[[0, 1, 2, 3]])
    out = kind.fused(model, kind.batch(0), sync_loss=False)
    assert torch.is_tensor(out) and out.numel() == 0
    assert worker.log == []


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_no_miss_returns_general_loss_unchanged(kind):
    model, worker, raw = kind.make(script=[[], []])
    out = kind.fused(model, kind.batch(0), sync_loss=False)
    assert torch.equal(out, raw.losses[0]) and out.numel() == B
    out = kind.fused(model, kind.batch(1), sync_loss=True)
    assert isinstance(out, float) and out == float(raw.losses[1].mean().item())
    assert worker.log == [] and model._deferred is None


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_fused_falls_back_to_classic_off_gpu(kind):
    """Without force_general a CPU store takes the classic step."""
    model, worker, raw = kind.make()
    batch = kind.batch(0)
    fn = model.train_pairs_fused if kind.name == "w2v" else model.train_batch_fused
    out = fn(*batch, sync_loss=False)
    rows = kind.rows(batch, kind.draws(model, 1)[0])
    loss = kind.assert_classic_step(model, worker.log, rows, kind.extra(batch))
    assert torch.equal(out, loss)
    assert raw.calls == []


# ------------------------------------------------------ negative stream


@pytest.mark.parametrize("kind", NEG_KINDS, ids=ids)
def test_negative_stream_is_the_model_rng(kind):
    """sampling=None: the negatives are successive draws of
    default_rng(seed + rank), drawn before the deferral merge (so a step
    that carries deferred samples still draws exactly B*N)."""
    model, _, raw = kind.make(script=[[1, 3], [0, 4], []])
    draws = kind.draws(model, 3)
    n_def = [0, 2, 1]
    for i in range(3):
        kind.fused(model, kind.batch(i), sync_loss=False)
        rows, _ = kind.call_rows(raw.calls[i])
        np.testing.assert_array_equal(rows[n_def[i]:, kind.fixed:], kind.neg_keys(draws[i]))
    # classic steps continue the same stream
    g = np.random.default_rng(model.cfg.seed + RANK)
    g.integers(0, ENT, size=3 * B * NEG, dtype=np.int64)
    nxt = g.integers(0, ENT, size=B * NEG, dtype=np.int64)
    model2, worker2, _ = kind.make()
    for i in range(3):
        kind.classic(model2, kind.batch(i))
    worker2.log.clear()
    kind.classic(model2, kind.batch(3))
    np.testing.assert_array_equal(worker2.log[0][1][kind.fixed * B:],
                                  kind.neg_keys(nxt).reshape(-1))


@pytest.mark.parametrize("kind", NEG_KINDS, ids=ids)
@pytest.mark.parametrize("fused", [False, True], ids=["classic", "fused"])
def test_sampling_manager_called_once_per_step(kind, fused):
    model, worker, raw = kind.make(script=[[], [], []], sampling=FakeSampling(ENT))
    for i in range(3):
        worker.sample_calls.clear()
        if fused:
            kind.fused(model, kind.batch(i), sync_loss=False)
            rows, _ = kind.call_rows(raw.calls[i])
            got = rows[:, kind.fixed:].reshape(-1)
        else:
            worker.log.clear()
            kind.classic(model, kind.batch(i))
            got = worker.log[0][1][kind.fixed * B:]
        assert worker.sample_calls == [("prepare", B * NEG), ("pull", 7, B * NEG),
                                       ("finish", 7)]
        want = (i * B * NEG + np.arange(B * NEG)) % ENT
        np.testing.assert_array_equal(got, kind.neg_keys(want).reshape(-1))


# ------------------------------------------------------ classic step layout


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_classic_step_layout_and_deltas(kind):
    model, worker, _ = kind.make()
    batch = kind.batch(0)
    out = kind.classic(model, batch, sync_loss=False)
    rows = kind.rows(batch, kind.draws(model, 1)[0])
    loss = kind.assert_classic_step(model, worker.log, rows, kind.extra(batch))
    assert torch.equal(out, loss)
    assert worker.waits == [PULL_TICKET0] and model._pending == [0]

    model, _, _ = kind.make()
    out = kind.classic(model, batch, sync_loss=True)
    assert isinstance(out, float) and out == float(loss.mean().item())


def test_explicit_negatives_bypass_the_draw():
    """neg_keys / neg_words given by the caller are used as they are and
    consume nothing from the rng."""
    for kind in NEG_KINDS:
        model, worker, _ = kind.make()
        batch = kind.batch(0)
        negs = np.arange(B * NEG, dtype=np.int64)[::-1].copy()
        kw = {"neg_words": negs} if kind.name == "w2v" else {"neg_keys": negs}
        kind.classic(model, batch, sync_loss=False, **kw)
        kind.assert_classic_step(model, worker.log, kind.rows(batch, negs), None)
        first = kind.draws(model, 1)[0]
        np.testing.assert_array_equal(
            model.rng.integers(0, ENT, size=B * NEG, dtype=np.int64), first)


# ------------------------------------------------------ pending cap


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_pending_cap_waits_fifo(kind):
    model, worker, _ = kind.make()
    batch = kind.batch(0)
    for _ in range(70):
        kind.classic(model, batch, sync_loss=False)
    assert worker.push_waits == [0, 1, 2, 3, 4, 5]
    assert model._pending == list(range(6, 70))
    model.drain()
    assert worker.push_waits == list(range(70))
    assert model._pending == []


@pytest.mark.parametrize("kind", KINDS, ids=ids)
def test_local_push_is_never_queued(kind):
    model, worker, _ = kind.make(push_ticket=-1)
    for i in range(3):
        kind.classic(model, kind.batch(i), sync_loss=False)
        assert model._pending == []
    model.drain()
    assert -1 not in worker.waits and worker.push_waits == []


# ------------------------------------------------------ prefetch


def test_prefetch_pair_equals_train_batch():
    kind = KINDS[0]
    batches = [kind.batch(i)[0] for i in range(2)]
    ref, ref_worker, _ = kind.make()
    for t in batches:
        ref.train_batch(t, sync_loss=False)

    model, worker, _ = kind.make()
    handles = [model.prefetch(t) for t in batches]  # two pulls in flight
    assert [e[0] for e in worker.log] == ["pull", "pull"]
    assert worker.waits == []
    losses = [model.train_prefetched(h) for h in handles]
    assert [e[0] for e in worker.log] == ["pull", "pull", "push", "push"]
    assert worker.waits == [PULL_TICKET0, PULL_TICKET0 + 1]
    assert model._pending == [0, 1]

    pulls = [e for e in ref_worker.log if e[0] == "pull"]
    pushes = [e for e in ref_worker.log if e[0] == "push"]
    for i in range(2):
        np.testing.assert_array_equal(worker.log[i][1], pulls[i][1])
        np.testing.assert_array_equal(worker.log[2 + i][1], pushes[i][1])
        assert torch.equal(worker.log[2 + i][2], pushes[i][2])
        assert losses[i].numel() == B
    assert isinstance(model.train_prefetched(model.prefetch(batches[0]), sync_loss=True), float)
