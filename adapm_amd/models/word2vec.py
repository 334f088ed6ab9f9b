"""word2vec SGNS on the adaptive parameter manager.

Rebuild of the reference app (reference apps/word2vec.cc):
  - keys: syn0(word w) = 2w, syn1(w) = 2w+1 (reference :83-105)
  - value layout [embedding(dim) | AdaGrad accum(dim)]
  - negatives from the unigram^0.75 distribution (reference :125-146)
    via the sampling manager
  - sentence look-ahead intent prefetch (reference :563-618)
  - fused SGNS step kernel (kernels_hip.hip k_w2v_step; reference
    :679-745)
  - window step from a token stream (w2v_window_hip.hip; the reference's
    loop shape, one context window per sentence position): subsampling,
    windows, pairs and negatives made on the device (train_tokens_fused)
  - checkpoint: word2vec text-format embedding export (reference
    :367-416)
"""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

import adapm_amd
from adapm_amd import _C

from ._step import StepModel


@dataclasses.dataclass
class W2VConfig:
    vocab_size: int = 1_000_000
    dim: int = 300
    window: int = 5
    negative: int = 5
    batch_pairs: int = 16384
    lr: float = 0.025
    eps: float = 1e-6
    lookahead_sentences: int = 100
    accum_init: float = 1.0  # AdaGrad accumulator start (0 diverges: first
                             # step would be lr*sign(g) per element)
    seed: int = 13

    @property
    def num_keys(self):
        return 2 * self.vocab_size

    @property
    def row(self):
        return 2 * self.dim


def syn0(words):
    return 2 * np.asarray(words, dtype=np.int64)


def syn1(words):
    return 2 * np.asarray(words, dtype=np.int64) + 1


class Word2Vec(StepModel):
    def __init__(self, cfg: W2VConfig, server, worker):
        super().__init__(cfg, server, worker)
        self._keep_prob = None
        self._keep_dev = None  # _keep_prob as fp32 on the store's device
        self.last_counts = None
        self.words = None  # real-corpus vocab strings (data_io.build_vocab)

    def init_embeddings(self):
        cfg = self.cfg

        def fill(ks, vals):
            # syn0 random-uniform (reference: (rand-0.5)/dim), syn1 zero
            mask = torch.from_numpy((ks % 2 == 0)).to(self.dev)
            vals[:, :cfg.dim] = (torch.rand(len(ks), cfg.dim, device=self.dev) - 0.5) / cfg.dim
            vals[~mask, :cfg.dim] = 0.0
            vals[:, cfg.dim:] = cfg.accum_init

        self._init_owned(cfg.num_keys, max(1, 2 ** 25 // cfg.row), fill)

    def set_vocab_counts(self, counts, sample: float = 1e-3):
        """Frequent-word subsampling (reference word2vec.cc 'sample'
        parameter): P(keep w) = min(1, sqrt(t/f) + t/f)."""
        f = np.asarray(counts, dtype=np.float64)
        f = f / f.sum()
        with np.errstate(divide="ignore"):
            keep = np.sqrt(sample / f) + sample / f
        self._keep_prob = np.minimum(1.0, keep)
        self._keep_dev = None

    def pairs_from_sentences(self, sentences):
        """(center, context) pairs with the reference's shrinking window,
        after frequent-word subsampling when counts are set."""
        if self._keep_prob is not None:
            sentences = [s[self.rng.random(len(s)) < self._keep_prob[s]] for s in sentences]
            sentences = [s for s in sentences if len(s) >= 2]
        ctr, ctx = [], []
        for sent in sentences:
            L = len(sent)
            for i, w in enumerate(sent):
                b = self.rng.integers(1, self.cfg.window + 1)
                for j in range(max(0, i - b), min(L, i + b + 1)):
                    if j != i:
                        ctr.append(w)
                        ctx.append(sent[j])
        return np.array(ctr, dtype=np.int64), np.array(ctx, dtype=np.int64)

    def signal_intent(self, sentences, start, end=0):
        words = np.unique(np.concatenate([np.asarray(s, dtype=np.int64) for s in sentences]))
        self.worker.intent(np.concatenate([syn0(words), syn1(words)]), start, end)

    def _launch(self, v, d, loss):
        cfg = self.cfg
        _C.w2v_sgns_step(*v, *d, loss, cfg.negative, cfg.dim, cfg.lr, cfg.eps)

    def train_pairs(self, ctr_words, ctx_words, sync_loss=False, neg_words=None):
        t0 = self._t0()
        if neg_words is None:
            neg_words = self._negatives(len(ctr_words) * self.cfg.negative,
                                        self.cfg.vocab_size)
        t0 = self._ph("sample", t0)
        # one pull of all rows: [ctr | ctx | neg]
        handle = self._begin_step([syn0(ctr_words), syn1(ctx_words), syn1(neg_words)])
        return self._finish_step(handle, self._launch, sync_loss, t0)

    def _classic_step(self, arrays):
        ctr, ctx, negs2 = arrays
        return self.train_pairs(ctr, ctx, sync_loss=False, neg_words=negs2.reshape(-1))

    def _fused_identity_step(self, arrays):
        return self._fused_raw(self.server.raw.w2v_step_fused, arrays)

    def _fused_general_step(self, arrays):
        return self._fused_raw(self.server.raw.w2v_step_fused_general, arrays)

    def _fused_raw(self, step, arrays):
        cfg = self.cfg
        ctr, ctx, negs2 = arrays
        return step(torch.from_numpy(syn0(ctr)), torch.from_numpy(syn1(ctx)),
                    torch.from_numpy(syn1(negs2.reshape(-1))),
                    cfg.negative, cfg.dim, cfg.lr, cfg.eps)

    def train_pairs_fused(self, ctr_words, ctx_words, sync_loss=False,
                          force_general=False):
        """Fused slab-direct SGNS step. world==1 + identity layout uses
        the zero-host-work kernel (Server.w2v_step_fused); otherwise the
        general offsets path runs the fused kernel on all-local pairs
        and routes the remote remainder through the classic path."""
        cfg = self.cfg
        B = len(ctr_words)
        neg_words = np.ascontiguousarray(self._negatives(B * cfg.negative, cfg.vocab_size),
                                         dtype=np.int64)
        arrays = (np.asarray(ctr_words, dtype=np.int64), np.asarray(ctx_words, dtype=np.int64),
                  neg_words.reshape(B, cfg.negative))
        return self._fused_step(arrays, sync_loss, force_general)

    # ------------------------------------------------ token-stream training

    _window_calls = 0  # window launches so far: the step counter of the seed

    def _window_args(self, tokens, starts):
        """(tok, starts, keep, prob, alias, window, negative, seed) of the next
        window call. Every call takes seed = mix64(mix64(mix64(cfg.seed) ^ rank)
        ^ n), n = 1, 2, ... counting this model's window calls (the rule of
        kge._drop_tail): two models with equal seeds make equal pairs."""
        from .kge import _mix64

        cfg = self.cfg
        dist = self.server.sampling.dist if self.server.sampling is not None else None
        if dist is None or not hasattr(dist, "alias") or dist.key_of is not None:
            raise RuntimeError("train_tokens_fused draws its negatives from the server's "
                               "unigram sampler over word ids 0..V")
        if self._keep_prob is not None and self._keep_dev is None:
            self._keep_dev = torch.from_numpy(self._keep_prob.astype(np.float32)).to(self.dev)
        self._window_calls += 1
        seed = _mix64(_mix64(_mix64(cfg.seed) ^ self.rank) ^ self._window_calls)
        tok = torch.from_numpy(np.ascontiguousarray(tokens, dtype=np.int32))
        st = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int32))
        return (tok, st, self._keep_dev, dist.prob.to(self.dev), dist.alias.to(self.dev),
                cfg.window, cfg.negative, seed)

    def train_tokens_fused(self, tokens, starts, sync_loss=False):
        """One step over a token stream: `tokens` are word ids in corpus
        order, sentence s is tokens[starts[s]:starts[s+1]]. Subsampling,
        windows, pairs and negatives are made on the device (kernels.h,
        w2v_window_step). With one rank and the identity layout the window
        kernel trains on the slab itself; otherwise Server.w2v_window_pairs
        makes the same pairs and batch_pairs-sized slices of them, with
        their drawn negatives, go through the fused pair step.

        Returns the per-centre (window kernel) or per-pair losses without a
        host sync, or with sync_loss the mean loss per pair. `last_counts`
        holds (kept tokens, pairs) of the call as a device tensor."""
        cfg = self.cfg
        raw = self.server.raw
        tok, st, keep, prob, alias, W, N, seed = self._window_args(tokens, starts)
        if self.world == 1 and raw.layout_identity() and cfg.dim <= _C.W2V_WINDOW_MAX_DIM:
            loss, self.last_counts = raw.w2v_window_step(tok, st, keep, prob, alias, W, N,
                                                         cfg.dim, cfg.lr, cfg.eps, seed)
        else:
            ctr, ctx, neg, self.last_counts = raw.w2v_window_pairs(tok, st, keep, prob, alias,
                                                                   W, N, seed)
            ctr, ctx, neg = (t.cpu().numpy() for t in (ctr, ctx, neg))
            parts = [self._fused_step((ctr[i:i + cfg.batch_pairs], ctx[i:i + cfg.batch_pairs],
                                       neg[i:i + cfg.batch_pairs]), False, False)
                     for i in range(0, len(ctr), cfg.batch_pairs)]
            loss = torch.cat(parts) if parts else torch.zeros(0, device=self.dev)
        if not sync_loss:
            return loss
        pairs = int(self.last_counts[1].item())
        return float(loss.sum().item()) / pairs if pairs else 0.0

    def export_text(self, path: str, max_words: int = None, chunk: int = 65536):
        """word2vec text format: '<vocab> <dim>' header then word vectors
        (reference word2vec.cc:367-416)."""
        self.drain()
        self.worker.wait_sync()
        self.worker.barrier()
        if self.rank == 0:
            n = min(self.cfg.vocab_size, max_words or self.cfg.vocab_size)
            with open(path, "w") as f:
                f.write(f"{n} {self.cfg.dim}\n")
                for i in range(0, n, chunk):
                    ks = syn0(np.arange(i, min(i + chunk, n)))
                    buf = np.zeros((len(ks), self.cfg.row), dtype=np.float32)
                    self.worker.pull(ks, buf)
                    for j, wv in enumerate(buf[:, :self.cfg.dim]):
                        name = self.words[i + j] if self.words else f"w{i+j}"
                        f.write(f"{name} " + " ".join(f"{x:.6f}" for x in wv) + "\n")
        self.worker.barrier()

    def export_binary(self, path: str, max_words: int = None, chunk: int = 65536):
        """Classic word2vec BINARY format (reference word2vec.cc:367-380)."""
        from .data_io import export_word2vec_binary

        self.drain()
        self.worker.wait_sync()
        self.worker.barrier()
        if self.rank == 0:
            n = min(self.cfg.vocab_size, max_words or self.cfg.vocab_size)
            vecs = np.zeros((n, self.cfg.dim), dtype=np.float32)
            for i in range(0, n, chunk):
                ks = syn0(np.arange(i, min(i + chunk, n)))
                buf = np.zeros((len(ks), self.cfg.row), dtype=np.float32)
                self.worker.pull(ks, buf)
                vecs[i:i + len(ks)] = buf[:, :self.cfg.dim]
            names = self.words[:n] if self.words else [f"w{i}" for i in range(n)]
            export_word2vec_binary(path, names, vecs)
        self.worker.barrier()


def make_synthetic_sentences(n_sentences, vocab_size, mean_len=12, zipf_a=1.2, seed=0):
    """Zipf-distributed synthetic corpus (no network for real data)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_sentences):
        L = max(2, int(rng.poisson(mean_len)))
        words = rng.zipf(zipf_a, size=L)
        out.append(np.minimum(words - 1, vocab_size - 1).astype(np.int64))
    return out


def token_chunks(sentences, chunk_tokens):
    """[(tokens, starts)]: the sentences as int32 token streams of about
    chunk_tokens tokens each, whole sentences only, for train_tokens_fused."""
    out, cur, n = [], [], 0
    for s in list(sentences) + [None]:
        if cur and (s is None or n + len(s) > chunk_tokens):
            starts = np.concatenate([[0], np.cumsum([len(x) for x in cur])]).astype(np.int32)
            out.append((np.concatenate(cur).astype(np.int32), starts))
            cur, n = [], 0
        if s is not None:
            cur.append(s)
            n += len(s)
    return out


def main():
    """CLI (rebuild of reference apps/word2vec.cc): SGNS on a synthetic
    corpus with subsampling + unigram negatives; exports embeddings."""
    import argparse
    import time

    import adapm_amd as _a

    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=100_000)
    ap.add_argument("--dim", type=int, default=100)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--sentences", type=int, default=20_000)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch-pairs", type=int, default=16384)
    ap.add_argument("--output", type=str, default="")
    ap.add_argument("--binary-output", type=str, default="",
                    help="also write the classic word2vec binary format")
    ap.add_argument("--corpus", type=str, default="",
                    help="train on a real text corpus (vocabulary built from the "
                         "file, reference LearnVocabFromTrainFile); default: synthetic")
    ap.add_argument("--min-count", type=int, default=5)
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--device-pairs", action="store_true",
                    help="train from the token stream: subsampling, windows, pairs and "
                         "negatives are made on the device (train_tokens_fused)")
    ap.add_argument("--chunk-tokens", type=int, default=65536,
                    help="with --device-pairs: tokens per call, in whole sentences")
    a = ap.parse_args()

    words = None
    if a.corpus:
        from .data_io import build_vocab, read_sentences

        words, wcounts, word2id = build_vocab(a.corpus, min_count=a.min_count,
                                              max_vocab=a.vocab)
        a.vocab = len(words)
        counts = wcounts.astype(np.float64)
    else:
        counts = (1.0 / np.arange(1, a.vocab + 1)) ** 0.75 * 1e9

    cfg = W2VConfig(vocab_size=a.vocab, dim=a.dim, window=a.window, negative=a.negative,
                    batch_pairs=a.batch_pairs)
    _a.setup(num_keys=cfg.num_keys, num_threads=1, device=a.device)
    server = _a.Server(cfg.row)
    server.enable_sampling_support("local", True, "unigram", 0, a.vocab, counts=counts)
    worker = _a.Worker(0, server)
    model = Word2Vec(cfg, server, worker)
    model.set_vocab_counts(counts)
    model.words = words
    model.init_embeddings()
    rank = server.my_rank()
    world = server.rt.world
    if a.corpus:
        sents = [s for i, s in enumerate(read_sentences(a.corpus, word2id))
                 if i % world == rank]  # sentence partition (reference file-offset split)
    else:
        sents = make_synthetic_sentences(a.sentences // world, a.vocab, seed=rank)
    chunks = token_chunks(sents, a.chunk_tokens) if a.device_pairs else []
    for ep in range(a.epochs if a.device_pairs else 0):
        t0 = time.time()
        loss_sum = torch.zeros((), dtype=torch.float64, device=model.dev)
        done = torch.zeros(2, dtype=torch.int64, device=model.dev)
        for tokens, starts in chunks:
            if world > 1:
                model.signal_intent([tokens], worker.current_clock() + 1,
                                    worker.current_clock() + 3)
            loss_sum += model.train_tokens_fused(tokens, starts).sum()
            done += model.last_counts
            worker.advance_clock()
        model.drain()
        kept, pairs = (int(x) for x in done.tolist())  # the epoch's one host sync
        total = worker.allreduce(float(loss_sum.item()) / max(pairs, 1))
        if rank == 0:
            dt = time.time() - t0
            print(f"[w2v] epoch {ep}: loss {total / world:.4f} ({kept} words, {pairs} pairs, "
                  f"{dt:.1f}s, {sum(len(t) for t, _ in chunks) / dt:.0f} words/s)")
    for ep in range(0 if a.device_pairs else a.epochs):
        t0 = time.time()
        ctr, ctx = model.pairs_from_sentences(sents)
        losses = []
        for i in range(0, len(ctr), a.batch_pairs):
            model.signal_intent([np.unique(ctr[i:i + a.batch_pairs])],
                                worker.current_clock() + 1, worker.current_clock() + 3)
            losses.append(model.train_pairs(ctr[i:i + a.batch_pairs],
                                            ctx[i:i + a.batch_pairs], sync_loss=True))
            worker.advance_clock()
        model.drain()
        total = worker.allreduce(float(np.mean(losses)))
        if rank == 0:
            print(f"[w2v] epoch {ep}: loss {total / world:.4f} "
                  f"({len(ctr)} pairs, {time.time()-t0:.1f}s)")
    if a.output:
        model.export_text(a.output, max_words=min(a.vocab, 10000))
        if rank == 0:
            print(f"[w2v] embeddings -> {a.output}")
    if a.binary_output:
        model.export_binary(a.binary_output, max_words=min(a.vocab, 10000))
        if rank == 0:
            print(f"[w2v] binary embeddings -> {a.binary_output}")
    worker.finalize()
    server.shutdown()


if __name__ == "__main__":
    main()
