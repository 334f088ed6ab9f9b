"""word2vec SGNS on the adaptive parameter manager.

Rebuild of the reference app (reference apps/word2vec.cc):
  - keys: syn0(word w) = 2w, syn1(w) = 2w+1 (reference :83-105)
  - value layout [embedding(dim) | AdaGrad accum(dim)]
  - negatives from the unigram^0.75 distribution (reference :125-146)
    via the sampling manager
  - sentence look-ahead intent prefetch (reference :563-618)
  - fused SGNS step kernel (kernels_hip.hip k_w2v_step; reference
    :679-745)
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
    for ep in range(a.epochs):
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
