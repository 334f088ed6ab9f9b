#!/usr/bin/env python3
"""word2vec SGNS benchmark (BASELINE config 2: dim=300, 1M-vocab synthetic
corpus, 1x MI355X). Same JSON contract as bench.py; metric = SGNS
(center, context) pairs trained per second, whole job."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bench_tokens(args, model, server, worker):
    """Corpus throughput: words/s and pairs/s from sentences to trained pairs,
    pair generation included."""
    from adapm_amd.models.word2vec import make_synthetic_sentences, token_chunks

    total = args.warmup + args.steps
    sents = make_synthetic_sentences(int(total * args.tokens / 11) + 64, args.vocab, seed=2000)
    chunks = token_chunks(sents, args.tokens)[:total]
    assert len(chunks) == total, "too few synthetic sentences for the requested steps"
    is_cuda = server.rt.device.type == "cuda"
    bp = model.cfg.batch_pairs
    pairs = torch.zeros((), dtype=torch.int64, device=server.rt.device)

    def step(tok, starts):
        nonlocal pairs
        if not args.host_pairs:
            model.train_tokens_fused(tok, starts)
            pairs += model.last_counts[1]
            return
        ctr, ctx = model.pairs_from_sentences(
            [tok[a:b].astype(np.int64) for a, b in zip(starts[:-1], starts[1:])])
        for i in range(0, len(ctr), bp):
            model.train_pairs_fused(ctr[i:i + bp], ctx[i:i + bp])
        pairs += len(ctr)

    for c in chunks[:args.warmup]:
        step(*c)
    model.drain()
    if is_cuda:
        torch.cuda.synchronize()
    pairs.zero_()
    t0 = time.perf_counter()
    for c in chunks[args.warmup:]:
        step(*c)
    model.drain()
    if is_cuda:
        torch.cuda.synchronize()
    el = time.perf_counter() - t0
    words = sum(len(t) for t, _ in chunks[args.warmup:])
    print(json.dumps({
        "metric": "sgns_corpus_words_per_s", "value": words / el, "unit": "words/s",
        "pairs_per_s": int(pairs.item()) / el, "pairs": int(pairs.item()), "words": words,
        "ms_per_chunk": 1000 * el / args.steps, "steps": args.steps, "warmup": args.warmup,
        "higher_is_better": True, "dtype": "fp32", "data": "synthetic",
        "config": {"model": "word2vec_sgns", "pairs_made": "host" if args.host_pairs else "device",
                   "vocab": args.vocab, "dim": args.dim, "window": args.window,
                   "negative": args.negative, "chunk_tokens": args.tokens},
    }), flush=True)
    worker.finalize()
    server.shutdown()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=300)
    ap.add_argument("--negative", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=65536, help="pairs per step")
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--no-fused", action="store_true",
                    help="disable the fused slab-direct kernel (single-rank GPU fast path)")
    ap.add_argument("--tokens", type=int, default=0,
                    help="time corpus training instead: synthetic sentences in chunks of this "
                         "many tokens through train_tokens_fused (pairs made on the device)")
    ap.add_argument("--host-pairs", action="store_true",
                    help="with --tokens: the same chunks through pairs_from_sentences and "
                         "train_pairs_fused (pairs made in Python)")
    ap.add_argument("--window", type=int, default=5)
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", str(args.gpus)))

    import adapm_amd
    from adapm_amd.models.word2vec import W2VConfig, Word2Vec

    cfg = W2VConfig(vocab_size=args.vocab, dim=args.dim, negative=args.negative,
                    window=args.window)
    adapm_amd.setup(num_keys=cfg.num_keys, num_threads=1, device=args.device,
                    capacity_factor=2.0, max_sync_per_sec=2000.0)
    server = adapm_amd.Server(cfg.row)
    counts = (1.0 / np.arange(1, args.vocab + 1)) ** 0.7 * 1e9  # Zipf-ish counts
    server.enable_sampling_support("local", True, "unigram", 0, args.vocab, counts=counts)
    worker = adapm_amd.Worker(0, server)
    model = Word2Vec(cfg, server, worker)
    model.set_vocab_counts(counts)
    model.init_embeddings()

    if args.tokens:
        return bench_tokens(args, model, server, worker)

    rng = np.random.default_rng(2000 + rank)
    # training pairs follow the SUBSAMPLED word distribution (reference
    # word2vec 'sample' parameter drops frequent words before pairing —
    # the same subsampling Word2Vec.set_vocab_counts implements), drawn
    # via the alias table
    from adapm_amd.sampling import Unigram

    f = counts / counts.sum()
    keep = np.minimum(1.0, np.sqrt(1e-3 / f) + 1e-3 / f)
    pair_dist = Unigram(counts * keep, None, 1.0, seed=2000 + rank,
                        device=server.rt.device)
    total = args.warmup + args.steps
    batches = [(pair_dist.draw(args.pairs), pair_dist.draw(args.pairs))
               for _ in range(total)]

    is_cuda = server.rt.device.type == "cuda"
    use_fused = (not args.no_fused) and world == 1 and is_cuda
    step_fn = model.train_pairs_fused if use_fused else model.train_pairs
    for i in range(args.warmup):
        step_fn(*batches[i])
    model.drain()
    worker.barrier()
    if is_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.warmup, total):
        step_fn(*batches[i])
    model.drain()
    if is_cuda:
        torch.cuda.synchronize()
    el = time.perf_counter() - t0
    worker.barrier()
    if world > 1:
        el = worker.allreduce(el, op="max")

    pairs_per_s = args.pairs * args.steps * world / el
    keys_per_step = 2 * (2 + args.negative) * args.pairs
    if rank == 0:
        print(json.dumps({
            "metric": "sgns_pairs_per_s", "value": pairs_per_s, "unit": "pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1000 * el / args.steps, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "fp32",
            "data": "synthetic",
            "config": {"model": "word2vec_sgns_dim300", "vocab": args.vocab,
                       "dim": args.dim, "negative": args.negative,
                       "global_batch": args.pairs * world,
                       "pull_push_ops_per_s": keys_per_step * args.steps * world / el,
                       "parallelism": f"ps-async-dp{world}"},
        }), flush=True)
    worker.finalize()
    server.shutdown()


if __name__ == "__main__":
    main()
