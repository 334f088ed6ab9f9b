#!/usr/bin/env python3
"""Cost of the ComplEx sides step next to the one-sided fused step, on the
flagship setup (world 1, dim 512, batch 16384, 10M entities, negatives drawn
on the device). One process measures one step:

  --step sides   N object-side + NS subject-side negatives, gammas 1e-3
  --step one     the existing step with N + NS object-side negatives

Both touch 3 + N + NS rows per positive. Run them ABBA in one session on one
box and compare by slot parity (docs/NOTES_NEXT_ROUND.md). Prints one JSON
line; metric = ms per step."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["sides", "one"], default="sides")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--warmup-budget-s", type=float, default=4.0)
    ap.add_argument("--entities", type=int, default=10_000_000)
    ap.add_argument("--relations", type=int, default=1_000)
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--neg", type=int, default=8, help="object-side negatives of the sides step")
    ap.add_argument("--neg-subject", type=int, default=8)
    ap.add_argument("--gamma", type=float, default=1e-3)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--device", type=str, default=None)
    args = ap.parse_args()

    import adapm_amd
    from adapm_amd.models.kge import ComplEx, ComplExConfig

    adapm_amd.setup(num_keys=args.entities + args.relations, num_threads=1, device=args.device,
                    capacity_factor=3.0, max_sync_per_sec=2000.0)
    server = adapm_amd.Server(2 * args.dim)
    server.enable_sampling_support("local", True, "uniform", 0, args.entities)
    worker = adapm_amd.Worker(0, server)
    if args.step == "sides":
        cfg = ComplExConfig(num_entities=args.entities, num_relations=args.relations,
                            dim=args.dim, neg_samples=args.neg, batch_size=args.batch, seed=7,
                            neg_samples_subject=args.neg_subject, gamma_entity=args.gamma,
                            gamma_relation=args.gamma)
    else:
        cfg = ComplExConfig(num_entities=args.entities, num_relations=args.relations,
                            dim=args.dim, neg_samples=args.neg + args.neg_subject,
                            batch_size=args.batch, seed=7)
    model = ComplEx(cfg, server, worker)
    torch.manual_seed(cfg.seed)
    model.init_embeddings()
    is_cuda = server.rt.device.type == "cuda"

    rng = np.random.default_rng(1000)

    def batch():
        return np.stack([rng.integers(0, args.entities, size=args.batch),
                         rng.integers(0, args.relations, size=args.batch),
                         rng.integers(0, args.entities, size=args.batch)], axis=1).astype(np.int64)

    total = args.warmup + args.steps
    batches = [batch() for _ in range(total)]

    def step(b):
        out = model.train_batch_fused(b)
        worker.advance_clock()
        return out

    def sync():
        model.drain()
        if is_cuda:
            torch.cuda.synchronize()

    for i in range(args.warmup):
        out = step(batches[i])
    sync()
    t_w, extra = time.perf_counter(), 0
    while time.perf_counter() - t_w < args.warmup_budget_s:  # clocks ramp for ~2 s
        out = step(batches[extra % args.warmup])
        sync()
        extra += 1
    float(out.mean().item())  # load the reduction kernel before the clock starts

    t0 = time.perf_counter()
    for i in range(args.warmup, total):
        out = step(batches[i])
    last_loss = float(out.mean().item())
    sync()
    el = time.perf_counter() - t0

    rows = 3 + args.neg + args.neg_subject
    print(json.dumps({
        "metric": "kge_step_ms", "value": 1000 * el / args.steps, "unit": "ms/step",
        "higher_is_better": False, "step": args.step, "steps": args.steps,
        "warmup": args.warmup, "warmup_extra_steps": extra, "last_loss": last_loss,
        "config": {"dim": args.dim, "batch": args.batch, "entities": args.entities,
                   "neg_object": cfg.neg_samples, "neg_subject": cfg.neg_samples_subject,
                   "gamma": args.gamma if args.step == "sides" else 0.0,
                   "rows_per_positive": rows,
                   "pull_push_ops_per_s": 2 * rows * args.batch * args.steps / el},
    }), flush=True)
    worker.finalize()
    server.shutdown()


if __name__ == "__main__":
    main()
