#!/usr/bin/env python3
"""RESCAL whole-step A/B on a real world-1 GPU store: Rescal.train_batch
(grouped: four pulls, six launches, four pushes) against
Rescal.train_batch_fused (host offset pass, four slab-direct launches).
Unlike scripts/bench_rescal.py, which times the kernels on resident
buffers, a step here includes everything a training loop pays for, and the
clock stops only after drain() and a device synchronise.

Both paths run the same batches with the same pre-drawn negatives, in the
order F C C F, twice, in one process; every run and the medians are printed,
then one JSON line.

--neg-samples-subject, --gamma-entity or --gamma-relation off their defaults
select the two-sided objective: the F runs are the two-sided fused step
(train_batch_fused(fuse_sides=True)), the C runs the two-sided classic step
(ten launches around five pulls and five pushes).

--dropout-entity or --dropout-relation off their defaults select the drop step
on both paths (rescal_drop_hip.hip: two launches, fused or between five pulls
and five pushes); compare two invocations to see what dropout costs.

Run on a GPU box:  python scripts/bench_rescal_fused.py [--dim 128] [--batch 2048]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--relations", type=int, default=32)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--neg", type=int, default=8)
    ap.add_argument("--neg-samples-subject", type=int, default=0)
    ap.add_argument("--gamma-entity", type=float, default=0.0)
    ap.add_argument("--gamma-relation", type=float, default=0.0)
    ap.add_argument("--dropout-entity", type=float, default=0.0)
    ap.add_argument("--dropout-relation", type=float, default=0.0)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--order", type=str, default="FCCFFCCF",
                    help="the runs, F fused and C classic; a profile wants one path, e.g. F")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU store"

    import adapm_amd
    from adapm_amd.models.kge import ComplExConfig, Rescal

    E, R, D, B, N = args.entities, args.relations, args.dim, args.batch, args.neg
    NS = args.neg_samples_subject
    cfg = ComplExConfig(num_entities=E, num_relations=R, dim=D, neg_samples=N, batch_size=B,
                        neg_samples_subject=NS, gamma_entity=args.gamma_entity,
                        gamma_relation=args.gamma_relation, dropout_entity=args.dropout_entity,
                        dropout_relation=args.dropout_relation)
    adapm_amd.setup(num_keys=E + R, num_threads=1, device="cuda:0")
    server = adapm_amd.Server(torch.from_numpy(Rescal.value_lengths(E, R, D)))
    worker = adapm_amd.Worker(0, server)
    model = Rescal(cfg, server, worker)
    model.init_embeddings()

    rng = np.random.default_rng(0)
    total = args.warmup + args.steps
    batches = [(np.stack([rng.integers(0, E, B), rng.integers(0, R, B), rng.integers(0, E, B)],
                         axis=1).astype(np.int64),
                rng.integers(0, E, B * (N + NS), dtype=np.int64)) for _ in range(total)]

    def classic(t, neg):
        model.train_batch(t, sync_loss=False, grouped=True, neg_keys=neg)

    def fused(t, neg):
        model.train_batch_fused(t, sync_loss=False, neg_keys=neg, fuse_sides=True)

    def run(step):
        for t, neg in batches[:args.warmup]:
            step(t, neg)
        model.drain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t, neg in batches[args.warmup:]:
            step(t, neg)
        model.drain()
        torch.cuda.synchronize()
        return 1000 * (time.perf_counter() - t0) / args.steps

    ms = {"fused": [], "classic": []}
    for name in ("fused" if c == "F" else "classic" for c in args.order.upper()):
        ms[name].append(run(fused if name == "fused" else classic))
        print(f"{name}: {ms[name][-1]:.3f} ms/step", flush=True)
    med = {k: statistics.median(v) if v else float("nan") for k, v in ms.items()}
    print(f"median: classic {med['classic']:.3f} ms, fused {med['fused']:.3f} ms, "
          f"classic / fused = {med['classic'] / med['fused']:.2f}x "
          f"(E={E}, R={R}, D={D}, B={B}, N={N}, NS={NS}, gamma_e={args.gamma_entity:g}, "
          f"gamma_r={args.gamma_relation:g}, p_e={args.dropout_entity:g}, "
          f"p_r={args.dropout_relation:g})")
    print(json.dumps({"metric": "rescal_step_ms", "classic_ms": ms["classic"],
                      "fused_ms": ms["fused"], "classic_median_ms": med["classic"],
                      "fused_median_ms": med["fused"],
                      "ratio": med["classic"] / med["fused"],
                      "config": {"entities": E, "relations": R, "dim": D, "batch": B, "neg": N,
                                 "neg_subject": NS, "gamma_entity": args.gamma_entity,
                                 "gamma_relation": args.gamma_relation,
                                 "dropout_entity": args.dropout_entity,
                                 "dropout_relation": args.dropout_relation,
                                 "steps": args.steps, "warmup": args.warmup}}), flush=True)
    worker.finalize()
    server.shutdown()


if __name__ == "__main__":
    main()
