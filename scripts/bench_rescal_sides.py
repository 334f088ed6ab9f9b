#!/usr/bin/env python3
"""RESCAL two-sided step against the one-sided step at equal entity rows:
--objective sides runs _C.rescal_step_sides and _C.rescal_step_sides_grouped
at N = NS = 4 with gamma_e = gamma_r = 1e-3, --objective one runs
_C.rescal_step and _C.rescal_step_grouped at N = 8. Either way a positive
brings nine entity rows besides its subject; the two-sided step adds three
dim^2 products (v = R o, R^T z, z o^T) and a second pass.

One objective per process, so that an A/B is a sequence of runs (S O O S):

    python scripts/bench_rescal_sides.py --objective sides
    python scripts/bench_rescal_sides.py --objective one

Prints one line per path and a JSON line with the ms/step of both.
"""
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
    ap.add_argument("--objective", choices=["sides", "one"], required=True)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--relations", type=int, default=32)
    ap.add_argument("--rows", type=int, default=8,
                    help="negative entity rows per positive: N = NS = rows / 2, or N = rows")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from adapm_amd import _C

    sides = args.objective == "sides"
    B, D, G = args.batch, args.dim, args.relations
    N, NS = (args.rows // 2, args.rows - args.rows // 2) if sides else (args.rows, 0)
    gamma = 1e-3 if sides else 0.0
    assert torch.cuda.is_available()
    gen = torch.Generator().manual_seed(0)
    rels = np.sort(np.random.default_rng(0).integers(0, G, size=B))
    uniq, first = np.unique(rels, return_index=True)
    starts_t = torch.from_numpy(np.append(first, B).astype(np.int32))
    Gu = len(uniq)

    def rows(n, L, scale=1.0):
        return torch.randn(n, 2 * L, generator=gen).abs_().mul_(scale).cuda()

    s, o, neg_o, neg_s = rows(B, D), rows(B, D), rows(B * N, D), rows(B * NS, D)
    rm_u = rows(Gu, D * D, 0.05)
    # the per-triple path pulls one R copy per triple
    rm_b = rm_u.index_select(0, torch.from_numpy(np.searchsorted(uniq, rels)).cuda()).contiguous()
    ds, do, dno, dns = (torch.empty_like(t) for t in (s, o, neg_o, neg_s))
    drl_b, drl_u = torch.empty_like(rm_b), torch.empty_like(rm_u)
    loss = torch.empty(B, device="cuda")
    tail = (D, 0.1, 1e-8)

    if sides:
        def run_classic():
            _C.rescal_step_sides(s, rm_b, o, neg_o, neg_s, ds, drl_b, do, dno, dns, loss, N, NS,
                                 *tail, gamma, gamma)

        def run_grouped():
            _C.rescal_step_sides_grouped(s, rm_u, o, neg_o, neg_s, ds, drl_u, do, dno, dns,
                                         starts_t, N, NS, *tail, gamma, gamma)
    else:
        def run_classic():
            _C.rescal_step(s, rm_b, o, neg_o, ds, drl_b, do, dno, loss, N, *tail)

        def run_grouped():
            _C.rescal_step_grouped(s, rm_u, o, neg_o, ds, drl_u, do, dno, starts_t, N, *tail)

    out = {"objective": args.objective, "B": B, "D": D, "G": Gu, "N": N, "NS": NS}
    for name, fn in (("classic", run_classic), ("grouped", run_grouped)):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.iters
        out[f"{name}_ms"] = round(dt * 1e3, 4)
        print(f"{args.objective} {name}: {dt*1e3:.3f} ms/step  "
              f"({B / dt:.0f} triples/s, D={D}, G={Gu}, N={N}, NS={NS})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
