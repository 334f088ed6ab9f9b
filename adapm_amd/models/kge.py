"""Knowledge-graph embeddings (ComplEx) on the adaptive parameter manager.

Rebuild of the reference app (reference apps/knowledge_graph_embeddings.cc):
  - value layout: [embedding(dim) | AdaGrad accumulators(dim)] per key
    (reference entity_vector_length = 2*dim, :1243-1254)
  - entity keys [0, E), relation keys [E, E+R)
  - negatives via PrepareSample/PullSample (reference train() 437-531)
  - intent look-ahead: announce the keys of future batches
    `lookahead` batches ahead with per-batch clocks (reference
    signal_intent_ahead, :1059-1123)
  - score/grad/AdaGrad: one fused device kernel per batch
    (kernels_hip.hip k_kge_step; reference :832-858, 415-435)
  - the reference's two-sided objective, opt-in: subject-side negatives
    and L2 on the positive's rows (neg_samples_subject, gamma_entity,
    gamma_relation; k_kge_step_sides, reference train() and :1106).
    Dropout is not built.
  - eval: MRR / Hits@k by scoring candidate sets (reference :544-712)
  - checkpoint: WaitSync -> Barrier -> rank-0 full pull -> save
    (reference :327-401)
"""
from __future__ import annotations

import dataclasses
import os
from typing import Optional

import numpy as np
import torch

# A/B switch: keep the host draw of the negatives on the fused world==1 path
_HOST_NEGATIVES = os.environ.get("ADAPM_HOST_NEGATIVES", "0") == "1"

import adapm_amd
from adapm_amd import _C

from ._step import StepModel
from .kge_eval import evaluate_ranks, format_ranks


@dataclasses.dataclass
class ComplExConfig:
    num_entities: int = 1_000_000
    num_relations: int = 1_000
    dim: int = 512            # embedding dim (complex dim = dim/2)
    neg_samples: int = 16     # o-side negatives per positive
    batch_size: int = 4096
    lr: float = 0.1
    eps: float = 1e-6
    lookahead: int = 4        # batches of intent signaled ahead
    init_scale: float = 0.1
    seed: int = 42
    # the sides step: any of these off its default selects it
    neg_samples_subject: int = 0  # s-side negatives per positive
    gamma_entity: float = 0.0     # L2 on the positive's s and o rows
    gamma_relation: float = 0.0   # L2 on the positive's r row

    @property
    def sides(self) -> bool:
        return bool(self.neg_samples_subject or self.gamma_entity or self.gamma_relation)

    @property
    def num_keys(self) -> int:
        return self.num_entities + self.num_relations

    @property
    def row(self) -> int:
        return 2 * self.dim


class ComplEx(StepModel):
    # ------------------------------------------------------------ init

    def init_embeddings(self):
        """Each rank initializes the keys it manages (key % world == rank)
        with set(); AdaGrad accumulators start at 0."""
        cfg = self.cfg
        self._init_owned(  # ~128MB of values per set
            cfg.num_keys, max(1, 2 ** 25 // cfg.row),
            lambda ks, vals: vals[:, :cfg.dim].normal_(0.0, cfg.init_scale))

    # ------------------------------------------------------------ train

    def keys_of(self, triples: np.ndarray):
        s = triples[:, 0].astype(np.int64)
        r = (self.cfg.num_entities + triples[:, 1]).astype(np.int64)
        o = triples[:, 2].astype(np.int64)
        return s, r, o

    def signal_intent(self, triples: np.ndarray, start: int, end: int = 0):
        s, r, o = self.keys_of(triples)
        self.worker.intent(np.concatenate([s, r, o]), start, end)

    def _draw_negatives(self, B):
        """One draw per step. The sides step splits it: the first
        B * neg_samples keys corrupt the object, the rest the subject."""
        cfg = self.cfg
        return self._negatives(B * (cfg.neg_samples + cfg.neg_samples_subject),
                               cfg.num_entities)

    def _neg_parts(self, neg_keys, B):
        """The negative key arrays of the classic step, role by role."""
        if not self.cfg.sides:
            return [neg_keys]
        n_o = B * self.cfg.neg_samples
        return [neg_keys[:n_o], neg_keys[n_o:]]

    def _sides_tail(self):
        cfg = self.cfg
        return (cfg.neg_samples, cfg.neg_samples_subject, cfg.dim, cfg.lr, cfg.eps,
                cfg.gamma_entity, cfg.gamma_relation)

    def _launch(self, v, d, loss):
        cfg = self.cfg
        if cfg.sides:  # v, d: s | r | o | neg_o | neg_s
            _C.kge_complex_step_sides(*v, *d, loss, *self._sides_tail())
            return
        _C.kge_complex_step(*v, *d, loss, cfg.neg_samples, cfg.dim, cfg.lr, cfg.eps)

    def train_batch(self, triples: np.ndarray, async_push: bool = True,
                    sync_loss: bool = True, neg_keys: np.ndarray = None):
        """One training step over B positive triples. Returns mean loss
        (float if sync_loss else a device tensor, no host sync)."""
        t0 = self._t0()
        if neg_keys is None:
            neg_keys = self._draw_negatives(len(triples))
        t0 = self._ph("sample", t0)
        handle = self._begin_step([*self.keys_of(triples),
                                   *self._neg_parts(neg_keys, len(triples))])
        return self._finish_step(handle, self._launch, sync_loss, t0,
                                 wait_push=not async_push)

    def _classic_step(self, arrays):
        if self.cfg.sides:
            triples, negs_o, negs_s = arrays
            return self.train_batch(triples, sync_loss=False, neg_keys=np.concatenate(
                [negs_o.reshape(-1), negs_s.reshape(-1)]))
        triples, negs2 = arrays
        return self.train_batch(triples, sync_loss=False, neg_keys=negs2.reshape(-1))

    def _fused_identity_step(self, arrays):
        raw = self.server.raw
        return self._fused_raw(
            raw.kge_step_sides_fused if self.cfg.sides else raw.kge_step_fused, arrays)

    def _fused_general_step(self, arrays):
        raw = self.server.raw
        return self._fused_raw(raw.kge_step_sides_fused_general if self.cfg.sides
                               else raw.kge_step_fused_general, arrays)

    def _fused_raw(self, step, arrays):
        cfg = self.cfg
        if cfg.sides:
            triples, negs_o, negs_s = arrays
            return step(*map(torch.from_numpy, self.keys_of(triples)),
                        torch.from_numpy(np.ascontiguousarray(negs_o.reshape(-1))),
                        torch.from_numpy(np.ascontiguousarray(negs_s.reshape(-1))),
                        *self._sides_tail())
        triples, negs2 = arrays
        return step(*map(torch.from_numpy, self.keys_of(triples)),
                    torch.from_numpy(np.ascontiguousarray(negs2.reshape(-1))),
                    cfg.neg_samples, cfg.dim, cfg.lr, cfg.eps)

    def train_batch_fused(self, triples: np.ndarray, sync_loss: bool = False,
                          force_general: bool = False):
        """Fused slab-direct step: kernels read rows straight from the
        HBM slab and accumulate the AdaGrad deltas back — no pull/push
        buffers. world==1 with the identity layout uses the zero-host-
        work path (Server.kge_step_fused); otherwise the general path
        (kge_step_fused_general) resolves slab offsets in a host pass,
        runs the fused kernel on the samples whose keys are all local
        (>95% after intent-driven relocation) and routes the rest
        through the classic pull/kernel/push path. force_general also
        enables the general path on the CPU store (the gloo test tier)."""
        cfg = self.cfg
        w = self.worker
        B = len(triples)
        smp = self.server.sampling
        if (smp is not None and not _HOST_NEGATIVES and self._fused_identity(force_general)
                and smp.device_stream() is not None):
            # negatives drawn on the device inside the step: the same keys
            # the host draw would give (ADAPM_HOST_NEGATIVES=1 keeps that
            # draw, for A/B runs)
            NN = B * (cfg.neg_samples + cfg.neg_samples_subject)
            sid = w.prepare_sample(NN, w.current_clock(), w.current_clock() + 2)
            us = smp.pull_device(w, sid, NN, draw=False)
            w.finish_sample(sid)
            if cfg.sides:
                loss, _neg = self.server.raw.kge_step_sides_fused_sampled(
                    *map(torch.from_numpy, self.keys_of(triples)), us, *self._sides_tail())
                return self._loss_out(loss, sync_loss)
            loss, _neg = self.server.raw.kge_step_fused_sampled(
                *map(torch.from_numpy, self.keys_of(triples)),
                us, cfg.neg_samples, cfg.dim, cfg.lr, cfg.eps)
            return self._loss_out(loss, sync_loss)
        negs2 = np.ascontiguousarray(self._draw_negatives(B), dtype=np.int64)
        if cfg.sides:
            n_o = B * cfg.neg_samples
            return self._fused_step((triples, negs2[:n_o].reshape(B, cfg.neg_samples),
                                     negs2[n_o:].reshape(B, cfg.neg_samples_subject)),
                                    sync_loss, force_general)
        return self._fused_step((triples, negs2.reshape(B, cfg.neg_samples)),
                                sync_loss, force_general)

    # ---------------------------------------------- prefetch pipeline

    def prefetch(self, triples: np.ndarray):
        """Start the pulls for a future batch (bounded async, like the
        reference's max_concurrent_loops pipelining): sample negatives,
        allocate buffers, issue one async pull. Returns a handle for
        train_prefetched."""
        return self._begin_step([*self.keys_of(triples), *self._neg_parts(
            self._draw_negatives(len(triples)), len(triples))])

    def train_prefetched(self, handle, sync_loss: bool = False):
        """Finish a prefetched batch: wait for the pull, run the step
        kernel, push the deltas."""
        return self._finish_step(handle, self._launch, sync_loss)

    # ------------------------------------------------------------ eval

    @torch.no_grad()
    def evaluate_full(self, triples: np.ndarray, hits_at=(1, 3, 10),
                      chunk: int = 65536, filter_triples: np.ndarray = None) -> dict:
        """Rank the true object among ALL entities, chunked (the reference
        evaluates against every entity, knowledge_graph_embeddings.cc:
        716-774 — there with OpenMP, here with the batched scoring
        kernel).

        filter_triples: known-true (s, r, o) triples (train+valid+test).
        When given, the FILTERED rank excludes other true objects of the
        same (s, r) from the competitors (reference computes filtered and
        raw ranks, knowledge_graph_embeddings.cc:544-712): `mrr`/`mr`/
        `hits@k` become the filtered metrics and `*_raw` carry the raw
        ones."""
        cfg = self.cfg
        w = self.worker
        B = len(triples)
        s_keys, r_keys, o_keys = self.keys_of(triples)
        opts = dict(dtype=torch.float32, device=self.dev)
        s_v = torch.empty(B, cfg.row, **opts)
        r_v = torch.empty(B, cfg.row, **opts)
        o_v = torch.empty(B, cfg.row, **opts)
        w.pull(s_keys, s_v)
        w.pull(r_keys, r_v)
        w.pull(o_keys, o_v)
        dc = cfg.dim // 2
        sr_re = s_v[:, :dc] * r_v[:, :dc] - s_v[:, dc:cfg.dim] * r_v[:, dc:cfg.dim]
        sr_im = s_v[:, dc:cfg.dim] * r_v[:, :dc] + s_v[:, :dc] * r_v[:, dc:cfg.dim]
        true_scores = (sr_re * o_v[:, :dc] + sr_im * o_v[:, dc:cfg.dim]).sum(1, keepdim=True)

        better = torch.zeros(B, dtype=torch.float32, device=self.dev)
        c_v = torch.empty(chunk, cfg.row, **opts)
        scores = torch.empty(B, chunk, **opts)
        for e0 in range(0, cfg.num_entities, chunk):
            n = min(chunk, cfg.num_entities - e0)
            cand = np.arange(e0, e0 + n, dtype=np.int64)
            cv = c_v[:n] if n == chunk else torch.empty(n, cfg.row, **opts)
            sv = scores[:, :n] if n == chunk else torch.empty(B, n, **opts)
            w.pull(cand, cv)
            _C.kge_complex_score(s_v, r_v, cv, sv, cfg.dim)
            better += (sv > true_scores).sum(1).float()
        rank_raw = 1 + better

        def metrics(rank, suffix=""):
            m = {f"mrr{suffix}": float((1.0 / rank).mean().item()),
                 f"mr{suffix}": float(rank.mean().item())}
            for h in hits_at:
                m[f"hits@{h}{suffix}"] = float((rank <= h).float().mean().item())
            return m

        if filter_triples is None:
            out = metrics(rank_raw)
        else:
            # filtered rank: other KNOWN-TRUE objects of the same (s, r)
            # do not count as competitors. Score only those few objects
            # and subtract the ones that out-ranked the true object.
            from collections import defaultdict

            true_objs = defaultdict(list)
            for fs, fr, fo in filter_triples:
                true_objs[(int(fs), int(fr))].append(int(fo))
            b_idx, obj_ids = [], []
            for b, (ts, tr, to) in enumerate(triples):
                for o2 in true_objs.get((int(ts), int(tr)), ()):
                    if o2 != int(to):
                        b_idx.append(b)
                        obj_ids.append(o2)
            filtered_better = torch.zeros_like(better)
            if b_idx:
                uniq, inv = np.unique(np.asarray(obj_ids, dtype=np.int64),
                                      return_inverse=True)
                u_v = torch.empty(len(uniq), cfg.row, **opts)
                w.pull(uniq, u_v)
                bi = torch.as_tensor(b_idx, dtype=torch.long, device=self.dev)
                ov2 = u_v[torch.as_tensor(inv, dtype=torch.long, device=self.dev)]
                sc = (sr_re[bi] * ov2[:, :dc] + sr_im[bi] * ov2[:, dc:cfg.dim]).sum(1)
                beats = (sc > true_scores[bi, 0]).float()
                filtered_better.scatter_add_(0, bi, beats)
            rank_filt = 1 + better - filtered_better
            out = metrics(rank_filt)
            out.update(metrics(rank_raw, "_raw"))
        out["n"] = float(B)
        if self.world > 1:
            vec = torch.tensor([out["n"]] + [out[k] * out["n"] for k in sorted(out) if k != "n"])
            vec = w.allreduce(vec)
            names = [k for k in sorted(out) if k != "n"]
            out = {k: float(vec[1 + i] / vec[0]) for i, k in enumerate(names)}
            out["n"] = float(vec[0])
        return out

    def _rank_layout(self):
        return self.cfg.dim, self.cfg.row, self.cfg.dim, self.cfg.row

    def _rank_query(self, side, s_v, r_v, o_v):
        """psi = sum (s_re r_re - s_im r_im) o_re + (s_im r_re + s_re r_im) o_im
        is linear in each of s, r, o: the query of a side holds the
        coefficients of that side's [re | im] halves."""
        dc = self.cfg.dim // 2
        a, b = {"o": (s_v, r_v), "s": (r_v, o_v), "r": (s_v, o_v)}[side]
        a_re, a_im, b_re, b_im = a[:, :dc], a[:, dc:2 * dc], b[:, :dc], b[:, dc:2 * dc]
        if side == "o":
            return torch.cat([a_re * b_re - a_im * b_im, a_im * b_re + a_re * b_im], dim=1)
        return torch.cat([a_re * b_re + a_im * b_im, a_re * b_im - a_im * b_re], dim=1)

    def evaluate_ranks(self, triples, filter_triples=None, sides="sro", hits_at=(1, 3, 10),
                       chunk: int = 65536, return_ranks: bool = False) -> dict:
        """Subject, relation and object ranks against ALL candidates, raw and
        (s, o sides) filtered: kge_eval.evaluate_ranks."""
        return evaluate_ranks(self, triples, filter_triples, sides, hits_at, chunk,
                              return_ranks)

    @torch.no_grad()
    def evaluate(self, triples: np.ndarray, num_candidates: int = 1000,
                 hits_at=(1, 3, 10)) -> dict:
        """Rank the true object among `num_candidates` random candidates
        (+ the true one). Aggregated over ranks via allreduce (reference
        eval: knowledge_graph_embeddings.cc:544-712)."""
        cfg = self.cfg
        w = self.worker
        B = len(triples)
        s_keys, r_keys, o_keys = self.keys_of(triples)
        cand = self.rng.integers(0, cfg.num_entities, size=num_candidates, dtype=np.int64)

        opts = dict(dtype=torch.float32, device=self.dev)
        s_v = torch.empty(B, cfg.row, **opts)
        r_v = torch.empty(B, cfg.row, **opts)
        o_v = torch.empty(B, cfg.row, **opts)
        c_v = torch.empty(num_candidates, cfg.row, **opts)
        w.pull(s_keys, s_v)
        w.pull(r_keys, r_v)
        w.pull(o_keys, o_v)
        w.pull(cand, c_v)

        cand_scores = torch.empty(B, num_candidates, **opts)
        _C.kge_complex_score(s_v, r_v, c_v, cand_scores, cfg.dim)
        true_scores = torch.empty(B, 1, **opts)
        # score the true o: reuse the kernel with E=1 per row via batched diag
        # (cheap path: einsum on device)
        dc = cfg.dim // 2
        sr_re = s_v[:, :dc] * r_v[:, :dc] - s_v[:, dc:cfg.dim] * r_v[:, dc:cfg.dim]
        sr_im = s_v[:, dc:cfg.dim] * r_v[:, :dc] + s_v[:, :dc] * r_v[:, dc:cfg.dim]
        true_scores[:, 0] = (sr_re * o_v[:, :dc] + sr_im * o_v[:, dc:cfg.dim]).sum(1)

        rank = 1 + (cand_scores > true_scores).sum(1).float()
        out = {
            "mrr": float((1.0 / rank).mean().item()),
            "mr": float(rank.mean().item()),
            "n": float(B),
        }
        for h in hits_at:
            out[f"hits@{h}"] = float((rank <= h).float().mean().item())
        # aggregate across ranks (weighted by n)
        if self.world > 1:
            vec = torch.tensor([out["n"]] + [out[k] * out["n"] for k in sorted(out) if k != "n"])
            vec = w.allreduce(vec)
            names = [k for k in sorted(out) if k != "n"]
            out = {k: float(vec[1 + i] / vec[0]) for i, k in enumerate(names)}
            out["n"] = float(vec[0])
        return out

    # ------------------------------------------------------------ checkpoint

    def save_checkpoint(self, path: str, chunk_keys: int = 65536):
        """rank 0 pulls the full model (incl. AdaGrad state) and writes an
        .npz (reference pull_full_model + write_checkpoint, :209-231,327-401)."""
        self.drain()
        self.worker.wait_sync()
        self.worker.barrier()
        if self.rank == 0:
            cfg = self.cfg
            out = np.empty((cfg.num_keys, cfg.row), dtype=np.float32)
            for i in range(0, cfg.num_keys, chunk_keys):
                ks = np.arange(i, min(i + chunk_keys, cfg.num_keys), dtype=np.int64)
                buf = np.zeros((len(ks), cfg.row), dtype=np.float32)
                self.worker.pull(ks, buf)
                out[i:i + len(ks)] = buf
            np.savez(path, values=out,
                     num_entities=cfg.num_entities, num_relations=cfg.num_relations,
                     dim=cfg.dim)
        self.worker.barrier()

    def load_checkpoint(self, path: str, chunk_keys: int = 65536):
        """rank 0 reads and set()s the full model."""
        if self.rank == 0:
            data = np.load(path)
            vals = data["values"]
            for i in range(0, len(vals), chunk_keys):
                ks = np.arange(i, min(i + chunk_keys, len(vals)), dtype=np.int64)
                self.worker.set(ks, np.ascontiguousarray(vals[i:i + len(ks)]))
        self.worker.wait_sync()
        self.worker.barrier()


def make_synthetic_triples(n: int, num_entities: int, num_relations: int,
                           seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.stack([
        rng.integers(0, num_entities, size=n),
        rng.integers(0, num_relations, size=n),
        rng.integers(0, num_entities, size=n),
    ], axis=1).astype(np.int64)


def main():
    """CLI (rebuild of the reference app binary,
    apps/knowledge_graph_embeddings.cc CLI): train ComplEx on a synthetic
    graph, report loss + eval, optionally checkpoint."""
    import argparse
    import time

    import adapm_amd as _a

    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=100_000)
    ap.add_argument("--relations", type=int, default=100)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--neg", type=int, default=8)
    ap.add_argument("--neg-samples-subject", type=int, default=0,
                    help="subject-side negatives per positive (reference: as many as --neg)")
    ap.add_argument("--gamma-entity", type=float, default=0.0,
                    help="L2 on the positive's entity rows (reference: 1e-3)")
    ap.add_argument("--gamma-relation", type=float, default=0.0,
                    help="L2 on the positive's relation row (reference: 1e-3)")
    ap.add_argument("--triples", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--lr", type=float, default=0.1)
    ap.add_argument("--eval-every", type=int, default=1)
    ap.add_argument("--eval-triples", type=int, default=1024)
    ap.add_argument("--eval-full", action="store_true",
                    help="rank against ALL entities (reference eval)")
    ap.add_argument("--eval-ranks", action="store_true",
                    help="subject / relation / object ranks against ALL candidates, "
                         "filtered and raw, printed as the reference's table")
    ap.add_argument("--checkpoint", type=str, default="")
    ap.add_argument("--device", type=str, default=None)
    a = ap.parse_args()

    _a.setup(num_keys=a.entities + a.relations, num_threads=1, device=a.device)
    server = _a.Server(2 * a.dim)
    server.enable_sampling_support("local", True, "uniform", 0, a.entities)
    worker = _a.Worker(0, server)
    cfg = ComplExConfig(num_entities=a.entities, num_relations=a.relations, dim=a.dim,
                        neg_samples=a.neg, batch_size=a.batch, lr=a.lr,
                        neg_samples_subject=a.neg_samples_subject,
                        gamma_entity=a.gamma_entity, gamma_relation=a.gamma_relation)
    model = ComplEx(cfg, server, worker)
    model.init_embeddings()
    rank = server.my_rank()
    world = server.rt.world
    triples = make_synthetic_triples(a.triples // world, a.entities, a.relations,
                                     seed=100 + rank)
    for ep in range(a.epochs):
        t0 = time.time()
        losses = []
        for i in range(0, len(triples), a.batch):
            b = triples[i:i + a.batch]
            model.signal_intent(b, worker.current_clock() + 1, worker.current_clock() + 3)
            losses.append(model.train_batch(b, sync_loss=True))
            worker.advance_clock()
        model.drain()
        total = worker.allreduce(float(np.mean(losses)))
        if rank == 0:
            print(f"[kge] epoch {ep}: loss {total / world:.4f} ({time.time()-t0:.1f}s)")
        if a.eval_every and (ep + 1) % a.eval_every == 0 and a.eval_ranks:
            ev = model.evaluate_ranks(triples[:a.eval_triples], filter_triples=triples)
            if rank == 0:
                print(format_ranks(ev, prefix="[kge] eval"))
        elif a.eval_every and (ep + 1) % a.eval_every == 0:
            ev = (model.evaluate_full(triples[:a.eval_triples], filter_triples=triples)
                  if a.eval_full else model.evaluate(triples[:a.eval_triples]))
            if rank == 0:
                print(f"[kge] eval: {ev}")
    if a.checkpoint:
        model.save_checkpoint(a.checkpoint)
        if rank == 0:
            print(f"[kge] checkpoint -> {a.checkpoint}")
    worker.finalize()
    server.shutdown()


if __name__ == "__main__":
    main()


class Rescal(StepModel):
    """RESCAL scorer (reference knowledge_graph_embeddings.cc:895-922):
    psi = e_s^T R e_o with a D x D matrix per relation. Exercises the
    store's NON-UNIFORM value lengths: entity rows 2*D floats, relation
    rows 2*D*D floats, so it pulls and pushes role by role instead of
    taking the skeleton's one-buffer classic step. The two-sided
    objective of ComplExConfig (neg_samples_subject, gamma_entity,
    gamma_relation) selects rescal_step_sides / rescal_step_sides_grouped."""

    @staticmethod
    def value_lengths(num_entities, num_relations, dim):
        lens = np.full(num_entities + num_relations, 2 * dim, dtype=np.int64)
        lens[num_entities:] = 2 * dim * dim
        return lens

    def init_embeddings(self):
        cfg = self.cfg
        my_keys = np.arange(self.rank, cfg.num_keys, self.world, dtype=np.int64)
        ents = my_keys[my_keys < cfg.num_entities]
        rels = my_keys[my_keys >= cfg.num_entities]
        chunk = max(1, 2 ** 24 // (2 * cfg.dim))
        for i in range(0, len(ents), chunk):
            ks = ents[i:i + chunk]
            v = torch.zeros(len(ks), 2 * cfg.dim, dtype=torch.float32, device=self.dev)
            v[:, :cfg.dim].normal_(0, cfg.init_scale)
            self.worker.set(ks, v)
        rchunk = max(1, 2 ** 24 // (2 * cfg.dim * cfg.dim))
        for i in range(0, len(rels), rchunk):
            ks = rels[i:i + rchunk]
            v = torch.zeros(len(ks), 2 * cfg.dim * cfg.dim, dtype=torch.float32,
                            device=self.dev)
            v[:, :cfg.dim * cfg.dim].normal_(0, cfg.init_scale / cfg.dim ** 0.5)
            self.worker.set(ks, v)
        self.worker.wait_sync()
        self.worker.barrier()

    def _rank_layout(self):
        D = self.cfg.dim
        return D, 2 * D, D * D, 2 * D * D

    def _rank_query(self, side, s_v, r_v, o_v):
        """psi = s^T R o with R row-major: the object is scored by R^T s,
        the subject by R o, the relation by outer(s, o) flattened."""
        D = self.cfg.dim
        s, o = s_v[:, :D], o_v[:, :D]
        if side == "r":
            return (s.unsqueeze(2) * o.unsqueeze(1)).reshape(-1, D * D)
        Rm = r_v[:, :D * D].reshape(-1, D, D)
        if side == "o":
            return torch.bmm(s.unsqueeze(1), Rm).squeeze(1)
        return torch.bmm(Rm, o.unsqueeze(2)).squeeze(2)

    def evaluate_ranks(self, triples, filter_triples=None, sides="sro", hits_at=(1, 3, 10),
                       chunk: int = 65536, return_ranks: bool = False) -> dict:
        """Subject, relation and object ranks against ALL candidates, raw and
        (s, o sides) filtered: kge_eval.evaluate_ranks."""
        return evaluate_ranks(self, triples, filter_triples, sides, hits_at, chunk,
                              return_ranks)

    def train_batch(self, triples: np.ndarray, sync_loss: bool = True,
                    grouped: bool = None, neg_keys: np.ndarray = None):
        """One RESCAL step. grouped=True (default on GPU): sort the batch
        by relation, pull each distinct relation matrix ONCE and run the
        three dim^2 products as MFMA-tiled grouped GEMMs
        (rescal_step_grouped) — the reference's per-triple scalar loops
        (knowledge_graph_embeddings.cc:895-922) are GEMM-shaped once
        triples share R. Also cuts the pull/push volume for R from
        B x 2D^2 to G x 2D^2. AdaGrad on dR uses the group-summed
        gradient (minibatch semantics); the classic path transforms each
        triple's outer product separately (both from the same pulled
        accumulator snapshot).

        With cfg.sides (neg_samples_subject, gamma_entity or
        gamma_relation off its default) the step is the two-sided one,
        _train_batch_sides. neg_keys names the negatives, sample by
        sample in the order of `triples` as given."""
        cfg = self.cfg
        w = self.worker
        B = len(triples)
        D = cfg.dim
        if grouped is None:
            grouped = self.dev.type == "cuda" and D % 4 == 0
        order = None
        if grouped:
            order = np.argsort(triples[:, 1], kind="stable")
            triples = triples[order]
        s_keys = triples[:, 0].astype(np.int64)
        r_keys = (cfg.num_entities + triples[:, 1]).astype(np.int64)
        o_keys = triples[:, 2].astype(np.int64)
        if cfg.sides:
            return self._train_batch_sides(s_keys, r_keys, o_keys, order, neg_keys, sync_loss)
        if neg_keys is None:
            neg_keys = self._negatives(B * cfg.neg_samples, cfg.num_entities)
        else:
            neg_keys = self._by_sample(neg_keys, B, cfg.neg_samples, order)
        opts = dict(dtype=torch.float32, device=self.dev)
        s_v = torch.empty(B, 2 * D, **opts)
        o_v = torch.empty(B, 2 * D, **opts)
        n_v = torch.empty(B * cfg.neg_samples, 2 * D, **opts)

        if grouped:
            uniq_r, starts_np = np.unique(r_keys, return_index=True)
            starts = np.append(starts_np, B).astype(np.int32)
            r_v = torch.empty(len(uniq_r), 2 * D * D, **opts)
            for kt, vt in ((s_keys, s_v), (uniq_r, r_v), (o_keys, o_v), (neg_keys, n_v)):
                w.wait(w.pull(kt, vt, async_=True))
            ds, do, dn = (torch.empty_like(t) for t in (s_v, o_v, n_v))
            drl = torch.empty_like(r_v)
            loss = _C.rescal_step_grouped(s_v, r_v, o_v, n_v, ds, drl, do, dn,
                                          torch.from_numpy(starts), cfg.neg_samples, D,
                                          cfg.lr, cfg.eps)
            push_sets = ((s_keys, ds), (uniq_r, drl), (o_keys, do), (neg_keys, dn))
        else:
            r_v = torch.empty(B, 2 * D * D, **opts)
            for kt, vt in ((s_keys, s_v), (r_keys, r_v), (o_keys, o_v), (neg_keys, n_v)):
                w.wait(w.pull(kt, vt, async_=True))
            ds, drl, do, dn = (torch.empty_like(t) for t in (s_v, r_v, o_v, n_v))
            loss = torch.empty(B, dtype=torch.float32, device=self.dev)
            _C.rescal_step(s_v, r_v, o_v, n_v, ds, drl, do, dn, loss,
                           cfg.neg_samples, D, cfg.lr, cfg.eps)
            push_sets = ((s_keys, ds), (r_keys, drl), (o_keys, do), (neg_keys, dn))
        for kt, dt in push_sets:
            self._track(w.push(kt, dt, async_=True))
        return self._loss_out(loss, sync_loss)

    @staticmethod
    def _by_sample(keys, B, n, order):
        """[B*n] keys named sample by sample, in the order the step runs
        its samples (`order`: the grouped step's sort, else None)."""
        keys = np.ascontiguousarray(keys, dtype=np.int64).reshape(B, n)
        return keys.reshape(-1) if order is None else keys[order].reshape(-1)

    def _train_batch_sides(self, s_keys, r_keys, o_keys, order, neg_keys, sync_loss):
        """The two-sided step (reference train(), knowledge_graph_embeddings.cc:
        437-531, which RESCAL shares with ComplEx): one draw of
        B * (neg_samples + neg_samples_subject) keys, the first
        B * neg_samples corrupt the object and the rest the subject; a fifth
        pull and push for the subject-side negatives; gamma * E on the
        positive's rows inside the kernels (rescal_step_sides, and
        rescal_step_sides_grouped when `order` is the grouped sort)."""
        cfg = self.cfg
        w = self.worker
        B, D, N, NS = len(s_keys), cfg.dim, cfg.neg_samples, cfg.neg_samples_subject
        if neg_keys is None:
            neg_keys = self._negatives(B * (N + NS), cfg.num_entities)
            no_keys, ns_keys = neg_keys[:B * N], neg_keys[B * N:]
        else:
            neg_keys = np.asarray(neg_keys, dtype=np.int64)
            no_keys = self._by_sample(neg_keys[:B * N], B, N, order)
            ns_keys = self._by_sample(neg_keys[B * N:], B, NS, order)
        opts = dict(dtype=torch.float32, device=self.dev)
        s_v = torch.empty(B, 2 * D, **opts)
        o_v = torch.empty(B, 2 * D, **opts)
        no_v = torch.empty(B * N, 2 * D, **opts)
        ns_v = torch.empty(B * NS, 2 * D, **opts)
        tail = (N, NS, D, cfg.lr, cfg.eps, cfg.gamma_entity, cfg.gamma_relation)
        if order is not None:
            rk, starts_np = np.unique(r_keys, return_index=True)
            starts = np.append(starts_np, B).astype(np.int32)
        else:
            rk = r_keys
        r_v = torch.empty(len(rk), 2 * D * D, **opts)
        pulls = ((s_keys, s_v), (rk, r_v), (o_keys, o_v), (no_keys, no_v), (ns_keys, ns_v))
        for kt, vt in pulls:
            if len(kt):  # a side without negatives has nothing to pull or push
                w.wait(w.pull(kt, vt, async_=True))
        deltas = [torch.empty_like(vt) for _, vt in pulls]
        if order is not None:
            loss = _C.rescal_step_sides_grouped(s_v, r_v, o_v, no_v, ns_v, *deltas,
                                                torch.from_numpy(starts), *tail)
        else:
            loss = torch.empty(B, dtype=torch.float32, device=self.dev)
            _C.rescal_step_sides(s_v, r_v, o_v, no_v, ns_v, *deltas, loss, *tail)
        for (kt, _), dt in zip(pulls, deltas):
            if len(kt):
                self._track(w.push(kt, dt, async_=True))
        return self._loss_out(loss, sync_loss)
