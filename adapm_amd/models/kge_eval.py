"""Three-sided KGE evaluation, counted on the device.

Every test triple (s, r, o) is ranked three ways (reference
Evaluator::rank / Evaluator::evaluate, knowledge_graph_embeddings.cc:
544-774): the true subject among all entities, the true relation among
all relations, the true object among all entities. Raw ranks on all
three sides; on the subject and object sides also filtered ranks, which
do not count the other known-true subjects of (r, o) / objects of (s, r).

Each side is one query vector per triple, dotted with the first K floats
of every candidate row, so one kernel pair serves every scorer and side:

  _C.pair_scores  the score of a (query, candidate) pair: the true
                  triple's own score `base`, and the scores of the few
                  known-true competitors of the filter
  _C.rank_count   counts[b] += #{candidates scoring strictly above
                  base[b], or NaN}, with no score matrix in between

pair_scores returns the bits rank_count compares, so the true candidate
never counts against itself and a filtered competitor is subtracted
exactly when it was counted.

A model takes part through two hooks:

  _rank_layout()                -> (K_ent, row_ent, K_rel, row_rel)
      floats scored / floats stored per entity row and per relation row
  _rank_query(side, s_v, r_v, o_v) -> [B, K] query tensor
      for side in "s", "r", "o" from the pulled true rows

Candidates come through Worker.pull in chunks of `chunk` keys (entities
are keys 0..E-1, relations E..E+R-1), so this works at any world size
and with non-uniform value lengths.
"""
from __future__ import annotations

import numpy as np
import torch

from adapm_amd import _C

KINDS = ("s", "r", "o", "s_raw", "o_raw")


def _competitors(grp, answer, f_grp, f_answer):
    """Known answers of the filter that compete with each evaluated triple:
    for triple i every f_answer[j] with f_grp[j] == grp[i] (rows compared)
    and f_answer[j] != answer[i]. Returns (owner, ids): ids[p] competes
    with triple owner[p]. Sorting and searching, no loop over triples."""
    B = len(grp)
    _, inv = np.unique(np.concatenate([grp, f_grp]), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ge, gf = inv[:B], inv[B:]
    order = np.argsort(gf, kind="stable")
    gfs = gf[order]
    lo = np.searchsorted(gfs, ge, side="left")
    n = np.searchsorted(gfs, ge, side="right") - lo
    owner = np.repeat(np.arange(B, dtype=np.int64), n)
    first = np.cumsum(n) - n
    pos = np.arange(len(owner), dtype=np.int64) - np.repeat(first, n) + np.repeat(lo, n)
    ids = f_answer[order][pos]
    keep = ids != answer[owner]
    return owner[keep], ids[keep]


def _stream_counts(model, q, base, K, row, key0, n_cand, chunk):
    """#candidates of keys [key0, key0 + n_cand) above base, per query."""
    w = model.worker
    B = q.shape[0]
    counts = torch.zeros(B, dtype=torch.int32, device=model.dev)
    buf = torch.empty(min(chunk, n_cand), row, dtype=torch.float32, device=model.dev)
    for c0 in range(0, n_cand, chunk):
        n = min(chunk, n_cand - c0)
        cv = buf[:n]
        w.pull(np.arange(key0 + c0, key0 + c0 + n, dtype=np.int64), cv)
        _C.rank_count(q, cv, base, counts, K)
    return counts.cpu().numpy().astype(np.float64)


def _filtered_away(model, q, base_h, K, row, owner, ids, chunk):
    """Per triple, the competitors (owner, ids) scoring strictly above its
    base. A NaN competitor does not count here (reference :763-771)."""
    w = model.worker
    out = np.zeros(len(base_h), dtype=np.float64)
    for p0 in range(0, len(ids), chunk):
        own, idc = owner[p0:p0 + chunk], ids[p0:p0 + chunk]
        uniq, inv = np.unique(idc, return_inverse=True)
        u_v = torch.empty(len(uniq), row, dtype=torch.float32, device=model.dev)
        w.pull(uniq, u_v)
        cv = u_v[torch.from_numpy(inv.reshape(-1)).to(model.dev)]
        sc = torch.empty(len(idc), dtype=torch.float32, device=model.dev)
        _C.pair_scores(q, cv, torch.from_numpy(own.astype(np.int32)), sc, K)
        beats = sc.cpu().numpy() > base_h[own]
        out += np.bincount(own[beats], minlength=len(base_h))
    return out


@torch.no_grad()
def evaluate_ranks(model, triples, filter_triples=None, sides="sro", hits_at=(1, 3, 10),
                   chunk=65536, return_ranks=False) -> dict:
    """Rank the true subject, relation and object of every triple among all
    entities / relations / entities (`sides` picks a subset of "sro").

    Returns mrr_X / mr_X / hits@k_X for the computed sides X, mrr_X_raw /
    mr_X_raw for X in s, o, `mrr` and `mr` (the mean of the s and o sides,
    when both are computed) and `n`. With filter_triples (known-true
    triples, e.g. train + valid + test) the unsuffixed s and o metrics are
    the filtered ones; without, they equal the raw ones. The relation side
    is never filtered. A triple whose own score is NaN on a computed side
    gets NaN ranks on every side, as in the reference. Over several ranks
    the metrics are aggregated weighted by n. return_ranks=True adds
    `ranks`: per rank kind the float64 ranks of this process's triples."""
    if not sides or set(sides) - set("sro"):
        raise ValueError(f"sides must be a non-empty subset of 'sro', got {sides!r}")
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    cfg, w, dev = model.cfg, model.worker, model.dev
    E, R = cfg.num_entities, cfg.num_relations
    K_ent, row_ent, K_rel, row_rel = model._rank_layout()
    triples = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    B = len(triples)
    sides = [x for x in "sro" if x in sides]
    kinds = [k for k in KINDS if k[0] in sides]
    ranks = {k: np.zeros(0, dtype=np.float64) for k in kinds}

    if B:
        filt = None
        if filter_triples is not None and len(filter_triples):
            filt = np.unique(np.asarray(filter_triples, dtype=np.int64).reshape(-1, 3), axis=0)
        opts = dict(dtype=torch.float32, device=dev)
        s_v = torch.empty(B, row_ent, **opts)
        r_v = torch.empty(B, row_rel, **opts)
        o_v = torch.empty(B, row_ent, **opts)
        w.pull(triples[:, 0], s_v)
        w.pull(E + triples[:, 1], r_v)
        w.pull(triples[:, 2], o_v)
        true_rows = {"s": s_v, "r": r_v, "o": o_v}
        own = torch.arange(B, dtype=torch.int32)
        nan_base = np.zeros(B, dtype=bool)
        for side in sides:
            q = model._rank_query(side, s_v, r_v, o_v).contiguous()
            K, row, key0, n_cand = ((K_rel, row_rel, E, R) if side == "r"
                                    else (K_ent, row_ent, 0, E))
            base = torch.empty(B, **opts)
            _C.pair_scores(q, true_rows[side], own, base, K)
            raw = 1.0 + _stream_counts(model, q, base, K, row, key0, n_cand, chunk)
            base_h = base.cpu().numpy()
            nan_base |= np.isnan(base_h)
            if side == "r":
                ranks["r"] = raw
                continue
            ranks[side + "_raw"] = raw
            ranks[side] = raw.copy()
            if filt is not None:
                # s side: the other known subjects of (r, o); o side: the
                # other known objects of (s, r)
                cols, ans = ([1, 2], 0) if side == "s" else ([0, 1], 2)
                owner, ids = _competitors(triples[:, cols], triples[:, ans],
                                          filt[:, cols], filt[:, ans])
                ranks[side] -= _filtered_away(model, q, base_h, K, row, owner, ids, chunk)
        for k in kinds:
            ranks[k][nan_base] = np.nan

    names, sums = [], []
    with np.errstate(invalid="ignore"):
        for k in kinds:
            names += [f"mrr_{k}", f"mr_{k}"]
            sums += [float((1.0 / ranks[k]).sum()), float(ranks[k].sum())]
        for h in hits_at:
            for x in sides:
                names.append(f"hits@{h}_{x}")
                sums.append(float((ranks[x] <= h).sum()))
    vec = torch.tensor([float(B)] + sums, dtype=torch.float64)
    if model.world > 1:
        vec = w.allreduce(vec)
    n = float(vec[0])
    out = {k: (float(vec[1 + i]) / n if n else float("nan")) for i, k in enumerate(names)}
    if "s" in sides and "o" in sides:
        out["mrr"] = 0.5 * (out["mrr_s"] + out["mrr_o"])
        out["mr"] = 0.5 * (out["mr_s"] + out["mr_o"])
    out["n"] = n
    if return_ranks:
        out["ranks"] = ranks
    return out


def format_ranks(ev: dict, prefix: str = "") -> str:
    """The reference's three-sided table (pretty_print, :777-786): one line
    per metric, columns subject / relation / object."""
    def line(label, key, scale, cols):
        vals = [f"{scale * ev[key.format(c)]:.2f}" if key.format(c) in ev else "-"
                for c in cols]
        return f"{prefix}  {label:<8}\t" + "\t".join(vals)

    rows = [line("MRR", "mrr_{}", 100, "sro"), line("MRR_RAW", "mrr_{}_raw", 100, "so"),
            line("MR", "mr_{}", 1, "sro"), line("MR_RAW", "mr_{}_raw", 1, "so")]
    hits = sorted({int(k.split("@")[1].split("_")[0]) for k in ev if k.startswith("hits@")})
    rows += [line(f"Hits@{h:02d}", f"hits@{h}" + "_{}", 100, "sro") for h in hits]
    if "mrr" in ev:
        rows.append(f"{prefix}  MRR (s+o)/2 {100 * ev['mrr']:.2f}   MR (s+o)/2 {ev['mr']:.2f}"
                    f"   n {ev['n']:.0f}")
    return "\n".join(rows)
