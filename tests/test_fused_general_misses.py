"""The general fused steps (Server.*_step_fused_general) with MISSED samples in
the batch: the host pass compacts the hit samples, the kernels run on the
compacted arrays, and everything that rides on the compaction (the order across
the 1024-sample chunks of the pass, MF's ratings, the dropout masks' index, the
RESCAL groups and tiles, the model's map back through its sort) is compared
with the fp64 references evaluated on the hit samples alone.

Misses are made in one process, two ways (tests/miss_refs.py): the raw entries
run on rank 0 of a two-rank world built alone, which owns the even keys, so a
sample misses exactly when it names an odd key; the models run on a world-1
store whose device tier is capped, so a sample misses when one of its keys is
in the host-spill tier (Server.key_tier, read, not assumed).

Comparison as everywhere: step_refs.assert_half_close, one half of one table
at a time, err <= 16 * max(e32, 2^-23) with e32 from the fp32 evaluation of the
same reference; every owned row that no hit sample names keeps its bits.
"""
import numpy as np
import pytest
import torch

import miss_refs as mr
import step_refs as sr
from miss_refs import DTS, LR, P_E, P_R, RESCAL, UNIFORM

DEVS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
SEED = 0x5EEDD20B0C0FFEE5  # above 2^62: the whole 64-bit range reaches the kernels
CHUNK = 1024               # samples per chunk of the host pass (resolve_fused)
B_CHUNKS = 2 * CHUNK + 37


def _fam(name, device):
    return f"{name}_general_miss[{'cpu' if device == 'cpu' else 'gpu'}]"


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def _only_missed(keys, missed, hit):
    """The owned (even) keys that missed samples name and no hit sample does."""
    k = np.setdiff1d(np.unique(keys[missed]), np.unique(keys[hit]))
    return k[k % 2 == 0]


def _loss_close(loss, refs, what, fam):
    assert loss.shape == refs[0]["loss"].shape, f"{what}: {tuple(loss.shape)} losses"
    return sr.assert_half_close(loss, refs[0]["loss"], refs[1]["loss"], f"{what} loss", fam)


def run_uniform(device, name, keys, D, N, NS, lr=LR, states=False):
    """One step of a uniform-length entry over `keys` [B][S] (miss_refs
    .unique_keys or any other keys, odd ones missing) on a fresh lone rank."""
    e = UNIFORM[name]
    per, B = e.per(N, NS), keys.shape[0]
    missed = np.flatnonzero((keys % 2).any(1))
    hit = np.setdiff1d(np.arange(B), missed)
    st = mr.LoneStore(device, [(int(keys.max()) + 2, D, 0.3)], seed=71000 + D + B)
    x = 0.5 + torch.arange(B, dtype=torch.float32) / B if name == "mf" else None
    role_keys = mr.split_roles(keys, per)
    rest_keys = _only_missed(keys, missed, hit)
    before = st.key_state(rest_keys) if states else None
    loss, missed_t = e.call(st.raw, role_keys, x, N, NS, D, lr, SEED)
    _sync(device)
    assert missed_t.dtype == torch.int64 and missed_t.tolist() == missed.tolist()
    hk = mr.hit_rows(role_keys, per, hit)
    ins = [st.init[0][k] for k in hk]
    xh = None if x is None else x[torch.from_numpy(hit)]

    def refs(masks):
        return tuple(e.ref(ins, xh, N, NS, D, lr, masks, dt) for dt in DTS)

    masks = e.drop(SEED, len(hit), N, NS, D, P_E, P_R) if e.drop else None
    what, fam = f"{name} B={B} hit={len(hit)} D={D}", _fam(name, device)
    r = refs(masks)
    _loss_close(loss, r, what, fam)
    n_rest = mr.check_table(st, 0, hk, r, e.roles, what, fam, rest_keys, emb_fixed=lr == 0.0)
    return dict(store=st, loss=loss.cpu(), refs=r, refs_of=refs, hit=hit, missed=missed,
                rest_keys=rest_keys, n_rest=n_rest, before=before)


def run_rescal(device, name, D, sizes, N, NS, misses, lr=LR):
    """One step of a RESCAL entry over groups of `sizes` samples with all keys
    different. `misses` = {sample: column of its odd entity key, or "r"}."""
    e = RESCAL[name]
    per, B = e.per(N, NS), sum(sizes)
    ekeys = mr.unique_keys(B, per, {b: c for b, c in misses.items() if c != "r"})
    E = 2 * B * sum(per)
    r_missed = np.array([misses.get(b) == "r" for b in range(B)])
    kr_rel, R = mr.relation_runs(np.repeat(np.arange(len(sizes)), sizes), r_missed)
    missed = np.flatnonzero((ekeys % 2).any(1) | r_missed)
    assert missed.tolist() == sorted(misses)
    hit = np.setdiff1d(np.arange(B), missed)
    st = mr.LoneStore(device, [(E, D, 0.3), (R, D * D, 0.3 / D ** 0.5)], seed=72000 + D + B)
    kr = torch.from_numpy(E + kr_rel)
    role_keys = mr.split_roles(ekeys, per)
    loss, missed_t = e.call(st.raw, [role_keys[0], kr, *role_keys[1:]], None, N, NS, D, lr, SEED)
    _sync(device)
    assert missed_t.dtype == torch.int64 and missed_t.tolist() == missed.tolist()
    what, fam = f"{name} B={B} groups={len(sizes)} hit={len(hit)} D={D}", _fam(name, device)
    if len(hit) == 0:
        assert loss.numel() == 0
        for t in (0, 1):
            assert mr.bits_equal(st.pull(t), st.init[t]), f"{what}: table {t} changed"
        return None
    hk = mr.hit_rows(role_keys, per, hit)
    rel, counts = torch.unique_consecutive(kr[torch.from_numpy(hit)], return_counts=True)
    starts = np.concatenate([[0], np.cumsum(counts.numpy())])
    ins = [st.init[0][hk[0]], st.init[1][rel - E]] + [st.init[0][k] for k in hk[1:]]

    def refs(masks):
        return tuple(e.ref(ins, starts, N, NS, D, lr, masks, dt) for dt in DTS)

    masks = e.drop(SEED, len(hit), N, NS, D, P_E, P_R) if e.drop else None
    r = refs(masks)
    _loss_close(loss, r, what, fam)
    mr.check_table(st, 0, hk, r, e.roles, what, fam, _only_missed(ekeys, missed, hit))
    # R's rows of the runs without a hit sample keep their bits
    lost = np.setdiff1d(E + kr_rel[kr_rel % 2 == 0], rel.numpy())
    mr.check_table(st, 1, [rel], r, ("r",), what, fam, lost)
    return dict(loss=loss.cpu(), refs=r, refs_of=refs, hit=hit, starts=starts, lost=lost)


def _rotate(samples, choices):
    """{sample: choice}, the choices taken in turn."""
    return {int(b): choices[i % len(choices)] for i, b in enumerate(samples)}


# ------------------------------------------------------------ A: compaction across chunks

def _share_ok(n_missed, B):
    assert 0.15 * B <= n_missed <= 0.35 * B, f"{n_missed} of {B} samples miss"


@pytest.mark.parametrize("device", DEVS)
@pytest.mark.parametrize("name", list(UNIFORM))
def test_compaction_across_chunks(device, name, monkeypatch):
    """Three chunks on four pass threads, all keys different, misses through
    every role in turn: the losses are those of the hit samples IN ORDER (for
    MF with their own ratings, for the drop step with the masks of their
    position among the hits), their rows moved, all other rows kept."""
    monkeypatch.setenv("ADAPM_PASS_THREADS", "4")
    B, D, N, NS = B_CHUNKS, 8, 2, 2
    pattern = mr.chunk_pattern(B)
    assert {0, CHUNK - 1, CHUNK, CHUNK + 1, B - 1} <= set(pattern.tolist())
    _share_ok(len(pattern), B)
    S = sum(UNIFORM[name].per(N, NS))
    out = run_uniform(device, name, mr.unique_keys(B, UNIFORM[name].per(N, NS),
                                                   _rotate(pattern, list(range(S)))), D, N, NS)
    assert out["missed"].tolist() == pattern.tolist()
    # every missed sample names S - 1 owned rows, and only it does
    assert len(out["rest_keys"]) == len(pattern) * (S - 1)


@pytest.mark.parametrize("device", DEVS)
@pytest.mark.parametrize("name", list(RESCAL))
def test_compaction_across_chunks_rescal(device, name, monkeypatch):
    """The same for RESCAL, in groups of 17, 16, 1 and 5: a miss through the
    relation cuts its group in two, one through an entity shortens it."""
    monkeypatch.setenv("ADAPM_PASS_THREADS", "4")
    B, D, N, NS = B_CHUNKS, 8, 2, 2
    sizes = ([17, 16, 1, 5] * (B // 39 + 1))
    sizes = sizes[:next(i for i in range(len(sizes)) if sum(sizes[:i + 1]) >= B)]
    sizes.append(B - sum(sizes))
    pattern = mr.chunk_pattern(B)
    _share_ok(len(pattern), B)
    S = sum(RESCAL[name].per(N, NS))
    out = run_rescal(device, name, D, sizes, N, NS, _rotate(pattern, list(range(S)) + ["r"]))
    assert len(out["hit"]) == B - len(pattern)


# ------------------------------------------------------------ B: dropout masks by hit position

def _positions_matter(out, drop, B, N, NS, D, what):
    """The masks are indexed by the position among the HIT samples: the
    reference with masks indexed by the position in the batch is another
    function, by more than the bound, and the step is not that one."""
    by_batch = tuple(m[torch.from_numpy(out["hit"])] for m in drop(SEED, B, N, NS, D, P_E, P_R))
    other = out["refs_of"](by_batch)
    ref64, ref32 = (r["loss"] for r in out["refs"])
    bound = sr.K_MARGIN * max(sr.rel_err(ref32, ref64), sr.EPS_F32)
    assert sr.rel_err(other[0]["loss"], ref64) > bound, f"{what}: take another seed"
    assert sr.rel_err(out["loss"], other[0]["loss"]) > bound, f"{what}: masks by batch position"


@pytest.mark.parametrize("device", DEVS)
def test_drop_masks_by_hit_position_complex(device):
    B, D, N, NS = 40, 8, 2, 2
    keys = mr.unique_keys(B, UNIFORM["kge_drop"].per(N, NS), {0: 0, 1: 3, 2: 5, 7: 1})
    out = run_uniform(device, "kge_drop", keys, D, N, NS)
    assert out["hit"][0] == 3 and len(out["hit"]) == 36
    _positions_matter(out, UNIFORM["kge_drop"].drop, B, N, NS, D, "kge_drop")


@pytest.mark.parametrize("device", DEVS)
def test_drop_masks_by_hit_position_rescal(device):
    D, N, NS = 8, 2, 2
    out = run_rescal(device, "rescal_drop", D, [17, 16, 5], N, NS, {0: 0, 1: 2, 20: 1})
    assert out["starts"].tolist() == [0, 15, 30, 35]
    _positions_matter(out, RESCAL["rescal_drop"].drop, 38, N, NS, D, "rescal_drop")


# ------------------------------------------------------------ C: RESCAL group edges

GROUPS = [17, 16, 1, 5]  # samples 0..16 | 17..32 | 33 | 34..38
EDGES = {
    "17-to-16": ({5: 0}, [0, 16, 32, 33, 38]),
    "single-by-entity": ({33: 1}, [0, 17, 33, 38]),
    "single-by-relation": ({33: "r"}, [0, 17, 33, 38]),
    "first-and-last": ({17: 2, 32: 0, 34: "r", 38: "r"}, [0, 17, 31, 32, 35]),
    "one-group-left": ({**{b: "r" for b in range(17)}, 33: 0, **_rotate(range(34, 39), [0, 1, 2, 3])},
                       [0, 16]),
    "all-missed": (_rotate(range(39), [0, 1, 2, "r"]), None),
}


@pytest.mark.parametrize("device", DEVS)
@pytest.mark.parametrize("edge", list(EDGES))
@pytest.mark.parametrize("D", [8, 64])
@pytest.mark.parametrize("name", list(RESCAL))
def test_rescal_group_edges(device, name, D, edge):
    """Groups, starts and the 16-row tiles are rebuilt from the compacted
    relation offsets: a tile less, a group less, a group cut at its ends, one
    group left, none."""
    misses, starts = EDGES[edge]
    out = run_rescal(device, name, D, GROUPS, 2, 1, misses)
    if starts is None:
        assert out is None
        return
    assert out["starts"].tolist() == starts
    if edge in ("single-by-entity", "one-group-left"):
        assert len(out["lost"]) >= 1  # a relation row named by missed samples only


# ------------------------------------------------------------ D: shared rows, lr = 0

@pytest.mark.parametrize("device", DEVS)
@pytest.mark.parametrize("name,N,NS", [("kge_sides", 2, 2), ("w2v", 3, 0), ("mf", 0, 0)])
def test_shared_rows_lr0(device, name, N, NS):
    """Few rows, so hit samples share them (tests/test_kge_sides.py says why
    lr = 0): embeddings keep their bits, accumulators are acc0 + sum of g^2 over
    the HIT samples' occurrences, and the rows that only missed samples name,
    drawn from a range of their own, are unchanged."""
    B, D = 64, 8
    S = sum(UNIFORM[name].per(N, NS))
    rng = np.random.default_rng(9)
    keys = 2 * rng.integers(0, 10, size=(B, S))            # hit samples: keys 0, 2, .. 18
    missed = np.arange(1, B, 4)
    keys[missed] = 2 * rng.integers(0, 20, size=(len(missed), S))  # and 20, 22, .. 38
    for i, b in enumerate(missed):
        keys[b, i % S] = 41 + 2 * i                          # the odd key of a missed sample
    out = run_uniform(device, name, keys.astype(np.int64), D, N, NS, lr=0.0)
    assert out["missed"].tolist() == missed.tolist()
    assert len(out["rest_keys"]) >= 5 and out["rest_keys"].min() >= 20
    hit_named = np.unique(keys[out["hit"]])
    assert len(hit_named) <= 10 < len(out["hit"])  # rows are shared


# ------------------------------------------------------------ E: bookkeeping

def test_missed_samples_leave_no_sync_state():
    """The pass marks keys for the sync protocol for hit samples only: a key
    that only missed samples name keeps its flags (no UPDATED) and version."""
    from adapm_amd import _C  # noqa: F401

    F_UPDATED = 8
    B, D, N, NS = 40, 8, 2, 1
    S = sum(UNIFORM["kge_sides"].per(N, NS))
    keys = mr.unique_keys(B, UNIFORM["kge_sides"].per(N, NS), _rotate(range(0, B, 3), list(range(S))))
    out = run_uniform("cpu", "kge_sides", keys, D, N, NS, states=True)
    assert len(out["rest_keys"]) == len(out["missed"]) * (S - 1)
    after = out["store"].key_state(out["rest_keys"])
    assert after == out["before"]
    assert all(not (flags & F_UPDATED) and version == 0 for flags, _, version, _ in after)


# ------------------------------------------------------------ G: guard

@pytest.mark.parametrize("device,x_device", [
    ("cpu", "meta"), pytest.param("cuda", "cuda:0", marks=pytest.mark.gpu),
    pytest.param("cpu", "cuda:0", marks=pytest.mark.gpu)])
def test_mf_ratings_must_be_on_the_host(device, x_device):
    """The ratings are compacted on the host: a tensor elsewhere is refused
    before the pass touches a key."""
    st = mr.LoneStore(device, [(16, 8, 0.3)], seed=73000)
    k = torch.tensor([0, 2, 4], dtype=torch.int64)
    before = st.raw.stats()
    with pytest.raises(RuntimeError, match="ratings must be a CPU tensor"):
        st.raw.mf_step_fused_general(k, k + 6, torch.empty(3, dtype=torch.float32, device=x_device),
                                     8, LR, mr.LAM, mr.EPS)
    after = st.raw.stats()
    assert all(after[n] == before[n] for n in ("pulls", "pushes", "pull_keys", "push_keys"))
    assert mr.bits_equal(st.pull(0), st.init[0])


# ------------------------------------------------------------ F: the models on a tiered store

B_M, D_M, N_M, NS_M = 16, 8, 2, 2
CFG_SEED = 5


def _draw(pools, tiers_wanted, rng):
    """One key per wanted tier, each from its pool, never twice."""
    return [pools[t].pop(int(rng.integers(len(pools[t])))) for t in tiers_wanted]


def _two_batches(st, tables_of_cols, rng):
    """Two batches [B_M][S] of keys, no key twice: column c takes its keys from
    table tables_of_cols[c]; every third sample misses, through one spilled key
    in a column, taken in turn, whose table has spilled keys. Returns the
    batches and, per batch, the samples that miss by the tiers as read."""
    pools = {}
    for t in set(tables_of_cols):
        ks = st.keys(t)
        pools[t] = {tier: ks[st.tier[ks] == tier].tolist() for tier in (0, 1)}
    can_miss = [c for c, t in enumerate(tables_of_cols) if pools[t][1]]
    batches, missed, turn = [], [], 0
    for _ in range(2):
        keys = np.empty((B_M, len(tables_of_cols)), dtype=np.int64)
        for b in range(B_M):
            tiers = [0] * len(tables_of_cols)
            if b % 3 == 1:
                tiers[can_miss[turn % len(can_miss)]] = 1
                turn += 1
            keys[b] = [_draw(pools[t], [tier], rng)[0] for t, tier in zip(tables_of_cols, tiers)]
        batches.append(keys)
        m = np.flatnonzero((st.tier[keys] == 1).any(1))
        assert m.tolist() == list(range(1, B_M, 3))  # the split, from key_tier as read
        missed.append(m)
    return batches, missed


def _finish(st, model, names_by_table, keys_by_role, refs, what, fam):
    """Drain, then the whole store against the references: refs is a list of
    (fp64, fp32) pairs, one per launch, keys_by_role[name] the keys of every
    launch's samples in the same order."""
    model.drain()
    st.worker.wait_sync()
    for t, names in enumerate(names_by_table):
        L = st.tables[t][1]
        idx = torch.cat([keys_by_role[n] for n in names]) - int(st.base[t])
        deltas = [torch.cat([torch.cat([torch.cat(r[i][n], dim=1) for r in refs]) for n in names])
                  for i in (0, 1)]
        mr.check_rows(st.init[t], st.pull(t), idx, deltas, L, what, fam)


def _launches(hits, misses, sort_by=None):
    """The samples (indices into both batches, 0..2B-1) of every launch of two
    fused steps and a drain, in launch order: the hit samples of step 1 and of
    step 2, then step 1's missed samples (classic, in step 2, after their
    second miss) and step 2's (classic, at drain)."""
    out = [hits[0], B_M + hits[1], misses[0], B_M + misses[1]]
    if sort_by is not None:  # RESCAL runs every launch sorted by relation
        out = [l[np.argsort(sort_by[l], kind="stable")] for l in out]
    return out


KGE_KINDS = {
    "plain": dict(),
    "sides": dict(neg_samples_subject=NS_M, gamma_entity=mr.GE, gamma_relation=mr.GR),
    "drop": dict(neg_samples_subject=NS_M, gamma_entity=mr.GE, gamma_relation=mr.GR,
                 dropout_entity=P_E, dropout_relation=P_R),
}


def _kge_refs(kind, scorer, ins_of, launches, D):
    """One (fp64, fp32) reference per launch; without dropout the launches are
    one function of the samples, so one call over all of them."""
    import dropout_refs
    import rescal_dropout_refs
    import rescal_sides_refs
    import sides_refs

    NS = 0 if kind == "plain" else NS_M
    tail = (N_M, NS, D, LR, mr.EPS, mr.GE, mr.GR)
    if kind != "drop":
        launches = [np.concatenate(launches)]
    refs = []
    for n, l in enumerate(launches, start=1):
        ins = ins_of(l)
        if kind == "plain":
            f = sr.complex_ref if scorer == "complex" else sr.rescal_ref
            refs.append(tuple(f(*ins[:4], N_M, D, LR, mr.EPS, dt) for dt in DTS))
        elif kind == "sides":
            f = (sides_refs.complex_sides_ref if scorer == "complex"
                 else rescal_sides_refs.rescal_sides_ref)
            refs.append(tuple(f(*ins, *tail, dt) for dt in DTS))
        elif scorer == "complex":
            masks = dropout_refs.drop_masks(mr.launch_seed(CFG_SEED, n), len(l), N_M, NS, D, P_E, P_R)
            refs.append(tuple(dropout_refs.complex_drop_ref(*ins, *tail, masks, dt) for dt in DTS))
        else:  # groups of one sample: every sample has a relation of its own
            masks = rescal_dropout_refs.drop_masks(mr.launch_seed(CFG_SEED, n), len(l), N_M, NS, D,
                                                   P_E, P_R)
            refs.append(tuple(rescal_dropout_refs.rescal_drop_ref(
                ins[0], ins[1], np.arange(len(l) + 1), *ins[2:], *tail, masks, dt) for dt in DTS))
    return launches, refs


@pytest.mark.parametrize("device", DEVS)
@pytest.mark.parametrize("kind", list(KGE_KINDS))
@pytest.mark.parametrize("scorer", ["complex", "rescal"])
def test_model_steps_on_a_tiered_store(device, scorer, kind):
    """Two fused general steps and a drain, no key twice: every sample is
    applied exactly once, the hit ones by the fused step of their batch, the
    spilled ones by the classic step after their second miss or at drain. For
    Rescal the batches are not in relation order, so the missed positions come
    back through the model's sort. The drop models take one seed per launch."""
    from adapm_amd.models.kge import ComplEx, ComplExConfig, Rescal

    D, E, R = D_M, 2 * B_M * (2 + N_M + NS_M) + 9, 4 * B_M + 4
    LR_ = D if scorer == "complex" else D * D
    NS = 0 if kind == "plain" else NS_M
    # every entity and some relations on the device, the relations after them spilled
    cap = E * 2 * D + (R // 2) * 2 * LR_
    st = mr.TieredStore(device, [(E, D, 0.3), (R, LR_, 0.3 if scorer == "complex" else 0.3 / D ** 0.5)],
                        cap, seed=74000)
    try:
        rng = np.random.default_rng(3)
        cols = [0, 1, 0] + [0] * (N_M + NS)  # s | r | o | neg_o | neg_s
        batches, missed = _two_batches(st, cols, rng)
        hits = [np.setdiff1d(np.arange(B_M), m) for m in missed]
        cfg = ComplExConfig(num_entities=E, num_relations=R, dim=D, neg_samples=N_M, lr=LR,
                            eps=mr.EPS, batch_size=B_M, seed=CFG_SEED, **KGE_KINDS[kind])
        model = (ComplEx if scorer == "complex" else Rescal)(cfg, st.server, st.worker)
        negs = [np.concatenate([k[:, 3:3 + N_M].reshape(-1), k[:, 3 + N_M:].reshape(-1)])
                for k in batches]
        draws = iter(negs)
        model._negatives = lambda n, num_keys: next(draws)
        for k, neg in zip(batches, negs):
            triples = np.stack([k[:, 0], k[:, 1] - E, k[:, 2]], axis=1)
            if scorer == "complex":
                model.train_batch_fused(triples, force_general=True)
            else:
                model.train_batch_fused(triples, force_general=True, neg_keys=neg,
                                        fuse_sides=kind == "sides")
        both = torch.from_numpy(np.concatenate(batches))
        launches = _launches(hits, missed, both[:, 1].numpy() if scorer == "rescal" else None)

        def ins_of(l):
            k = both[torch.from_numpy(l)]
            return [st.init[0][k[:, 0]], st.init[1][k[:, 1] - E] if scorer == "rescal"
                    else torch.cat(st.init)[k[:, 1]], st.init[0][k[:, 2]],
                    st.init[0][k[:, 3:3 + N_M].reshape(-1)], st.init[0][k[:, 3 + N_M:].reshape(-1)]]

        launches, refs = _kge_refs(kind, scorer, ins_of, launches, D)
        ks = [both[torch.from_numpy(l)] for l in launches]
        neg_names = ("neg",) if kind == "plain" else ("neg_o", "neg_s")
        by_role = {"s": torch.cat([k[:, 0] for k in ks]), "r": torch.cat([k[:, 1] for k in ks]),
                   "o": torch.cat([k[:, 2] for k in ks]),
                   neg_names[0]: torch.cat([k[:, 3:3 + N_M].reshape(-1) for k in ks])}
        if kind != "plain":
            by_role["neg_s"] = torch.cat([k[:, 3 + N_M:].reshape(-1) for k in ks])
        what, fam = f"{scorer} {kind} model", _fam(f"{scorer}_{kind}_model", device)
        if scorer == "complex":  # one table in the store's eyes: uniform rows
            st.tables, st.init, st.base = [(E + R, D, 0)], [torch.cat(st.init)], st.base[[0, 2]]
            _finish(st, model, [("s", "r", "o") + neg_names], by_role, refs, what, fam)
        else:
            _finish(st, model, [("s", "o") + neg_names, ("r",)], by_role, refs, what, fam)
        if kind == "drop":  # two fused launches, two classic ones
            assert model._drop_steps == 4
    finally:
        st.close()


@pytest.mark.parametrize("device", DEVS)
def test_w2v_model_on_a_tiered_store(device):
    from adapm_amd.models.word2vec import W2VConfig, Word2Vec, syn0, syn1

    V, D, N = 4 * B_M * (2 + N_M), D_M, N_M
    st = mr.TieredStore(device, [(2 * V, D, 0.3)], (2 * V * 2 * D) * 3 // 5, seed=75000)
    try:
        rng = np.random.default_rng(4)
        # words, no word twice: a sample's keys are syn0(centre), syn1(context), syn1(negatives)
        word_tier = {t: [w for w in range(V) if st.tier[2 * w] == st.tier[2 * w + 1] == t]
                     for t in (0, 1)}
        words, missed = [], []
        for _ in range(2):
            w = np.empty((B_M, 2 + N), dtype=np.int64)
            for b in range(B_M):
                tiers = [0] * (2 + N)
                if b % 3 == 1:
                    tiers[(b // 3) % (2 + N)] = 1
                w[b] = _draw(word_tier, tiers, rng)
            words.append(w)
            keys = np.concatenate([syn0(w[:, :1]), syn1(w[:, 1:])], axis=1)
            missed.append(np.flatnonzero((st.tier[keys] == 1).any(1)))
            assert missed[-1].tolist() == list(range(1, B_M, 3))
        cfg = W2VConfig(vocab_size=V, dim=D, negative=N, lr=LR, eps=mr.EPS)
        model = Word2Vec(cfg, st.server, st.worker)
        draws = iter([w[:, 2:].reshape(-1) for w in words])
        model._negatives = lambda n, num_keys: next(draws)
        for w in words:
            model.train_pairs_fused(w[:, 0], w[:, 1], force_general=True)
        w = np.concatenate(words)
        by_role = {"ctr": torch.from_numpy(syn0(w[:, 0])), "ctx": torch.from_numpy(syn1(w[:, 1])),
                   "neg": torch.from_numpy(syn1(w[:, 2:].reshape(-1)))}
        ins = [st.init[0][by_role[n]] for n in ("ctr", "ctx", "neg")]
        refs = [tuple(sr.sgns_ref(*ins, N, D, LR, mr.EPS, dt) for dt in DTS)]
        _finish(st, model, [("ctr", "ctx", "neg")], by_role, refs, "w2v model",
                _fam("w2v_model", device))
    finally:
        st.close()


@pytest.mark.parametrize("device", DEVS)
def test_mf_model_on_a_tiered_store(device):
    from adapm_amd.models.mf import MF, MFConfig

    NR = NC = 4 * B_M
    R = D_M
    st = mr.TieredStore(device, [(NR, R, 0.3), (NC, R, 0.3)], (NR + NC // 2) * 2 * R, seed=76000)
    try:
        batches, missed = _two_batches(st, [0, 1], np.random.default_rng(6))
        x = [(0.5 + (i * B_M + np.arange(B_M)) / (2 * B_M)).astype(np.float32) for i in (0, 1)]
        cfg = MFConfig(num_rows=NR, num_cols=NC, rank=R, lr=LR, lam=mr.LAM, eps=mr.EPS)
        model = MF(cfg, st.server, st.worker)
        for k, xi in zip(batches, x):
            model.train_batch_fused(k[:, 0], k[:, 1] - NR, xi, force_general=True)
        both = torch.from_numpy(np.concatenate(batches))
        ins = [st.init[0][both[:, 0]], st.init[1][both[:, 1] - NR]]
        refs = [tuple(sr.mf_ref(*ins, torch.from_numpy(np.concatenate(x)), R, LR, mr.LAM, mr.EPS, dt)
                      for dt in DTS)]
        by_role = {"w": both[:, 0], "h": both[:, 1]}
        st.tables, st.init, st.base = [(NR + NC, R, 0)], [torch.cat(st.init)], st.base[[0, 2]]
        _finish(st, model, [("w", "h")], by_role, refs, "mf model", _fam("mf_model", device))
    finally:
        st.close()
