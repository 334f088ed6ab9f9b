"""References for the word2vec window step, written from the contract in
kernels.h (w2v_window_step): rules 1-5 on Python ints, rules 7-9 on top of
step_refs.sgns_ref in the dtype asked for."""
import torch

from step_refs import sgns_ref

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def mix(x):  # pcg_hash64
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    return x ^ (x >> 33)


def _unit(h):
    return ((h >> 40) & 0xFFFFFF) * 2.0 ** -24  # exact, as the fp32 product is


def window_plan_ref(tok, starts, keep, prob, alias, W, N, seed):
    """Rules 1-5 -> (ctok, pairs): pairs lists (c, ctr, ctx, [negs]) in (c, a) order."""
    sd = [mix(seed + k) for k in range(3)]
    ctok, lo, hi = [], [], []
    for s in range(len(starts) - 1):
        first = len(ctok)
        for p in range(starts[s], starts[s + 1]):
            if keep is None or _unit(mix(sd[0] ^ p * GOLD)) < float(keep[tok[p]]):
                ctok.append(int(tok[p]))
        lo += [first] * (len(ctok) - first)
        hi += [len(ctok)] * (len(ctok) - first)
    pairs = []
    for c, w in enumerate(ctok):
        b = 1 + mix(sd[1] ^ c * GOLD) % W
        for a in range(W - b, W + b + 1):
            j = c - W + a
            if a == W or not lo[c] <= j < hi[c]:
                continue
            negs = []
            for d in range(N):
                h = mix(sd[2] ^ ((c * (2 * W + 1) + a) * N + d) * GOLD)
                slot = h % len(prob)
                negs.append(slot if _unit(h) < float(prob[slot]) else int(alias[slot]))
            pairs.append((c, w, ctok[j], negs))
    return ctok, pairs


def window_step_ref(store, pairs, T, N, D, lr, eps, dtype):
    """Rules 7-9, serial and in compacted order, in `dtype`: (store after,
    loss[T]). store is [2V][2D], row 2w syn0 and row 2w+1 syn1 of word w. Each
    pair is one sgns_ref step of the held centre; its deltas land on the
    target rows one occurrence after the other."""
    st = store.to(dtype).clone()
    loss = torch.zeros(T, dtype=dtype)
    cur = held = read = None
    for c, wc, wx, negs in pairs + [(None, None, None, None)]:
        if c != cur:
            if cur is not None:
                st[2 * cw] += held - read
            if c is None:
                break
            cur, cw = c, wc
            read = st[2 * wc].clone()
            held = read.clone()
        rows = [2 * wx + 1] + [2 * w + 1 for w in negs]
        r = sgns_ref(held[None], st[rows[:1]], st[rows[1:]].reshape(N, 2 * D), N, D, lr, eps,
                     dtype)
        loss[c] += r["loss"][0]
        for i, row in enumerate(rows):
            delta, g2 = r["ctx"] if i == 0 else r["neg"]
            st[row, :D] += delta[max(i - 1, 0)]
            st[row, D:] += g2[max(i - 1, 0)]
        held[:D] += r["ctr"][0][0]
        held[D:] += r["ctr"][1][0]
    return st, loss
