"""The parameter store's own kernels (adapm_amd/csrc/ops_hip.hip) and their
CPU twins against the plain references of tests/slab_refs.py, reached through
the test-only bindings _C.slab_op and _C.slab_keys_op at shapes the Server
never produces: misaligned slab offsets, rows around the thread-loop
boundaries at 256 and 1024 floats, batches around the 16384-workgroup cap,
skipped entries, every placement of value and sync state across HBM slab and
host arena, duplicate destinations, padded slots wider than their row, and
slab offsets past 2^31 floats.

Every comparison but one is bit for bit (slab_refs.py says why that is the
right demand). Slab and arena start out filled with random normal fp32 numbers
and are compared whole, so a float the batch does not name has to keep its
bits; rows lie at least 5 floats apart. Out buffers start as NaN with a
sentinel behind them, and ranges the batch does not name (those of skipped
entries among them) have to stay NaN.

Value families:
  wide   sign * [1, 2) * 2^[-20, 20]. Every such number is a multiple of
         2^-43, so no sum or difference of them is subnormal.
  grid   k / 1024 with integer |k| <= 4096, for duplicate destinations. A sum
         of m such terms is a multiple of 2^-10 below m * 4 <= 2^14 for
         m <= 2^12, hence exact in fp32 in any order. The tests assert that
         the fp64 reference survives a round trip through fp32.
  int    sync integer in [-100, 100], val - sync integer in [-8, 8]
         (delta_sqnorm): a norm of at most 5000 * 64 < 2^24 is exact in any
         order.
  normal standard normal (delta_sqnorm), compared with
         step_refs.assert_half_close: err <= 16 * max(e32, 2^-23), e32 being
         the error of the fp32 front-to-back sum of the same case.

Largest err / max(e32, 2^-23) of the normal family over rows of 1 to 5000
floats (bound 16):

    delta_sqnorm[cpu]   1.00   (the CPU twin is the front-to-back sum itself)
    delta_sqnorm[gpu]   0.554  (at 257 floats; the tree sum is mostly closer
                                to fp64 than the front-to-back sum)

The fp32 atomic add of the MI355X rounds like the plain add: scatter add,
refresh and scatter_keys add are bit-equal on the slab and on the arena.

delta_sqnorm used to take a -1 entry for an offset and read far outside the
slab (both backends; no caller sends one). Writing the skip cases showed it,
before they ever ran; it skips now as every other op does, and test_skips and
test_spill hold it to that.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import slab_refs as refs
import step_refs as sr
from adapm_amd import _C

CPU = pytest.param("cpu", id="cpu")
GPU = pytest.param("cuda:0", id="gpu", marks=pytest.mark.gpu)
DEVICES = [CPU, GPU]

SPILL = refs.SPILL_BIT
# (op, set): scatter_rmw has no CPU twin, so it has no CPU case
VARIANTS = [("gather", False), ("scatter", True), ("scatter", False), ("scatter_rmw", False),
            ("extract", False), ("refresh", False), ("zero", False), ("delta_sqnorm", False)]
OP_DEV = [pytest.param(op, st, dev.values[0], marks=dev.marks,
                       id=f"{op}{'_set' if st else ''}-{dev.id}")
          for (op, st) in VARIANTS for dev in DEVICES
          if not (op == "scatter_rmw" and dev.id == "cpu")]
AUX_OPS = ("extract", "refresh", "delta_sqnorm")
IN_OPS = ("scatter", "scatter_rmw", "refresh")  # the buffer is an input

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 252, 255, 256, 257, 260, 1020, 1024, 1028, 1031, 2052]
MODS = list(itertools.product(range(4), range(4)))  # (slab offset, buffer offset) mod 4


# ------------------------------------------------------------ values

def wide(rng, n):
    v = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-20, 21, n)
    return v.astype(np.float32)


def grid(rng, n):
    return (rng.integers(-4096, 4097, n) / 1024.0).astype(np.float32)


FILL = {"wide": wide, "grid": grid, "int": wide, "normal": wide}


# ------------------------------------------------------------ comparison

def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def assert_bits(got, want64, what):
    """fp32 `got` against the fp64 reference rounded to fp32, bit for bit;
    NaN (never written) has to sit in the same places."""
    want = want64.astype(np.float32)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (
        f"{what}: {int((gn & ~wn).sum())} floats left unwritten, {int((~gn & wn).sum())} written "
        f"that should not be; first at {int(np.flatnonzero(gn != wn)[0])}")
    bad = np.flatnonzero((bits(got) != bits(want)) & ~gn)
    assert bad.size == 0, (f"{what}: {bad.size} floats differ, first at {int(bad[0])}: "
                           f"got {got[bad[0]]!r} want {want[bad[0]]!r}")


def assert_roundtrips(x64, what):
    """Precondition of the order-free cases: fp32 holds the reference exactly."""
    ok = np.isnan(x64) | (x64.astype(np.float32).astype(np.float64) == x64)
    assert ok.all(), f"{what}: reference is not exact in fp32 at {int(np.flatnonzero(~ok)[0])}"


# ------------------------------------------------------------ cases

class Bump:
    """Rows one after another, each at a chosen offset mod 4, at least 5
    untouched floats apart."""

    def __init__(self):
        self.top = 8

    def take(self, n, mod):
        off = ((self.top + 3) & ~3) + mod
        self.top = off + n + 5
        return off

    def size(self):
        return ((self.top + 3) & ~3) + 8


class Case:
    pass


def E(n, smod=0, bmod=0, tier="d", atier="d", dest=None):
    """One batch entry: length, slab and buffer offset mod 4, where the value
    and the sync state live ('d' slab, 'h' arena, tier '-' = skipped), and an
    optional destination id that entries share to name the same row."""
    return (n, smod, bmod, tier, atier, dest)


def build(op, entries, seed, family="wide"):
    """Lay the entries out, draw the values, and run the reference."""
    rng = np.random.default_rng(seed)
    has_aux, is_in = op in AUX_OPS, op in IN_OPS
    slab = {"d": Bump(), "h": Bump()}
    bump = Bump()
    src, dst, lens, aux, rows, shared = [], [], [], [], [], {}
    for i, (n, smod, bmod, tier, atier, dest) in enumerate(entries):
        if tier == "-":
            s = -1
        elif dest is not None and dest in shared:
            s = shared[dest]
        else:
            s = slab[tier].take(n, smod) | (SPILL if tier == "h" else 0)
            if dest is not None:
                shared[dest] = s
        a = (slab[atier].take(n, smod) | (SPILL if atier == "h" else 0)) if has_aux else None
        if op == "zero":
            s, d = 0, s
        elif op == "delta_sqnorm":
            d = 2 * i + 1
        else:
            d = bump.take(n, bmod)
        src.append(s), dst.append(d), lens.append(n), aux.append(a)
        rows.append((s if op != "zero" else d, a, n))

    c = Case()
    c.op, c.n = op, len(entries)
    c.src, c.dst = np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)
    c.lens = np.array(lens, dtype=np.int32)
    c.aux = np.array(aux, dtype=np.int64) if has_aux else None
    c.dev0 = FILL[family](rng, slab["d"].size())
    c.host0 = FILL[family](rng, slab["h"].size()) if slab["h"].top > 8 else None
    c.buf_n = 0 if op == "zero" else 2 * c.n + 1 if op == "delta_sqnorm" else bump.size()
    c.buf0 = FILL[family](rng, c.buf_n) if is_in else None
    if family in ("int", "normal"):
        for s, a, n in rows:
            if s < 0:
                continue
            vb, s = refs._base(c.dev0, c.host0, s)
            sb, a = refs._base(c.dev0, c.host0, a)
            if family == "int":
                sb[a:a + n] = rng.integers(-100, 101, n)
                vb[s:s + n] = sb[a:a + n] + rng.integers(-8, 9, n)
            else:
                sb[a:a + n] = rng.standard_normal(n)
                vb[s:s + n] = rng.standard_normal(n)

    f64 = lambda x: None if x is None else x.astype(np.float64)
    c.dev64, c.host64 = f64(c.dev0), f64(c.host0)
    c.buf64 = f64(c.buf0) if is_in else np.full(c.buf_n, np.nan)
    return c


def reference(c, set_):
    refs.OFFSET_OPS[c.op](c.dev64, c.host64, c.src, c.dst, c.lens, c.aux, c.buf64, set_)
    for a in (c.dev0, c.host0, c.buf0, c.dev64, c.host64, c.buf64, c.src, c.dst, c.lens, c.aux):
        if a is not None:
            a.setflags(write=False)
    return c


def _sync(device):
    if device != "cpu":
        torch.cuda.synchronize()


def run(c, set_, device):
    """The op on copies of the case's inputs -> (slab, arena, buffer) after."""
    gpu = device != "cpu"
    dev = torch.from_numpy(c.dev0.copy()).to(device)
    host = None
    if c.host0 is not None:
        host = torch.from_numpy(c.host0.copy())
        host = host.pin_memory() if gpu else host
    guard = buf = None
    if c.buf0 is not None:
        buf = torch.from_numpy(c.buf0.copy()).to(device)
    elif c.op != "zero":
        guard = sr.guarded_vec(c.buf_n, device)
        buf = guard.out
    t = lambda x: None if x is None else torch.from_numpy(x.copy())
    _C.slab_op(c.op, dev, host, t(c.src), t(c.dst), t(c.lens), t(c.aux), buf, set_)
    _sync(device)
    if guard is not None:
        guard.check(c.op)
    return (dev.cpu().numpy(), None if host is None else host.numpy(),
            None if buf is None else buf.cpu().numpy())


def check(c, set_, device, what):
    """Run and compare everything bit for bit."""
    dev, host, buf = run(c, set_, device)
    assert_bits(dev, c.dev64, f"{what}: slab")
    if host is not None:
        assert_bits(host, c.host64, f"{what}: arena")
    if buf is not None:
        assert_bits(buf, c.buf64, f"{what}: buffer")


def fam(op):
    return "int" if op == "delta_sqnorm" else "wide"


@functools.lru_cache(maxsize=None)
def lengths_case(op, set_):
    return reference(build(op, [E(n) for n in LENGTHS], 11, fam(op)), set_)


@functools.lru_cache(maxsize=None)
def alignment_case(op, set_):
    ent = [E(n, sm, bm) for n in (8, 1028) for sm, bm in MODS]
    ent += [E(n) for n in (1026, 1027, 1029)]
    return reference(build(op, ent, 12, fam(op)), set_)


@functools.lru_cache(maxsize=None)
def skips_case(op, set_, only):
    if only:
        ent = [E(5, tier="-"), E(8, tier="-"), E(1028, tier="-")]
    else:
        ent = [E(8, tier="-"), E(8), E(5, 1, 2), E(260, tier="-"), E(1028), E(3), E(1028, tier="-")]
    return reference(build(op, ent, 13, fam(op)), set_)


@functools.lru_cache(maxsize=None)
def batch_case(op, set_, n, length):
    return reference(build(op, [E(length)] * n, 14 + n + length, fam(op)), set_)


def spill_entries():
    """Slab and arena entries with skips between them; for the ops with a
    sync state, every (value, sync) placement at every length."""
    tiers = [("d", "d"), ("h", "h"), ("d", "h"), ("h", "d")]
    ent = []
    for i, n in enumerate([1, 3, 4, 5, 8, 255, 256, 257, 1020, 1024, 1028, 1031, 2052]):
        for j, (t, a) in enumerate(tiers):
            ent.append(E(n, tier=t, atier=a))
            if (i + j) % 5 == 0:
                ent.append(E(n, tier="-", atier=a))
    for k, (sm, bm) in enumerate(MODS):
        t, a = tiers[(k + k // 4) % 4]
        ent.append(E(8, sm, bm, t, a))
        t, a = tiers[(k + k // 4 + 1) % 4]
        ent.append(E(8, sm, bm, t, a))
    for k, (sm, bm) in enumerate([(0, 0), (1, 0), (0, 1), (3, 2), (2, 2), (0, 0), (0, 3), (2, 0)]):
        t, a = tiers[k % 4]
        ent.append(E(1028, sm, bm, t, a))
    return ent


@functools.lru_cache(maxsize=None)
def spill_case(op, set_):
    return reference(build(op, spill_entries(), 15, fam(op)), set_)


# ------------------------------------------------------------ offset-batch ops

@pytest.mark.parametrize("op,set_,device", OP_DEV)
def test_lengths(op, set_, device):
    """Rows on either side of the scalar loop's second trip (256 floats) and
    of the float4 loop's (1024 floats), all offsets aligned."""
    check(lengths_case(op, set_), set_, device, "lengths")


@pytest.mark.parametrize("op,set_,device", OP_DEV)
def test_alignment(op, set_, device):
    """All 16 (slab offset, buffer offset) mod 4 at 8 and 1028 floats, and
    aligned rows whose length is no multiple of 4: each of the three terms of
    vec_ok decides alone."""
    check(alignment_case(op, set_), set_, device, "alignment")


@pytest.mark.parametrize("only", [False, True], ids=["mixed", "only"])
@pytest.mark.parametrize("op,set_,device", OP_DEV)
def test_skips(op, set_, device, only):
    """-1 entries first, in the middle and last, and a batch of nothing else:
    their buffer ranges stay NaN, slab and arena keep every bit."""
    c = skips_case(op, set_, only)
    if only:
        assert (c.src if op != "zero" else c.dst).max() == -1
    check(c, set_, device, "skips")


@pytest.mark.parametrize("length", [4, 5])
@pytest.mark.parametrize("n", [0, 1, 2, 16384, 16385, 16403])
@pytest.mark.parametrize("op,set_,device", OP_DEV)
def test_batch_size(op, set_, device, n, length):
    """Around the cap of 16384 workgroups: above it a workgroup takes a
    second entry. An empty batch launches nothing and touches nothing."""
    check(batch_case(op, set_, n, length), set_, device, f"n={n} len={length}")


@pytest.mark.parametrize("op,set_,device", OP_DEV)
def test_spill(op, set_, device):
    """Slab and arena operands in one batch; value and sync state are placed
    independently."""
    c = spill_case(op, set_)
    assert c.host0 is not None
    if op in AUX_OPS:
        placed = {(bool(s & SPILL), bool(a & SPILL)) for s, a in zip(c.src, c.aux) if s >= 0}
        assert len(placed) == 4
    check(c, set_, device, "spill")


def test_scatter_rmw_has_no_cpu_twin():
    c = lengths_case("scatter", False)
    with pytest.raises(RuntimeError, match="no CPU backend"):
        t = lambda x: torch.from_numpy(x.copy())
        _C.slab_op("scatter_rmw", t(c.dev0), None, t(c.src), t(c.dst), t(c.lens), None, t(c.buf0),
                   False)


# ---- duplicate destinations (scatter add)

@functools.lru_cache(maxsize=None)
def dup_case(kind):
    if kind == "one_row":  # one destination named 512 times, among others
        ent = [E(260, bmod=i % 4, dest=0 if i % 2 == 0 or i >= 400 else None) for i in range(712)]
        assert sum(e[5] == 0 for e in ent) == 512
    else:  # half of 16400 entries on 4 destinations: 2050 terms and the prior
        ent = [E(5, dest=(i // 2) % 4 if i % 2 == 0 else None) for i in range(16400)]
    c = reference(build("scatter", ent, 21, "grid"), False)
    assert_roundtrips(c.dev64, f"duplicates {kind}")
    return c


@pytest.mark.parametrize("kind", ["one_row", "skewed"])
@pytest.mark.parametrize("device", DEVICES)
def test_scatter_add_duplicates(device, kind):
    """Sums whose every partial sum is exact: bit-equal in any order."""
    check(dup_case(kind), False, device, f"duplicates {kind}")


# ---- delta_sqnorm, standard-normal values

@functools.lru_cache(maxsize=None)
def sqnorm_normal_case():
    tiers = [("d", "d"), ("h", "h"), ("d", "h"), ("h", "d")]
    ent = [E(n, i % 4, 0, *tiers[i % 4]) for i, n in enumerate(LENGTHS + [4999, 5000])]
    ent.insert(3, E(64, tier="-"))
    c = reference(build("delta_sqnorm", ent, 31, "normal"), False)
    c.buf32 = np.full(c.buf_n, np.nan, dtype=np.float32)
    refs.delta_sqnorm_f32(c.dev0, c.host0, c.src, c.dst, c.lens, c.aux, c.buf32)
    return c


@pytest.mark.parametrize("device", DEVICES)
def test_delta_sqnorm_normal(device):
    """The wave and LDS reduction against the fp64 norm, K = 16 rule."""
    c = sqnorm_normal_case()
    dev, host, buf = run(c, False, device)
    assert_bits(dev, c.dev64, "sqnorm: slab")
    assert_bits(host, c.host64, "sqnorm: arena")
    named = ~np.isnan(c.buf64)
    assert np.array_equal(np.isnan(buf), ~named), "sqnorm: wrote a norm nobody asked for"
    label = f"delta_sqnorm[{'cpu' if device == 'cpu' else 'gpu'}]"
    worst = 0.0
    for i in np.flatnonzero(named):  # one norm at a time: each has its own scale
        j = (i - 1) // 2
        worst = max(worst, sr.assert_half_close(
            torch.tensor(buf[i:i + 1]), torch.tensor(c.buf64[i:i + 1]),
            torch.tensor(c.buf32[i:i + 1]), f"len={c.lens[j]}", label))
    print(f"RATIO {label} largest: {worst:.3g}")


# ---- slab offsets past 2^31 floats (GPU only)

@pytest.mark.gpu
@pytest.mark.parametrize("op,set_", [("gather", False), ("scatter", True), ("scatter", False)],
                         ids=["gather", "scatter_set", "scatter"])
def test_large_offsets(op, set_):
    """Rows astride, at and past 2^31 floats: a 32-bit offset would land near
    the start of the slab. The slab is left uninitialised but for a window
    around the rows, which is the reference's whole slab."""
    total = 2 ** 31 + 8192
    try:
        dev = torch.empty(total, dtype=torch.float32, device="cuda:0")
    except RuntimeError as e:  # OutOfMemoryError is one
        pytest.skip(f"cannot allocate a slab of 2^31 + 8192 floats: {e}")
    lo = 2 ** 31 - 8 - 64
    rows = [(2 ** 31 - 8, 16), (2 ** 31 + 72, 1028), (2 ** 31 + 72 + 1028 + 64 + 1, 257)]
    hi = rows[-1][0] + rows[-1][1] + 64
    assert hi <= total
    rng = np.random.default_rng(41)
    win0 = wide(rng, hi - lo)
    bump = Bump()
    dst = np.array([bump.take(n, m) for (_, n), m in zip(rows, (0, 0, 2))], dtype=np.int64)
    src = np.array([s for s, _ in rows], dtype=np.int64)
    lens = np.array([n for _, n in rows], dtype=np.int32)
    buf0 = wide(rng, bump.size()) if op == "scatter" else None
    win64 = win0.astype(np.float64)
    buf64 = buf0.astype(np.float64) if op == "scatter" else np.full(bump.size(), np.nan)
    refs.OFFSET_OPS[op](win64, None, src - lo, dst, lens, None, buf64, set_)

    dev[lo:hi] = torch.from_numpy(win0).cuda()
    dev[:4096] = 0.0  # where a truncated offset would point
    guard = None
    if op == "scatter":
        buf = torch.from_numpy(buf0.copy()).cuda()
    else:
        guard = sr.guarded_vec(bump.size(), "cuda:0")
        buf = guard.out
    _C.slab_op(op, dev, None, torch.from_numpy(src), torch.from_numpy(dst),
               torch.from_numpy(lens), None, buf, set_)
    torch.cuda.synchronize()
    if guard is not None:
        guard.check(op)
    assert_bits(dev[lo:hi].cpu().numpy(), win64, f"{op} past 2^31: window")
    assert_bits(buf.cpu().numpy(), buf64, f"{op} past 2^31: buffer")
    assert not dev[:4096].any().item(), f"{op} past 2^31: wrote near the start of the slab"
    del dev
    torch.cuda.empty_cache()


# ------------------------------------------------------------ key-batch ops

KEY_LENS = [1, 3, 4, 5, 64, 256, 260, 1028, 2052]
KEY_VARIANTS = [("gather_keys", False), ("scatter_keys", True), ("scatter_keys", False)]
KEY_OP_DEV = [pytest.param(op, st, dev.values[0], marks=dev.marks,
                           id=f"{op}{'_set' if st else ''}-{dev.id}")
              for (op, st) in KEY_VARIANTS for dev in DEVICES]


@functools.lru_cache(maxsize=None)
def keys_case(op, set_, keys_id, length, plen, world, rank, rows, seed):
    """keys_id: ("rand", n) keys drawn with repeats, ("perm", n) without,
    ("one", n) / ("skew", n) the duplicate mixes for add."""
    rng = np.random.default_rng(seed)
    kind, n = keys_id
    nk = rows * world
    if kind == "rand":
        keys = rng.integers(0, nk, n)
    elif kind == "perm":
        keys = rng.permutation(nk)[:n]
        assert len(keys) == n
    elif kind == "one":  # 512 times one owned key among others
        hot = rank + world * (rows // 2)
        keys = rng.permutation(nk)[:n]
        keys = keys[keys != hot][:n - 512]
        keys = rng.permutation(np.concatenate([keys, np.full(512, hot)]))
    else:  # half the batch on 4 owned keys
        hot = rank + world * np.arange(4)
        keys = rng.integers(0, nk, n)
        keys[::2] = hot[(np.arange(len(keys[::2]))) % 4]
    c = Case()
    c.keys = keys.astype(np.int64)
    # a set with a key named twice has no defined winner
    assert not (set_ and len(np.unique(c.keys)) != len(c.keys))
    exact = op == "scatter_keys" and not set_
    fill = grid if exact else wide
    c.dev0 = fill(rng, rows * plen + 8)
    c.buf_n = len(keys) * length
    c.buf0 = fill(rng, c.buf_n) if op == "scatter_keys" else None
    c.dev64 = c.dev0.astype(np.float64)
    if op == "gather_keys":
        c.buf64 = np.full(c.buf_n, np.nan)
        refs.gather_keys(c.dev64, c.keys, length, plen, world, rank, c.buf64)
    else:
        c.buf64 = c.buf0.astype(np.float64)
        refs.scatter_keys(c.dev64, c.keys, length, plen, world, rank, c.buf64, set_)
    if exact:
        assert_roundtrips(c.dev64, "scatter_keys add")
    for a in (c.keys, c.dev0, c.buf0, c.dev64, c.buf64):
        if a is not None:
            a.setflags(write=False)
    return c


def check_keys(op, set_, device, c, length, plen, world, rank, what):
    dev = torch.from_numpy(c.dev0.copy()).to(device)
    guard = None
    if c.buf0 is not None:
        buf = torch.from_numpy(c.buf0.copy()).to(device)
    else:
        guard = sr.guarded_vec(c.buf_n, device)
        buf = guard.out
    _C.slab_keys_op(op, dev, torch.from_numpy(c.keys.copy()), length, plen, world, rank, buf, set_)
    _sync(device)
    if guard is not None:
        guard.check(what)
    assert_bits(dev.cpu().numpy(), c.dev64, f"{what}: slab")
    assert_bits(buf.cpu().numpy(), c.buf64, f"{what}: buffer")


@pytest.mark.parametrize("length", KEY_LENS)
@pytest.mark.parametrize("op,set_,device", KEY_OP_DEV)
def test_keys_shapes(op, set_, device, length):
    """Every (world, rank), slots of padded(len) and of padded(len) + 4
    floats: rows of keys owned elsewhere stay NaN (gather) or untouched
    (scatter), and the slab is strided by plen, the buffer by len."""
    rows = 5
    for world in (1, 2, 3):
        for rank in range(world):
            for extra in (0, 4):
                plen = refs.padded(length) + extra
                kid = ("perm", rows * world) if set_ else ("rand", 2 * rows * world + 1)
                c = keys_case(op, set_, kid, length, plen, world, rank, rows, 51 + length)
                check_keys(op, set_, device, c, length, plen, world, rank,
                           f"{op} len={length} plen={plen} world={world} rank={rank}")


@pytest.mark.parametrize("length", [4, 5])
@pytest.mark.parametrize("n", [0, 1, 16385, 16403])
@pytest.mark.parametrize("op,set_,device", KEY_OP_DEV)
def test_keys_batch_size(op, set_, device, n, length):
    world, rank, rows = 2, 1, 8300
    c = keys_case(op, set_, ("perm" if set_ else "rand", n), length, refs.padded(length), world,
                  rank, rows, 61 + n)
    check_keys(op, set_, device, c, length, refs.padded(length), world, rank, f"{op} n={n}")


@pytest.mark.parametrize("kid", [("one", 712), ("skew", 16400)], ids=["one_row", "skewed"])
@pytest.mark.parametrize("device", DEVICES)
def test_keys_add_duplicates(device, kid):
    length = 260 if kid[0] == "one" else 5
    world, rank, rows = 2, 1, 600
    c = keys_case("scatter_keys", False, kid, length, refs.padded(length), world, rank, rows, 71)
    counts = np.unique(c.keys, return_counts=True)[1]
    assert counts.max() >= 512
    check_keys("scatter_keys", False, device, c, length, refs.padded(length), world, rank,
               f"scatter_keys duplicates {kid[0]}")


# ------------------------------------------------------------ binding guards

def test_bindings_refuse_ranges_outside_their_tensor():
    """The guard that keeps these tests from writing out of bounds."""
    dev, buf = torch.zeros(64), torch.zeros(16)
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    for src, dst, ln in [(60, 0, 5), (0, 12, 5), (-2, 0, 4), (0, -1, 4), (SPILL, 0, 4), (0, 0, -1)]:
        with pytest.raises(RuntimeError):
            _C.slab_op("gather", dev, None, i64(src), i64(dst), i32(ln), None, buf, False)
    with pytest.raises(RuntimeError):  # sync state outside the slab
        _C.slab_op("extract", dev, None, i64(0), i64(0), i32(4), i64(61), buf, False)
    with pytest.raises(RuntimeError):  # n differs
        _C.slab_op("gather", dev, None, i64(0, 8), i64(0), i32(4), None, buf, False)
    with pytest.raises(RuntimeError):  # arena offset outside the arena
        _C.slab_op("gather", dev, torch.zeros(8), i64(SPILL | 6), i64(0), i32(4), None, buf, False)
    for keys, ln, plen, world, rank in [((16,), 4, 4, 1, 0), ((0, 1, 2, 3, 4), 4, 4, 1, 0),
                                        ((0,), 8, 4, 1, 0), ((0,), 4, 6, 1, 0), ((0,), 4, 4, 2, 2),
                                        ((-1,), 4, 4, 1, 0)]:
        with pytest.raises(RuntimeError):
            _C.slab_keys_op("gather_keys", dev, i64(*keys), ln, plen, world, rank, buf, False)
    assert not dev.any() and not buf.any()


@pytest.mark.gpu
def test_gpu_arena_has_to_be_device_visible():
    """A pageable arena is refused on the host; no kernel gets to see it."""
    dev, buf = torch.zeros(64, device="cuda:0"), torch.zeros(16, device="cuda:0")
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="not device-visible"):
        _C.slab_op("gather", dev, torch.ones(64), i64(SPILL), i64(0),
                   torch.tensor([4], dtype=torch.int32), None, buf, False)
    torch.cuda.synchronize()
    assert not buf.any().item()


# ------------------------------------------------------------ through the Server

SERVER_LENS = [3, 5, 260, 1028, 2052, 4, 7, 256, 1, 1031]


def _server_roundtrip(device, spill):
    """set, pull, push, pull of every key of a non-uniform store in one batch:
    slab offsets are aligned, the flat buffer's are not."""
    import adapm_amd

    lens = np.array(SERVER_LENS * 3, dtype=np.int64)
    nk = len(lens)
    adapm_amd._SETUP.clear()
    adapm_amd.runtime._RUNTIME = None
    kw = {}
    if spill:  # room for about a third of the rows on the device
        kw = dict(device_cap_gb=int(lens.sum()) // 3 * 4 / 2 ** 30, host_spill_gb=0.01)
    adapm_amd.setup(num_keys=nk, num_threads=1, device=device, **kw)
    s = adapm_amd.Server(torch.from_numpy(lens))
    try:
        if spill:
            tiers = np.array([s.raw.key_tier(k) for k in range(nk)])
            assert (tiers == 0).any() and (tiers == 1).any(), tiers
        w = adapm_amd.Worker(0, s)
        rng = np.random.default_rng(81)
        keys = rng.permutation(nk).astype(np.int64)
        kl = lens[keys].astype(np.int32)
        flat = np.concatenate([[0], np.cumsum(kl)[:-1]]).astype(np.int64)
        assert (flat % 4 != 0).any()
        total = int(kl.sum())
        # the model store: key k's slot at the sum of the padded lengths before it
        slot = np.concatenate([[0], np.cumsum((lens + 3) & ~3)[:-1]]).astype(np.int64)
        model = np.zeros(int(slot[-1] + lens[-1] + 3), dtype=np.float64)
        v0, v1 = wide(rng, total), wide(rng, total)
        dev_t = lambda x: torch.from_numpy(x.copy()).to(device)

        def pull():
            g = sr.guarded_vec(total, device)
            w.pull(keys, g.out)
            _sync(device)
            g.check("pull")
            want = np.full(total, np.nan)
            refs.gather(model, None, slot[keys], flat, kl, None, want)
            assert_bits(g.out.cpu().numpy(), want, f"server pull (spill={spill})")

        w.set(keys, dev_t(v0))
        refs.scatter(model, None, slot[keys], flat, kl, None, v0.astype(np.float64), True)
        pull()
        w.push(keys, dev_t(v1))
        refs.scatter(model, None, slot[keys], flat, kl, None, v1.astype(np.float64), False)
        pull()
    finally:
        s.shutdown()


@pytest.mark.parametrize("device", DEVICES)
def test_server_nonuniform_misaligned_buffer(device):
    _server_roundtrip(device, spill=False)
    _server_roundtrip(device, spill=True)
