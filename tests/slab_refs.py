"""Plain references for the slab ops (adapm_amd/csrc/ops.h).

Each op is written down from its contract in ops.h as a Python loop over the
batch entries, on float64 numpy copies of the slab, the host arena and the
buffer, which it changes in place. Nothing is shared with ops_cpu.cpp or
ops_hip.hip. An offset with bit 62 set names the arena, -1 skips the entry.

The ops move data or add once per element, so a reference rounded to fp32 is
what a correct kernel stores, bit for bit:

  * a copy is exact;
  * fl32(a + b) of two fp32 numbers equals the fp64 sum rounded to fp32
    (fp64 carries more than 2 * 24 + 2 bits, so the second rounding is
    innocuous); extract's `cur - sync` is one such operation, a scatter add
    with unique destinations another;
  * refresh rounds twice, fl32(val + fl32(s - sync)), and the reference
    rounds the delta to fp32 where the contract does;
  * sums of many terms are order-dependent in fp32. The tests feed those
    cases values whose every partial sum is exactly representable, so that
    the fp64 result is the fp32 result in any order, or compare against the
    fp64 result with a tolerance (delta_sqnorm, standard-normal family).
"""
import numpy as np

SPILL_BIT = 1 << 62


def padded(n):
    """Slot length the allocator gives a row of n floats."""
    return (n + 3) & ~3


def _base(dev, host, off):
    off = int(off)
    if off & SPILL_BIT:
        return host, off & ~SPILL_BIT
    return dev, off


def _f32(x):
    return x.astype(np.float32).astype(np.float64)


def gather(dev, host, src, dst, lens, aux, buf, set_=False):
    """buf[dst : +len] = slab[src : +len]"""
    for s, d, n in zip(src, dst, lens):
        if s < 0:
            continue
        b, s = _base(dev, host, s)
        buf[d:d + n] = b[s:s + n]


def scatter(dev, host, src, dst, lens, aux, buf, set_=False):
    """slab[src : +len] += buf[dst : +len], or = when set"""
    for s, d, n in zip(src, dst, lens):
        if s < 0:
            continue
        b, s = _base(dev, host, s)
        if set_:
            b[s:s + n] = buf[d:d + n]
        else:
            b[s:s + n] += buf[d:d + n]


def extract(dev, host, src, dst, lens, aux, buf, set_=False):
    """v = val; buf = v - sync; sync = v"""
    for s, d, n, a in zip(src, dst, lens, aux):
        if s < 0:
            continue
        vb, s = _base(dev, host, s)
        sb, a = _base(dev, host, a)
        v = vb[s:s + n].copy()
        buf[d:d + n] = v - sb[a:a + n]
        sb[a:a + n] = v


def refresh(dev, host, src, dst, lens, aux, buf, set_=False):
    """s = buf; val += fl32(s - sync); sync = s"""
    for s, d, n, a in zip(src, dst, lens, aux):
        if s < 0:
            continue
        vb, s = _base(dev, host, s)
        sb, a = _base(dev, host, a)
        state = buf[d:d + n].copy()
        vb[s:s + n] += _f32(state - sb[a:a + n])
        sb[a:a + n] = state


def zero(dev, host, src, dst, lens, aux, buf, set_=False):
    """slab[dst : +len] = 0 (the slab row is named by dst)"""
    for d, n in zip(dst, lens):
        if d < 0:
            continue
        b, d = _base(dev, host, d)
        b[d:d + n] = 0.0


def delta_sqnorm(dev, host, src, dst, lens, aux, buf, set_=False):
    """buf[dst] = sum (val - sync)^2"""
    for s, d, n, a in zip(src, dst, lens, aux):
        if s < 0:
            continue
        vb, s = _base(dev, host, s)
        sb, a = _base(dev, host, a)
        delta = vb[s:s + n] - sb[a:a + n]
        buf[d] = float((delta * delta).sum())


def delta_sqnorm_f32(dev, host, src, dst, lens, aux, buf):
    """The same in fp32, summed front to back: the yardstick for how much
    error fp32 arithmetic alone puts into a case. Takes fp32 arrays."""
    for s, d, n, a in zip(src, dst, lens, aux):
        if s < 0:
            continue
        vb, s = _base(dev, host, s)
        sb, a = _base(dev, host, a)
        delta = vb[s:s + n] - sb[a:a + n]
        sq = delta * delta
        assert sq.dtype == np.float32
        buf[d] = np.add.accumulate(sq, dtype=np.float32)[-1] if n else np.float32(0)


OFFSET_OPS = {"gather": gather, "scatter": scatter, "scatter_rmw": scatter, "extract": extract,
              "refresh": refresh, "zero": zero, "delta_sqnorm": delta_sqnorm}


def gather_keys(dev, keys, length, plen, world, rank, buf):
    """buf row i = the slot of key i, for keys this rank owns"""
    for i, k in enumerate(keys):
        k = int(k)
        if k % world != rank:
            continue
        s = (k // world) * plen
        buf[i * length:(i + 1) * length] = dev[s:s + length]


def scatter_keys(dev, keys, length, plen, world, rank, buf, set_):
    """the slot of key i += (or =) buf row i, for keys this rank owns"""
    for i, k in enumerate(keys):
        k = int(k)
        if k % world != rank:
            continue
        s = (k // world) * plen
        row = buf[i * length:(i + 1) * length]
        if set_:
            dev[s:s + length] = row
        else:
            dev[s:s + length] += row
