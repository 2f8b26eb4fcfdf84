"""Deterministic (seg, band, null, maxDist) cases for the built-in spatial statistics (mean coordinates, edge
pixels, variogram).  Imports neither the GPU nor the library.

The variogram is where the kernels can go wrong quietly.  The reference adds (double)(int64)(d*d) into a float64
sum per (segment, bin), in the order (row, column, yo, xo); the device adds d*d as integers.  The two agree only
while every square and every bin total stay below 2^53, so the cases span:
  pixel types   u8, i16, u16 over their full range; i32 and u32 in three bands of values:
                  narrow  |d| < 2^20: every square and every bin total exact, nothing to recompute
                  mid     squares >= 2^53: the float64 sum rounds, the device's uint64 total wraps
                  full    the whole range: the reference's int64 square wraps negative (|d| > 3037000499)
  extremes      values only at the type's limits, the null at the minimum or at the maximum
  segments      1-pixel segments, an all-nodata segment, ids without pixels, segments on the right and bottom
                edges, interleaved non-convex combs (pairs only inside a segment), and one >= 10^6-pixel 16-bit
                checkerboard segment whose bin totals pass 2^53 with every square exact
  order         a diagonal chain of one uint32 segment whose bin-1 terms are +2^62, 40 terms of 484 that vanish
                under the ulp of 2^62, then -2^62 + 1790155657: the reference's sequential sum differs from the
                exact, the reversed and the pairwise sum (plant_chain), so only the reference's order passes
  maxDist       1, 2, 5, 12, 64 and 255 (256 is refused)

`case.make()` returns (seg uint32, band, null_val, max_seg_id); the values come from a stream seeded by the case
name, so two calls give the same arrays.  `WIDE` names the cases whose variogram the integer formula gets wrong
(`int_model_variogram` shows it); `BIG` names the case whose segment is too large for exact float64 coordinate
sums.
"""
import functools
import zlib

import numpy as np

MAXDISTS = (1, 2, 5, 12, 64, 255)
EXACT = 1 << 53


class Case:
    def __init__(self, name, layout, dtype, regime, null='min', maxds=(5,)):
        self.name, self.layout, self.dtype, self.regime = name, layout, np.dtype(dtype), regime
        self.null, self.maxds = null, tuple(maxds)

    def __repr__(self):
        return self.name

    def make(self):
        return _make(self.name)


def _blocks():
    """60 x 64: a 3 x 4 grid of blocks (the last row and column on the image's edges), a 1-pixel segment inside
    block 1, an all-nodata block (id 6, nulled by make), label-0 stripes and ids 14..16 without pixels."""
    seg = np.zeros((60, 64), dtype=np.uint32)
    for i in range(3):
        for j in range(4):
            seg[i * 20:(i + 1) * 20, j * 16:(j + 1) * 16] = 1 + i * 4 + j
    seg[7, 5] = 13                           # 1 pixel
    seg[30, 20:40] = 0
    seg[:, 47] = 0
    return seg, 16


def _combs():
    """40 x 44: two interleaved combs -- teeth of 2 columns, spine rows at the top (id 1) and bottom (id 2) -- and
    scattered single pixels of id 3 inside them; pairs of a comb never cross into the other."""
    seg = np.zeros((40, 44), dtype=np.uint32)
    for c in range(44):
        seg[2:38, c] = 1 if (c // 2) % 2 == 0 else 2
    seg[0:2, :] = 1
    seg[38:40, :] = 2
    seg[10::9, 5::11] = 3
    return seg, 3


def _big():
    """1100 x 1000, one segment of 1.1 * 10^6 pixels"""
    return np.ones((1100, 1000), dtype=np.uint32), 1


def _chain():
    """50 x 50 of segment 1; plant_chain puts segment 2 on the diagonal (3, 3) .. (45, 45)"""
    return np.ones((50, 50), dtype=np.uint32), 2


LAYOUTS = {'blocks': _blocks, 'combs': _combs, 'big': _big, 'chain': _chain}

# uint32 values down the chain: squares of differences 2^62, then 40 x 22^2, then the int64 wrap of
# 3719550787^2 = -2^62 + 1790155657 (the sum after the first term is 2^62 until the last term)
CHAIN = (1 << 31,) + tuple(22 * k for k in range(41)) + (880 + 3719550787,)


def plant_chain(seg, band, r0, c0, sid):
    """segment sid on the diagonal (r0 + i, c0 + i), i < len(CHAIN), with the CHAIN values (in place)"""
    for (i, v) in enumerate(CHAIN):
        seg[r0 + i, c0 + i] = sid
        band[r0 + i, c0 + i] = v


def reference_terms(seg, band, null, maxd, sid, b):
    """the terms the reference adds into bin b (1-based) of segment sid, in its order (pixels in raster order,
    each pixel's offsets (yo, xo) in order): the int64 square, wrapped as numba wraps it (the reference adds
    their float64 values)"""
    (nr, nc) = seg.shape
    mem = (seg == sid) & (band.astype(np.int64) != null)
    offs = [(yo, xo) for yo in range(1, maxd + 1) for xo in range(1, maxd + 1)
            if int(np.sqrt(yo * yo + xo * xo)) == b]
    out = []
    for (y, x) in zip(*np.nonzero(mem)):
        for (yo, xo) in offs:
            if y + yo < nr and x + xo < nc and mem[y + yo, x + xo]:
                sq = (int(band[y, x]) - int(band[y + yo, x + xo])) ** 2 % (1 << 64)
                out.append(sq - (1 << 64) if sq >= (1 << 63) else sq)
    return np.array(out, dtype=np.int64)


def _values(shape, dtype, regime, rng):
    info = np.iinfo(dtype)
    if regime == 'full':
        lo, hi = int(info.min), int(info.max)
    elif regime == 'narrow':
        lo, hi = (-(1 << 19), 1 << 19) if info.min < 0 else (1 << 30, (1 << 30) + (1 << 20))
    elif regime == 'mid':
        lo, hi = (-10 ** 9, 10 ** 9) if info.min < 0 else (0, 2 * 10 ** 9)
    elif regime == 'extreme':
        return np.where(rng.rand(*shape) < 0.5, info.min, info.max).astype(dtype)
    elif regime == 'chain':
        lo, hi = 1 << 30, (1 << 30) + 1000
    elif regime == 'checker':
        (r, c) = np.indices(shape)
        return np.where((r + c) % 2 == 0, 0, info.max - 1).astype(dtype)
    else:
        raise ValueError(regime)
    v = rng.randint(lo, hi, size=shape, dtype=np.int64)
    v[0, 0], v[-1, -1] = lo, hi                                      # the range's ends planted
    return v.astype(dtype)


@functools.lru_cache(maxsize=None)
def _make(name):
    case = CASES[name]
    (seg, S) = LAYOUTS[case.layout]()
    rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
    band = _values(seg.shape, case.dtype, case.regime, rng)
    info = np.iinfo(case.dtype)
    null = int(info.min) if case.null == 'min' else int(info.max)
    if case.regime == 'extreme':      # the other limit stays, the null's limit becomes its neighbour
        band = np.where(band == null, null + (1 if case.null == 'min' else -1), band).astype(case.dtype)
    elif case.regime != 'checker':
        band[band == null] = null + (1 if case.null == 'min' else -1)
    if case.layout != 'big':
        band[rng.rand(*band.shape) < 0.04] = null                   # scattered nodata
    if case.layout == 'blocks':
        band[seg == 6] = null                                         # one all-nodata segment
    if case.layout == 'chain':
        plant_chain(seg, band, 3, 3, 2)
    seg.setflags(write=False)
    band.setflags(write=False)
    return seg, band, null, S


_LIST = [
    Case('u8_full', 'blocks', 'uint8', 'full', maxds=(1, 5)),
    Case('i16_full', 'blocks', 'int16', 'full', maxds=(2, 5)),
    Case('u16_full', 'blocks', 'uint16', 'full', null='max', maxds=(5, 12)),
    Case('i32_narrow', 'blocks', 'int32', 'narrow', maxds=(1, 5, 12)),
    Case('u32_narrow', 'blocks', 'uint32', 'narrow', null='max', maxds=(5,)),
    Case('i32_mid', 'blocks', 'int32', 'mid', maxds=(1, 2, 5, 12)),
    Case('u32_mid', 'blocks', 'uint32', 'mid', maxds=(5, 64)),
    Case('i32_full', 'blocks', 'int32', 'full', maxds=(1, 5, 12, 255)),
    Case('u32_full', 'blocks', 'uint32', 'full', null='max', maxds=(2, 5, 64)),
    Case('i32_extreme_nullmin', 'blocks', 'int32', 'extreme', null='min', maxds=(1, 5)),
    Case('i32_extreme_nullmax', 'blocks', 'int32', 'extreme', null='max', maxds=(5,)),
    Case('u32_extreme_nullmin', 'blocks', 'uint32', 'extreme', null='min', maxds=(5,)),
    Case('u32_extreme_nullmax', 'blocks', 'uint32', 'extreme', null='max', maxds=(2, 5)),
    Case('i32_full_combs', 'combs', 'int32', 'full', maxds=(1, 5, 12)),
    Case('u32_mid_combs', 'combs', 'uint32', 'mid', null='max', maxds=(5, 64)),
    Case('u16_big', 'big', 'uint16', 'checker', null='max', maxds=(5,)),
    Case('u32_chain', 'chain', 'uint32', 'chain', null='max', maxds=(1, 5)),
]
CASES = {c.name: c for c in _LIST}
WIDE = tuple(c.name for c in _LIST if c.dtype.itemsize == 4 and c.regime != 'narrow')
NARROW = tuple(c.name for c in _LIST if c.name not in WIDE and c.layout != 'big')
BIG = ('u16_big',)
assert set(m for c in _LIST for m in c.maxds) == set(MAXDISTS)


def int_model_variogram(seg, band, null, maxd, S):
    """The device's variogram before the recompute, in numpy: per (segment, bin) a count and a wrapping uint64 sum
    of (d*d mod 2^64), then (float)sqrt(sum / count).  Returns (float32 (maxd, S + 1) with NaN where no pair,
    uint64 sums, counts)."""
    (nr, nc) = seg.shape
    v = band.astype(np.int64)
    valid = (seg != 0) & (seg <= S) & (v != null)
    sums = np.zeros((maxd, S + 1), dtype=np.uint64)
    cnts = np.zeros((maxd, S + 1), dtype=np.int64)
    for yo in range(1, min(maxd, nr - 1) + 1):
        for xo in range(1, min(maxd, nc - 1) + 1):
            b = int(np.sqrt(yo * yo + xo * xo))
            if b > maxd:
                continue
            a, q = (slice(0, nr - yo), slice(0, nc - xo)), (slice(yo, nr), slice(xo, nc))
            m = valid[a] & valid[q] & (seg[a] == seg[q])
            d = (v[a][m] - v[q][m]).astype(np.uint64)
            ids = seg[a][m].astype(np.int64)
            np.add.at(sums[b - 1], ids, d * d)
            np.add.at(cnts[b - 1], ids, 1)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = np.sqrt(sums.astype(np.float64) / cnts).astype(np.float32)
    return out, sums, cnts
