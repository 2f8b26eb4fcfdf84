"""Deterministic (seg, img, max_seg_id) generators for the per-segment tables: spectral sums
(buildSegmentSpectra), segment locations and sizes.  Imports neither the GPU nor the library.

A case is a segment raster plus a rule for the pixel values.  `make(case, dtype, nb)` returns
(seg, img, max_seg_id): seg is a uint32 (rows, cols) raster, img (nb, rows, cols) of `dtype`.  The
values of band b come from a stream seeded by (case, dtype, b), so two calls give the same arrays.

Value regimes (what the spectra kernels do with them):
  full       uniform over the dtype's whole range, the extremes planted: small segments stay exact,
             large ones cross the 2^24 bound early (at once for 32-bit types)
  exact      |v| <= 3: every sum stays an exact integer, whatever the segment size
  high       the top half of the dtype's range: past the bound every float32 add rounds
  altsign    +A, -A alternating in raster order (A = 30000 or 2^30): sum(|v|) crosses 2^24 while
             the sum itself stays small (signed types only)
  const:V    every pixel V (the bound crossed at a computable pixel)
  ramp:N:V   1 for the first N pixels of the raster, then V
  split      band 0 exact (<= 3), the other bands high: the cross-band bound is conservative
"""
import functools

import numpy as np

DTYPES = ('uint8', 'int16', 'uint16', 'int32', 'uint32')
ALL_NB = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17)
LIM = 1 << 24                         # float32 sums of integers are exact below this
SPECTRA_GRID_SLOTS = 4 * 4096         # k_spectra_big: 4 wavefronts x SPECTRA_GRID workgroups
RUN_POS_BITS = 26                     # csr.h: a run's start index is stored in 26 bits


class Case:
    def __init__(self, name, purpose, segfn, regime='full', dtypes=DTYPES, nbs=ALL_NB, extra_ids=0):
        self.name, self.purpose, self.segfn, self.regime = name, purpose, segfn, regime
        self.dtypes, self.nbs, self.extra_ids = tuple(dtypes), tuple(nbs), extra_ids

    def seg(self):
        """(seg, max_seg_id): max_seg_id = the largest id present + extra_ids"""
        seg = _seg_cached(self.name)
        return seg, int(seg.max()) + self.extra_ids

    def __repr__(self):
        return self.name


def bits_for(maxval):
    """sort.h bits_for: significant bits of the largest key (at least 1)"""
    return max(1, int(maxval).bit_length())


def radix_passes(max_seg_id):
    """passes of the radix sort that groups pixels (or runs) by segment id: ceil(bits_for(S) / 8)"""
    return (bits_for(max_seg_id) + 7) // 8


# ---- segment rasters ------------------------------------------------------------------------------

def _linear(sizes, shape, seed, ids=None):
    """segments laid out as consecutive ranges of linear pixel indices (so a segment is a run of whole
    and partial rows), ids shuffled so that raster order and id order differ; the rest null (0)"""
    sizes = np.asarray(sizes, dtype=np.int64)
    if isinstance(shape, int):                  # a width: as many rows as the segments need, plus one
        shape = (int(sizes.sum()) // shape + 2, shape)
    n = int(np.prod(shape))
    assert sizes.sum() <= n, (sizes.sum(), n)
    if ids is None:
        ids = np.random.RandomState(seed).permutation(len(sizes)) + 1
    seg = np.zeros(n, dtype=np.uint32)
    seg[:sizes.sum()] = np.repeat(np.asarray(ids, dtype=np.uint32), sizes)
    return seg.reshape(shape)


SIZES = (1, 2, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4096, 10007)


def _sizes():
    # every size three times, width 97: runs cut at row ends and at multiples of 64
    return _linear(np.repeat(SIZES, 3), 97, 1)


def _steps():
    # past the bound the ordered phase walks 64-pixel steps from a multiple of 512: a last step that is full,
    # a multiple of 8, or neither.  'high' values of 16- and 32-bit types cross the bound in the first or
    # second 512-pixel chunk; uint8 ones (127..255) would need ~85 000 pixels and stay exact here -- the
    # uint8 step shapes come from u8_255 (131 072, 70 000 and 65 794 pixels past a crossing at 65 794)
    return _linear((4096, 4160, 4136, 4133, 1090, 1027, 600, 577), 101, 2)


def _crossing():
    # one segment per crossing pattern (regime const / ramp decides where the bound falls)
    return _linear((300, 1024, 1100, 5000, 20000), 137, 3)


def _u8_crossing():
    # 255 * 65794 >= 2^24: a 70 000-pixel uint8 segment crosses after 65 794 pixels, a 131 072 one far past
    return _linear((70000, 131072, 65794, 65793, 100), 523, 4)


def _rounding():
    # every add past the bound rounds: a 10^4 and a ~10^6-pixel segment, plus small ones around them
    sizes = [10000, 1000003] + [65, 64, 9] * 10
    return _linear(sizes, 997, 5)


def _ids_257():
    # S = 257 (9 bits: 2 radix passes); ids 100..149 never occur; max_seg_id 5 above the largest id
    rng = np.random.RandomState(6)
    ids = np.array([i for i in range(1, 258) if not 100 <= i < 150])
    sizes = rng.randint(1, 140, size=len(ids))
    return _linear(sizes, 211, 6, ids=rng.permutation(ids))


def _ids_4097():
    # S = 4097 (13 bits): k_big_seg_list's second 4096-id block (first = 0) holds ids 4096 and 4097; 4097 is
    # big (300 pixels), 4096 big or small as drawn
    rng = np.random.RandomState(7)
    sizes = np.where(rng.rand(4097) < 0.3, rng.randint(65, 130, size=4097), rng.randint(1, 65, size=4097))
    sizes[-1] = 300
    return _linear(sizes, 439, 7, ids=np.arange(1, 4098))


def _ids_65537():
    # S = 65 537 (17 bits: 3 radix passes), id order unrelated to raster order, zeros scattered
    rng = np.random.RandomState(8)
    sizes = rng.randint(1, 12, size=65537)
    sizes[rng.randint(0, 65537, size=200)] = 200
    seg = _linear(sizes, 457, 8)
    seg[rng.rand(*seg.shape) < 0.01] = 0
    return seg


def _ids_sparse_2p24():
    # S = 2^24 + 3 (25 bits: 4 radix passes) on 64 x 67 pixels: ids spread over the whole space, most ids
    # without pixels, a 100-pixel segment at the very top id and one at id 1
    rng = np.random.RandomState(9)
    top = LIM + 3
    ids = np.unique(rng.randint(2, top - 1, size=900))
    seg = np.repeat(ids, 4).astype(np.uint32)
    seg = np.concatenate([np.full(100, top, np.uint32), seg, np.full(100, 1, np.uint32)])
    seg = seg[:64 * 67]
    out = np.zeros(64 * 67, dtype=np.uint32)
    out[:seg.size] = seg
    return out.reshape(64, 67)


def _null_big():
    # a 150 000-pixel null segment 0 around segments of all sizes
    seg = np.zeros((400, 517), dtype=np.uint32)
    inner = _linear(np.repeat((1, 5, 64, 65, 700, 3000), 8), (100, 517), 10)
    seg[150:250] = inner
    return seg


def _many_big():
    # 20 000 segments of 65..100 pixels: more than the 16 384 wavefront slots of k_spectra_big's grid,
    # so its round-robin wraps; plus a few small ones
    rng = np.random.RandomState(11)
    sizes = np.concatenate([rng.randint(65, 101, size=20000), rng.randint(1, 65, size=500)])
    return _linear(sizes, 1001, 11)


def _row_1xn():
    rng = np.random.RandomState(12)
    return _linear(rng.randint(1, 3000, size=60), (1, 100003), 12)


def _col_nx1():
    rng = np.random.RandomState(13)
    return _linear(rng.randint(1, 3000, size=40), 1, 13)


def _odd_shape():
    # n = 333 * 331 = 110 223: not a multiple of 4, 64 or 4096
    rng = np.random.RandomState(14)
    return _linear(rng.randint(1, 800, size=250), (333, 331), 14)


def _long_rows():
    # every row one id (rows of 1000 pixels: runs cut at multiples of 64), ids repeating every 37 rows
    r = np.arange(300, dtype=np.uint32)
    return np.repeat((r % 37 + 1)[:, None], 1000, axis=1)


def _checker():
    # every run one pixel long: 32 x 32 blocks, two ids per block on the checkerboard (512 pixels each)
    yy, xx = np.mgrid[0:320, 0:352]
    blk = (yy // 32) * 11 + xx // 32
    return (1 + 2 * blk + (yy + xx) % 2).astype(np.uint32)


CASES = [
    Case('sizes', 'segments of 1..10007 pixels, each size three times, full-range values', _sizes),
    Case('sizes_exact', 'the same segments with |v| <= 3: every sum exact', _sizes, 'exact'),
    Case('steps', 'past the bound, last 64-pixel step full / a multiple of 8 / neither', _steps, 'high'),
    Case('cross_first', '65535 everywhere: the bound crossed inside the first 512-pixel chunk', _crossing,
         'const:65535', dtypes=('uint16',)),
    Case('cross_boundary', '16384 everywhere: sum(|v|) reaches 2^24 exactly at pixel 1024, a chunk boundary',
         _crossing, 'const:16384', dtypes=('uint16',)),
    Case('cross_below', '16383 everywhere: the bound crossed inside the third chunk', _crossing,
         'const:16383', dtypes=('uint16',)),
    Case('cross_late', '1 for 2000 pixels, then 65535: the bound crossed several chunks in', _crossing,
         'ramp:2000:65535', dtypes=('uint16',)),
    Case('u8_255', 'uint8 255 everywhere: crosses after 65 794 pixels', _u8_crossing, 'const:255',
         dtypes=('uint8',), nbs=(1, 2, 8, 9)),
    Case('altsign', '+A, -A alternating: sum(|v|) crosses 2^24, the sum stays small', _crossing, 'altsign',
         dtypes=('int16', 'int32')),
    Case('split_bands', 'band 0 exact, the other bands high (the cross-band bound)', _steps, 'split',
         nbs=(2, 3, 8, 9, 17)),
    Case('rounding', 'top-half values on 10^4 and 10^6-pixel segments: every add rounds', _rounding, 'high',
         nbs=(1, 2, 8, 9)),
    Case('full32', 'full-range 32-bit values incl. 0xFFFFFFFF and -2^31 on every size', _sizes, 'full',
         dtypes=('int32', 'uint32')),
    Case('ids_257', 'S = 257, ids without pixels, max_seg_id above the largest id', _ids_257, extra_ids=5),
    Case('ids_4097', 'S = 4097: two blocks of k_big_seg_list', _ids_4097),
    Case('ids_65537', 'S = 65 537: 3 radix passes, scattered null pixels', _ids_65537),
    Case('ids_sparse_2p24', 'S = 2^24 + 3 on 4288 pixels: 4 radix passes, a big segment at the top id',
         _ids_sparse_2p24, nbs=(1, 2)),
    Case('null_big', 'a 150 000-pixel null segment 0 (k_spectra_big with first = 0)', _null_big),
    Case('many_big', '20 000 segments of 65..100 pixels: k_spectra_big round-robin wraps', _many_big,
         nbs=(1, 2, 5, 8, 9, 17)),
    Case('row_1xn', '1 x 100 003 raster', _row_1xn),
    Case('col_nx1', 'N x 1 raster (60 472 rows)', _col_nx1),
    Case('odd_shape', '333 x 331: n not a multiple of 4, 64 or 4096', _odd_shape),
    Case('long_rows', 'rows of one id, 1000 pixels wide: runs cut at multiples of 64', _long_rows),
    Case('checker', 'checkerboard: every run one pixel long', _checker),
]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=4)
def _seg_cached(name):
    seg = np.ascontiguousarray(BY_NAME[name].segfn(), dtype=np.uint32)
    seg.setflags(write=False)
    return seg


# ---- pixel values ---------------------------------------------------------------------------------

def hash_str(s):
    """FNV-1a: a seed from a string that does not depend on Python's hash randomisation"""
    h = 2166136261
    for ch in s.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def band_values(regime, dtype, n, band, seed):
    """the n values of one band, raster order, as int64"""
    info = np.iinfo(dtype)
    lo, hi = int(info.min), int(info.max)
    rng = np.random.RandomState(seed & 0xFFFFFFFF)
    if regime == 'split':
        regime = 'exact' if band == 0 else 'high'
    if regime == 'full':
        v = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.int64) % (hi - lo + 1) + lo
        v[::997] = hi
        v[498::997] = lo
        return v
    if regime == 'exact':
        return rng.randint(max(lo, -3), 4, size=n).astype(np.int64)
    if regime == 'high':
        half = hi // 2
        return rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.int64) % (hi - half + 1) + half
    if regime == 'altsign':
        a = 30000 if hi < (1 << 16) else (1 << 30)
        v = np.full(n, a, dtype=np.int64)
        v[1::2] = -a
        return v if band % 2 == 0 else -v
    if regime.startswith('const:'):
        return np.full(n, int(regime.split(':')[1]), dtype=np.int64)
    if regime.startswith('ramp:'):
        (_r, k, val) = regime.split(':')
        v = np.full(n, int(val), dtype=np.int64)
        v[:int(k)] = 1
        return v
    raise KeyError(regime)


def make(case, dtype, nb):
    """(seg, img, max_seg_id) of a case at one pixel type and band count"""
    if isinstance(case, str):
        case = BY_NAME[case]
    dtype = np.dtype(dtype)
    seg, S = case.seg()
    img = np.empty((nb,) + seg.shape, dtype=dtype)
    for b in range(nb):
        img[b].ravel()[:] = band_values(case.regime, dtype, seg.size, b,
                                        hash_str('%s/%s/%d' % (case.name, dtype.name, b)))
    return seg, img, S


def int_sums(seg, img, max_seg_id):
    """exact per-segment sums and sums of |v| (int64, (max_seg_id + 1, nb)) by a stable sort and reduceat"""
    nb = img.shape[0]
    flat = seg.ravel()
    order = np.argsort(flat, kind='stable')
    ids = flat[order]
    starts = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
    present = ids[starts]
    tot = np.zeros((max_seg_id + 1, nb), dtype=np.int64)
    absum = np.zeros((max_seg_id + 1, nb), dtype=np.int64)
    for b in range(nb):
        v = img[b].ravel().astype(np.int64)[order]
        tot[present, b] = np.add.reduceat(v, starts)
        absum[present, b] = np.add.reduceat(np.abs(v), starts)
    return tot, absum


def restated_spectra(seg, img, max_seg_id):
    """buildSegmentSpectra restated with numpy: float32 accumulators, unbuffered adds in raster order
    (np.add.at), each add the float32 rounding of float32 + float64(pixel)"""
    nb = img.shape[0]
    out = np.zeros((max_seg_id + 1, nb), dtype=np.float32)
    flat = seg.ravel()
    for b in range(nb):
        acc = np.zeros(max_seg_id + 1, dtype=np.float32)
        np.add.at(acc, flat, img[b].ravel().astype(np.float64))
        out[:, b] = acc
    return out
