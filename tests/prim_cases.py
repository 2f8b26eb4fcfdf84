"""The cases of tests/test_gpu_primitives.py -- csrc/scan.h's scan_exclusive and csrc/sort.h's sort_pairs called on
their own through shp_prim_scan / shp_prim_sort -- with their numpy definitions.

Importable without a GPU: tests/test_prim_cases_host.py counts what the case lists reach, and tests/knob_cases.py
takes a fixed subset for the knob matrix.  Every edge below is derived from the tile constants parsed out of scan.h and
sort.h, so a change of a tile size moves the cases with it.  Everything is integer work: results are compared with
numpy.array_equal, no tolerance anywhere.

How the sort's cross product is cut (the full one is 20 sizes x 9 widths x 10 contents x 2 x 2 x 2):
 * SORT_BY_SIZE: every size at bits 8 and 32 (one pass and four) with random keys and with runs of 65 equal keys, in
   both scatter forms;
 * SORT_BY_BITS: every width at n = SORT_TILE + 1 and 32 * SORT_TILE + 1 (two blocks; the first size whose histogram
   scan hands lazy block offsets to the scatter) with every content, in both scatter forms;
 * the two remaining switches -- values given or NULL (the index), keys wanted or not -- rotate through their four
   combinations along each list, so every combination meets every pass count, both scatter forms and sizes on both
   sides of each block edge (test_prim_cases_host.py checks that); a kernel does not branch on (content x these
   switches) jointly, so their product with every content is left out;
 * sizes other than the two of SORT_BY_BITS at 2 and 3 passes: the passes are the same kernels with another shift, and
   the ping-pong choice depends on the pass count alone, which SORT_BY_BITS covers at both sizes.
"""
import ctypes
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pyshepseg_amd', 'csrc')


def _define(text, name):
    m = re.search(r'^#define\s+%s\s+(\d+)u?\b' % name, text, flags=re.M)
    assert m, 'no #define %s' % name
    return int(m.group(1))


def _constants():
    scan = open(os.path.join(CSRC, 'scan.h')).read()
    sort = open(os.path.join(CSRC, 'sort.h')).read()
    sub, steps, rows = _define(scan, 'SCAN_SUB'), _define(scan, 'SCAN_STEPS'), _define(sort, 'SORT_ROWS')
    assert re.search(r'#define\s+SCAN_ITEMS\s+\(SCAN_SUB \* SCAN_STEPS\)', scan)
    m = re.search(r'#define\s+SORT_TILE\s+\((\d+)u \* SORT_ROWS \* (\d+)u\)', sort)
    assert m, 'SORT_TILE is no longer waves * SORT_ROWS * lanes'
    wide = re.search(r'\(staged && wide\) \? (\d+)u \* SORT_TILE : SORT_TILE', sort)
    assert wide, 'the wide tile is no longer a multiple of SORT_TILE'
    return sub, steps, rows, int(m.group(1)) * rows * int(m.group(2)), int(wide.group(1))


SCAN_SUB, SCAN_STEPS, SORT_ROWS, SORT_TILE, SORT_WIDE = _constants()
SCAN_ITEMS = SCAN_SUB * SCAN_STEPS
SORT_TILE_WIDE = SORT_WIDE * SORT_TILE
HIST_BLOCKS = SCAN_ITEMS // 256         # sort blocks whose 256 * nblk histogram words still fit one scan block
M32 = 0xFFFFFFFF


def _seed(name):
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


_pool = {}
POOL_WORDS = 1 << 19


def random_words(n, which='keys'):
    """the first n of one fixed stream of uniform uint32 per purpose, drawn once per process (a longer one, which
    only the largest scan asks for, is drawn for that call alone)"""
    if n > POOL_WORDS:
        return np.random.RandomState(_seed(which) + 1).randint(0, 1 << 32, size=n, dtype=np.uint32)
    if which not in _pool:
        _pool[which] = np.random.RandomState(_seed(which)).randint(0, 1 << 32, size=POOL_WORDS, dtype=np.uint32)
    return _pool[which][:n]


# ---- scan ---------------------------------------------------------------------------------------------------------
def scan_model(a):
    """(out, total) of an exclusive prefix sum modulo 2^32"""
    a = np.asarray(a, dtype=np.uint32)
    c = np.cumsum(a, dtype=np.uint64)
    out = ((c - a) & M32).astype(np.uint32)
    return out, (int(c[-1]) & M32 if a.size else 0)


def scan_blocks(n):
    return -(-n // SCAN_ITEMS)


def scan_lazy_count(n):
    """block offsets a lazy scan hands back: one per block, none for a single block"""
    nb = scan_blocks(n)
    return nb if nb > 1 else 0


def scan_lazy_apply(out_raw, boff):
    """what a consumer of the lazy form computes: out_raw[i] + boff[i // SCAN_ITEMS] (boff None: absent)"""
    if boff is None:
        return out_raw
    n = out_raw.size
    assert boff.size == scan_blocks(n)
    return out_raw + np.repeat(boff, SCAN_ITEMS)[:n]          # uint32: wraps


SCAN_BIG = SCAN_ITEMS * SCAN_ITEMS + 1          # top level in plain-store form, its totals scanned in one launch
SCAN_SIZES = (0, 1, 3, 4, 5, 255, 256, 257, SCAN_SUB - 1, SCAN_SUB, SCAN_SUB + 1, 4 * SCAN_SUB + 3, SCAN_ITEMS - 1,
              SCAN_ITEMS, SCAN_ITEMS + 1, 2 * SCAN_ITEMS, 2 * SCAN_ITEMS + 1, 3 * SCAN_ITEMS + SCAN_SUB - 3,
              33 * SCAN_ITEMS + 7, SCAN_BIG)
SCAN_CONTENT_N = 3 * SCAN_ITEMS + SCAN_SUB - 3
SCAN_CONTENTS = ('zeros', 'ones', 'allbits', 'random', 'one_first', 'one_last', 'one_block2')
SCAN_SKEW_SIZES = (SCAN_SUB + 3, SCAN_ITEMS + 1 + 3)
SCAN_FLAGS = ((True, False), (False, False), (True, True), (False, True))       # (get4, lazy)


class ScanCase(object):
    def __init__(self, name, n, content, skew_in=0, skew_out=0):
        self.name, self.n, self.content, self.skew_in, self.skew_out = name, n, content, skew_in, skew_out

    def data(self):
        n = self.n
        if self.content == 'random':
            return random_words(n, 'scan')
        a = np.zeros(n, dtype=np.uint32)
        if self.content == 'ones':
            a[:] = 1
        elif self.content == 'allbits':
            a[:] = M32
        elif self.content == 'one_first':
            a[0] = 0x80000001
        elif self.content == 'one_last':
            a[n - 1] = 0x80000001
        elif self.content == 'one_block2':
            a[SCAN_ITEMS] = 0x80000001
        else:
            assert self.content == 'zeros', self.content
        return a


def _scan_cases():
    out = [ScanCase('size-%d' % n, n, 'random') for n in SCAN_SIZES]
    # each content with 16-byte aligned pointers (the fast load -- when the functor has get4 -- and the fast store) and
    # with skewed ones (4-byte loads and stores whatever the functor)
    for content in SCAN_CONTENTS:
        out.append(ScanCase('%s-aligned' % content, SCAN_CONTENT_N, content))
        out.append(ScanCase('%s-skewed' % content, SCAN_CONTENT_N, content, 1, 3))
    for n in SCAN_SKEW_SIZES:
        for si in range(4):
            for so in range(4):
                out.append(ScanCase('skew-%d-in%d-out%d' % (n, si, so), n, 'random', si, so))
    return out


SCAN_CASES = _scan_cases()
# the knob matrix's share: every size up to 33 blocks
SCAN_KNOB_CASES = [c for c in SCAN_CASES if c.name.startswith('size-') and c.n != SCAN_BIG]


# ---- sort ---------------------------------------------------------------------------------------------------------
def sort_passes(bits):
    return max(1, -(-bits // 8))


def sort_model(keys, vals, bits):
    """(keys_out, vals_out) of sort_pairs.  It sorts WHOLE BYTES: the key bits at and above 8 * passes are ignored,
    those between `bits` and the end of the last byte are NOT (a caller whose keys have such bits set gets them
    sorted on).  Stable; vals None means the values are the indices.  keys_out are the full keys, ignored bits
    included."""
    keys = np.asarray(keys, dtype=np.uint32)
    mask = np.uint32((1 << (8 * sort_passes(bits))) - 1)
    order = np.argsort(keys & mask, kind='stable')
    vals_out = order.astype(np.uint32) if vals is None else np.asarray(vals, dtype=np.uint32)[order]
    return keys[order], vals_out


def digit_starts_model(keys):
    """the 257 starts of a one-pass sort: starts[d] = count((keys & 255) < d), starts[256] = n"""
    cnt = np.bincount(np.asarray(keys, dtype=np.uint32) & np.uint32(255), minlength=256)
    return np.r_[0, np.cumsum(cnt)].astype(np.uint32)


def sort_blocks(n, staged_wide=False):
    return -(-n // (SORT_TILE_WIDE if staged_wide else SORT_TILE))


SORT_SIZES = (0, 1, 2, 63, 64, 65, 511, 513, SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, SORT_TILE_WIDE - 1,
              SORT_TILE_WIDE, SORT_TILE_WIDE + 1, HIST_BLOCKS * SORT_TILE - 1, HIST_BLOCKS * SORT_TILE,
              HIST_BLOCKS * SORT_TILE + 1, (HIST_BLOCKS + 1) * SORT_TILE + 1, HIST_BLOCKS * SORT_TILE_WIDE + 1, 200003)
SORT_BITS = (1, 7, 8, 9, 16, 17, 24, 25, 32)
SORT_BITS_SIZES = (SORT_TILE + 1, HIST_BLOCKS * SORT_TILE + 1)
SORT_CONTENTS = ('const', 'alternate', 'mod256', 'runs64', 'runs65', 'runs2048', 'descending', 'random')
SORT_SWITCHES = ((True, True), (False, True), (True, False), (False, False))        # (values given, keys wanted)


class SortCase(object):
    def __init__(self, n, bits, content, staged, has_vals, want_keys):
        self.n, self.bits, self.content, self.staged = n, bits, content, staged
        self.has_vals, self.want_keys = has_vals, want_keys
        self.name = 'n%d-b%d-%s-%s-%s%s' % (n, bits, content, 'staged' if staged else 'direct',
                                            'v' if has_vals else 'i', 'k' if want_keys else '')

    @property
    def passes(self):
        return sort_passes(self.bits)

    def keys(self):
        n, bits = self.n, self.bits
        below = np.uint32((1 << bits) - 1)
        i = np.arange(n, dtype=np.uint64)
        if self.content == 'const':
            return np.full(n, 0xC3A5F00F, dtype=np.uint32) & below
        if self.content == 'alternate':
            return np.where(i % 2 == 1, below, below >> np.uint32(1)).astype(np.uint32)
        if self.content == 'mod256':
            # 64 different digits in every wavefront row, in every pass; below 8 bits the key still fills its byte:
            # bits between `bits` and the byte's end are sorted on
            return ((i % 256) * 0x01010101).astype(np.uint32) & np.uint32((1 << (8 * self.passes)) - 1)
        if self.content.startswith('runs'):
            # what labels look like: runs of equal keys, the same key coming back in later runs
            run = i // int(self.content[4:])
            return (((run * 2654435761) >> np.uint64(7)) & np.uint64(below)).astype(np.uint32)
        if self.content == 'descending':
            return (i[::-1] & np.uint64(below)).astype(np.uint32)
        if self.content == 'random':
            return random_words(n) >> np.uint32(32 - bits)
        assert self.content == 'random_high_bits' and bits == 8
        return random_words(n).copy()           # all 32 bits set at random: those above the byte are ignored

    def vals(self):
        """random with repeats, or None (the index)"""
        if not self.has_vals:
            return None
        return random_words(self.n, 'vals') % np.uint32(max(1, self.n // 3))


def _sort_cases(sizes, bits_list, contents, taken=()):
    """the product of its arguments and the two scatter forms; the switches rotate, and take another turn where a
    case of `taken` has the same combination already"""
    out, names = [], {c.name for c in taken}
    for n in sizes:
        for bits in bits_list:
            for content in contents + (('random_high_bits',) if bits == 8 and len(contents) > 2 else ()):
                for staged in (False, True):
                    turn = len(out) // 2 + len(out) // 8
                    case = SortCase(n, bits, content, staged, *SORT_SWITCHES[turn % 4])
                    while case.name in names:
                        turn += 1
                        case = SortCase(n, bits, content, staged, *SORT_SWITCHES[turn % 4])
                    out.append(case)
    return out


SORT_BY_SIZE = _sort_cases(SORT_SIZES, (8, 32), ('random', 'runs65'))
SORT_BY_BITS = _sort_cases(SORT_BITS_SIZES, SORT_BITS, SORT_CONTENTS, SORT_BY_SIZE)
SORT_CASES = SORT_BY_SIZE + SORT_BY_BITS
SORT_KNOB_CASES = SORT_BY_SIZE          # the knob matrix's share: every size, random and run keys, both scatter forms


# ---- the GPU side (only called where there is one) -------------------------------------------------------------------
GUARD = 8               # words around every output the library writes: they must keep their filler
FILL_BYTE = 0xEE
FILL_WORD = 0xEEEEEEEE
SHP_ERR_NOMEM = -4


class AllocRefused(Exception):
    """shp_dev_alloc said SHP_ERR_NOMEM"""


class Dev(object):
    """named grow-only device buffers in the calling thread's context, and the two entry points"""

    def __init__(self):
        from pyshepseg_amd import _lib
        self.c = _lib.ctx()
        self.L = self.c._L
        self.bufs = {}

    def buf(self, name, words):
        have = self.bufs.get(name)
        if have is not None and have[1] >= words:
            return have[0]
        if have is not None:
            del self.bufs[name]
            self.c.check(self.L.shp_dev_free(self.c.handle, have[0]))
        p = ctypes.c_void_p()
        rc = self.L.shp_dev_alloc(self.c.handle, max(words, 4) * 4, ctypes.byref(p))
        if rc == SHP_ERR_NOMEM:
            raise AllocRefused('%s: %d words' % (name, words))
        self.c.check(rc)
        self.bufs[name] = (p.value, words)
        return p.value

    def release(self, name):
        have = self.bufs.pop(name, None)
        if have is not None:
            self.c.check(self.L.shp_dev_free(self.c.handle, have[0]))

    def close(self):
        for name in list(self.bufs):
            self.release(name)

    def upload(self, name, a, skew=0):
        """a at word `skew` of the buffer (whose start is 256-byte aligned); returns the device address"""
        a = np.ascontiguousarray(a, dtype=np.uint32)
        p = self.buf(name, a.size + skew + 4) + 4 * skew
        if a.size:
            self.c.check(self.L.shp_dev_upload(self.c.handle, p, a.ctypes.data_as(ctypes.c_void_p), a.size * 4))
        return p

    def guarded(self, name, n, skew=0):
        """room for n words at word GUARD + skew of a buffer filled with FILL_WORD; returns the device address"""
        words = n + 2 * GUARD + 4
        base = self.buf(name, words)
        self.c.check(self.L.shp_dev_memset(self.c.handle, base, FILL_BYTE, words * 4))
        return base + 4 * (GUARD + skew)

    def fetch(self, name, n, skew=0):
        """the n words guarded() made room for, and whether the words around them kept their filler"""
        words = n + 2 * GUARD + 4
        a = np.empty(words, dtype=np.uint32)
        self.c.check(self.L.shp_dev_download(self.c.handle, a.ctypes.data_as(ctypes.c_void_p), self.bufs[name][0],
                                             words * 4))
        lo = GUARD + skew
        clean = bool((a[:lo] == FILL_WORD).all() and (a[lo + n:] == FILL_WORD).all())
        return a[lo:lo + n], clean

    def scan(self, d_in, n, get4, lazy, skew_out=0, out='scan_out'):
        """one shp_prim_scan of the n words at d_in -> dict(out_raw, boff or None, nboff, total_dev, total_mirror,
        clean, d_out)"""
        nb = scan_blocks(n)
        d_out = self.guarded(out, n, skew_out)
        d_boff = self.guarded('scan_boff', nb) if lazy else None
        tot, mir, nboff = ctypes.c_uint32(0x12345678), ctypes.c_uint32(0x12345678), ctypes.c_uint32(0x12345678)
        self.c.check(self.L.shp_prim_scan(self.c.handle, d_in, n, d_out, (0 if get4 else 1) | (2 if lazy else 0),
                                          ctypes.byref(tot), ctypes.byref(mir), d_boff,
                                          ctypes.byref(nboff) if lazy else None))
        raw, clean = self.fetch(out, n, skew_out)
        boff = None
        if lazy:
            b, bclean = self.fetch('scan_boff', nb)
            clean = clean and bclean and bool((b[nboff.value:] == FILL_WORD).all())
            boff = b[:nboff.value] if nboff.value else None
        return {'out_raw': raw, 'boff': boff, 'nboff': nboff.value if lazy else 0, 'total_dev': tot.value,
                'total_mirror': mir.value, 'clean': clean, 'd_out': d_out}

    def sort(self, keys, vals, bits, staged, want_keys, want_starts=True):
        """one shp_prim_sort -> dict(keys_out or None, vals_out, starts or None, clean)"""
        n = keys.size
        d_keys = self.upload('sort_keys', keys)
        d_vals = self.upload('sort_vals', vals) if vals is not None else None
        d_kout = self.guarded('sort_kout', n) if want_keys else None
        d_vout = self.guarded('sort_vout', n)
        starts = np.full(257, 0x12345678, dtype=np.uint32)
        self.c.check(self.L.shp_prim_sort(self.c.handle, d_keys, d_vals, n, bits, 1 if staged else 0, d_kout, d_vout,
                                          starts.ctypes.data_as(ctypes.c_void_p) if want_starts else None))
        vout, clean = self.fetch('sort_vout', n)
        kout = None
        if want_keys:
            kout, kclean = self.fetch('sort_kout', n)
            clean = clean and kclean
        return {'keys_out': kout, 'vals_out': vout, 'clean': clean,
                'starts': starts if want_starts and sort_passes(bits) == 1 else None}


def first_diff(got, want):
    """'' when equal, else where two arrays first differ"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return 'shape %s, expected %s' % (got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return ''
    i = int(bad[0])
    return 'first difference at index %d of %d (%d differ): got %d, expected %d' % (i, got.size, bad.size, got[i], want[i])


# ---- the knob matrix's two cases (tests/knob_cases.py) -----------------------------------------------------------------
def knob_scan_run():
    dev = Dev()
    out = {}
    try:
        for case in SCAN_KNOB_CASES:
            d_in = dev.upload('scan_in', case.data())
            for get4, lazy in SCAN_FLAGS:
                r = dev.scan(d_in, case.n, get4, lazy)
                key = '%s/get4_%d/lazy_%d' % (case.name, get4, lazy)
                out[key + '/out'] = scan_lazy_apply(r['out_raw'], r['boff'])
                out[key + '/totals'] = np.array([r['total_dev'], r['total_mirror'], r['nboff'], r['clean']], dtype=np.uint32)
    finally:
        dev.close()
    return out


def knob_scan_expected():
    out = {}
    for case in SCAN_KNOB_CASES:
        want, total = scan_model(case.data())
        for get4, lazy in SCAN_FLAGS:
            key = '%s/get4_%d/lazy_%d' % (case.name, get4, lazy)
            out[key + '/out'] = want
            out[key + '/totals'] = np.array([total, total, scan_lazy_count(case.n) if lazy else 0, 1], dtype=np.uint32)
    return out


def knob_sort_run():
    dev = Dev()
    out = {}
    try:
        for case in SORT_KNOB_CASES:
            r = dev.sort(case.keys(), case.vals(), case.bits, case.staged, case.want_keys)
            out[case.name + '/vals'] = r['vals_out']
            out[case.name + '/clean'] = np.array([r['clean']], dtype=np.uint32)
            if case.want_keys:
                out[case.name + '/keys'] = r['keys_out']
            if case.passes == 1:
                out[case.name + '/starts'] = r['starts']
    finally:
        dev.close()
    return out


def knob_sort_expected():
    out = {}
    for case in SORT_KNOB_CASES:
        keys = case.keys()
        kout, vout = sort_model(keys, case.vals(), case.bits)
        out[case.name + '/vals'] = vout
        out[case.name + '/clean'] = np.array([1], dtype=np.uint32)
        if case.want_keys:
            out[case.name + '/keys'] = kout
        if case.passes == 1:
            out[case.name + '/starts'] = digit_starts_model(keys)
    return out
