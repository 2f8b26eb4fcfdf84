"""CPU: the case lists of tests/prim_cases.py reach what they claim -- counted from the tile constants parsed out of
scan.h and sort.h -- and the numpy models give the answers written out here by hand."""
import itertools

import numpy as np

import prim_cases as pc


def test_constants_are_the_headers():
    assert pc.SCAN_ITEMS == pc.SCAN_SUB * pc.SCAN_STEPS
    assert pc.SORT_TILE == 4 * pc.SORT_ROWS * 64 and pc.SORT_TILE_WIDE == pc.SORT_WIDE * pc.SORT_TILE
    assert pc.SCAN_SUB % 4 == 0 and pc.HIST_BLOCKS * 256 == pc.SCAN_ITEMS
    # the sizes of today's constants, as the project's documents quote them
    if (pc.SCAN_SUB, pc.SCAN_STEPS, pc.SORT_ROWS, pc.SORT_WIDE) == (1024, 8, 8, 2):
        assert pc.SCAN_SIZES == (0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4099, 8191, 8192, 8193, 16384, 16385,
                                 3 * 8192 + 1021, 33 * 8192 + 7, 67108865)
        assert pc.SCAN_SKEW_SIZES == (1027, 8193 + 3)
        assert pc.SORT_SIZES == (0, 1, 2, 63, 64, 65, 511, 513, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 65537,
                                 2048 * 33 + 1, 131073, 200003)
        assert pc.SORT_BITS_SIZES == (2049, 65537)


def test_scan_cases_census():
    blocks = {pc.scan_blocks(c.n) for c in pc.SCAN_CASES}
    assert {1, 2} <= blocks
    assert any(2 < b <= pc.SCAN_ITEMS for b in blocks), 'no one-launch scan of more than two blocks'
    assert any(b > pc.SCAN_ITEMS for b in blocks), 'no scan whose block totals need a scan of their own'
    big = [c for c in pc.SCAN_CASES if pc.scan_blocks(c.n) > pc.SCAN_ITEMS]
    assert len(big) == 1 and 1 < pc.scan_blocks(pc.scan_blocks(big[0].n)) <= pc.SCAN_ITEMS      # the totals: one launch
    assert any(b > 32 for b in blocks if b <= pc.SCAN_ITEMS)       # many workgroups race for the last ticket
    assert any(0 < c.n < 4 for c in pc.SCAN_CASES) and any(c.n == 0 for c in pc.SCAN_CASES)
    assert any(c.n % 4 and pc.scan_blocks(c.n) > 1 for c in pc.SCAN_CASES)
    for edge in (pc.SCAN_SUB, pc.SCAN_ITEMS):
        assert {edge - 1, edge, edge + 1} <= {c.n for c in pc.SCAN_CASES}
    for n in pc.SCAN_SKEW_SIZES:
        pairs = {(c.skew_in, c.skew_out) for c in pc.SCAN_CASES if c.n == n and c.name.startswith('skew-')}
        assert pairs == set(itertools.product(range(4), range(4))), n
    assert pc.scan_blocks(pc.SCAN_SKEW_SIZES[0]) == 1 and pc.scan_blocks(pc.SCAN_SKEW_SIZES[1]) == 2
    # every content with aligned pointers (fast load and store) and with skewed ones (slow load and store), multi-block
    for content in pc.SCAN_CONTENTS:
        mine = [c for c in pc.SCAN_CASES if c.content == content and pc.scan_blocks(c.n) > 1]
        assert any(c.skew_in == 0 and c.skew_out == 0 for c in mine), content
        assert any(c.skew_in and c.skew_out for c in mine), content
    assert {(True, False), (False, False), (True, True), (False, True)} == set(pc.SCAN_FLAGS)
    one = {c.content: c.data() for c in pc.SCAN_CASES if c.content.startswith('one_')}
    assert [int(np.flatnonzero(one[k])[0]) for k in ('one_first', 'one_last', 'one_block2')] == \
        [0, pc.SCAN_CONTENT_N - 1, pc.SCAN_ITEMS]
    allbits = next(c for c in pc.SCAN_CASES if c.content == 'allbits').data()
    assert int(allbits.min()) == pc.M32                               # every partial sum wraps
    names = [c.name for c in pc.SCAN_CASES]
    assert len(set(names)) == len(names)
    assert {c.n for c in pc.SCAN_KNOB_CASES} == set(pc.SCAN_SIZES) - {pc.SCAN_BIG}


def test_sort_cases_census():
    cases = pc.SORT_CASES
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    nblk = {pc.sort_blocks(c.n) for c in cases}
    assert {1, pc.HIST_BLOCKS, pc.HIST_BLOCKS + 1} <= nblk
    assert pc.HIST_BLOCKS + 1 in {pc.sort_blocks(c.n, True) for c in cases if c.staged}
    assert pc.HIST_BLOCKS * 256 == pc.SCAN_ITEMS        # nblk HIST_BLOCKS + 1: the histogram's scan takes two blocks
    assert {c.passes for c in cases} == {1, 2, 3, 4}
    # every size at one pass and at four, random and run keys, both scatter forms
    for n in pc.SORT_SIZES:
        got = {(c.bits, c.content, c.staged) for c in pc.SORT_BY_SIZE if c.n == n}
        assert got == set(itertools.product((8, 32), ('random', 'runs65'), (False, True))), n
    # every width at the two sizes with every content, both scatter forms
    for n in pc.SORT_BITS_SIZES:
        for bits in pc.SORT_BITS:
            got = {(c.content, c.staged) for c in pc.SORT_BY_BITS if c.n == n and c.bits == bits}
            contents = pc.SORT_CONTENTS + (('random_high_bits',) if bits == 8 else ())
            assert got == set(itertools.product(contents, (False, True))), (n, bits)
    # values given or not x keys wanted or not: each combination meets every pass count in both scatter forms, and
    # sizes on both sides of the one-block and of the lazy-offset edge
    for sw in pc.SORT_SWITCHES:
        mine = [c for c in cases if (c.has_vals, c.want_keys) == sw]
        for staged in (False, True):
            assert {c.passes for c in mine if c.staged == staged} == {1, 2, 3, 4}, (sw, staged)
            blk = {pc.sort_blocks(c.n) for c in mine if c.staged == staged}
            assert 1 in blk and any(1 < b <= pc.HIST_BLOCKS for b in blk) and any(b > pc.HIST_BLOCKS for b in blk), sw
    # stability is observable: equal (masked) keys that carry different values
    seen = 0
    for c in cases:
        if c.n < 2 or c.content not in ('const', 'runs65', 'random'):
            continue
        keys, vals = c.keys(), c.vals()
        vals = np.arange(c.n) if vals is None else vals
        mask = np.uint32((1 << (8 * c.passes)) - 1)
        order = np.argsort(keys & mask, kind='stable')
        k, v = (keys & mask)[order], vals[order]
        seen += bool(((k[1:] == k[:-1]) & (v[1:] != v[:-1])).any())
    assert seen > 50
    # the ignored bits: keys with bits at or above 8 * passes set, which the sort must not look at
    high = [c for c in cases if c.content == 'random_high_bits']
    assert high and all(c.passes == 1 for c in high)
    for c in high:
        assert int(c.keys().max()) >> (8 * c.passes) != 0
    # bits between `bits` and the byte's end set: sorted on
    low = [c for c in cases if c.content == 'mod256' and c.bits < 8]
    assert low and all(int(c.keys().max()) >> c.bits != 0 for c in low)
    # every other content stays below 2^bits
    for c in cases:
        if c.content not in ('random_high_bits', 'mod256') and c.n:
            assert int(c.keys().max()) >> c.bits == 0, c.name
    assert pc.SORT_KNOB_CASES is pc.SORT_BY_SIZE


def test_scan_model_by_hand():
    out, total = pc.scan_model(np.array([1, 2, 3, 4], dtype=np.uint32))
    assert out.tolist() == [0, 1, 3, 6] and total == 10
    out, total = pc.scan_model(np.array([0xFFFFFFFF, 2, 0xFFFFFFFF], dtype=np.uint32))        # wraps twice
    assert out.dtype == np.uint32 and out.tolist() == [0, 0xFFFFFFFF, 1] and total == 0
    out, total = pc.scan_model(np.zeros(0, dtype=np.uint32))
    assert out.size == 0 and total == 0
    # the lazy form: the first block's items get boff[0], the two items of the second block boff[1]
    raw = np.r_[np.arange(pc.SCAN_ITEMS), [3, 0xFFFFFFFE]].astype(np.uint32)
    full = pc.scan_lazy_apply(raw, np.array([5, 7], dtype=np.uint32))
    assert full[:3].tolist() == [5, 6, 7] and full[-2:].tolist() == [10, 5] and full.dtype == np.uint32
    assert pc.scan_lazy_apply(raw[:4], None).tolist() == [0, 1, 2, 3]             # one block: no offsets, nothing added
    assert pc.scan_lazy_count(pc.SCAN_ITEMS) == 0 and pc.scan_lazy_count(pc.SCAN_ITEMS + 1) == 2


def test_sort_model_by_hand():
    keys = np.array([0x103, 0x002, 0x003, 0x101], dtype=np.uint32)
    vals = np.array([10, 20, 30, 40], dtype=np.uint32)
    # one pass: the low byte alone (3, 2, 3, 1); the two 3s keep their order; the keys come out whole
    kout, vout = pc.sort_model(keys, vals, 8)
    assert kout.tolist() == [0x101, 0x002, 0x103, 0x003] and vout.tolist() == [40, 20, 10, 30]
    kout, vout = pc.sort_model(keys, None, 8)
    assert vout.tolist() == [3, 1, 0, 2] and vout.dtype == np.uint32
    # nine bits are two passes: 16 bits decide
    kout, vout = pc.sort_model(keys, vals, 9)
    assert kout.tolist() == [0x002, 0x003, 0x101, 0x103] and vout.tolist() == [20, 30, 40, 10]
    # one bit asked for: the whole byte is sorted on, not bit 0 alone
    kout, vout = pc.sort_model(np.array([3, 2, 1, 0], dtype=np.uint32), None, 1)
    assert kout.tolist() == [0, 1, 2, 3] and vout.tolist() == [3, 2, 1, 0]
    assert [pc.sort_passes(b) for b in (0, 1, 8, 9, 16, 17, 24, 25, 32)] == [1, 1, 1, 2, 2, 3, 3, 4, 4]


def test_digit_starts_model_by_hand():
    starts = pc.digit_starts_model(np.array([0x101, 0x0FF, 0x001, 0x002], dtype=np.uint32))       # low bytes 1, 255, 1, 2
    assert starts.size == 257 and starts.dtype == np.uint32
    assert starts[:4].tolist() == [0, 0, 2, 3] and set(starts[3:256].tolist()) == {3} and starts[256] == 4
    assert pc.digit_starts_model(np.zeros(0, dtype=np.uint32)).tolist() == [0] * 257
