"""CPU: pyshepseg_amd.labelsource, the label raster under the per-segment calls -- what ``segfile`` may be and how it is
refused, the row-block plan, and LabelSource and mapBlocks against a context whose "device" is host memory: the fake
library's alloc, upload, download and free record their calls, so every byte that would cross to the GPU is looked at.
No GPU and no library are needed."""
import ctypes

import numpy as np
import pytest

from test_shapes_host import REFUSALS

NROWS, NCOLS, BLOCK = 33, 65, 11
SHAPES = [(0, 5, None), (5, 0, None), (1, 1, 1), (33, 65, 11 * 65), (33, 65, 64), (33, 65, 33 * 65), (33, 65, 10 ** 12), (7, 3, 0)]
GENERIC = "segfile must be a 2-D uint32 array, a .npy path of one, or a segmentation result kept on the device"


class Refused(Exception):
    pass


def labels_of(seg=None, devSeg=None, shape=None):
    from pyshepseg_amd import labelsource
    (nrows, ncols) = seg.shape if shape is None else shape
    return labelsource.Labels(seg, devSeg, nrows, ncols, None)


def raster():
    return np.random.default_rng(5).integers(0, 2 ** 32 - 2, size=(NROWS, NCOLS), dtype=np.uint32)


class FakeLib(object):
    """device memory is host memory: {address: buffer} of what is allocated, and the calls in order"""
    def __init__(self):
        self.live = {}
        self.allocated = []
        self.freed = []
        self.uploads = []       # (device address, the bytes)
        self.downloads = 0

    def _room(self, address, nbytes):
        """the allocation that holds [address, address + nbytes)"""
        for (base, buf) in self.live.items():
            if base <= address and address + nbytes <= base + len(buf):
                return (base, len(buf))
        raise AssertionError('%d bytes at %d lie in no live allocation' % (nbytes, address))

    def shp_dev_alloc(self, handle, nbytes, ref):
        buf = ctypes.create_string_buffer(nbytes)
        self.live[ctypes.addressof(buf)] = buf
        self.allocated.append(ctypes.addressof(buf))
        ref._obj.value = ctypes.addressof(buf)
        return 0

    def shp_dev_free(self, handle, p):
        del self.live[p.value]          # (a second free of one address is a KeyError)
        self.freed.append(p.value)
        return 0

    def shp_dev_upload(self, handle, dst, src, nbytes):
        self._room(dst.value, nbytes)
        ctypes.memmove(dst, src, nbytes)
        self.uploads.append((dst.value, ctypes.string_at(dst.value, nbytes)))
        return 0

    def shp_dev_download(self, handle, dst, src, nbytes):
        self._room(src.value, nbytes)
        ctypes.memmove(dst, src, nbytes)
        self.downloads += 1
        return 0

    def shp_shape_label_max_dev(self, handle, dseg, n, top, ms):
        self.maxCalls = getattr(self, 'maxCalls', 0) + 1
        top._obj.value = int(np.frombuffer(ctypes.string_at(dseg.value, 4 * n), dtype=np.uint32).max())
        ms._obj.value = 0.25
        return 0


class FakeCtx(object):
    def __init__(self):
        self._L = FakeLib()
        self.handle = ctypes.c_void_p(1)

    def check(self, rc):
        assert rc == 0


# ---- rowBlocks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('above', [False, True])
@pytest.mark.parametrize('below', [False, True])
@pytest.mark.parametrize('shape', SHAPES)
def test_row_blocks(shape, above, below):
    from pyshepseg_amd import labelsource, tilingstats
    (nrows, ncols, chunkPixels) = shape
    plan = labelsource.rowBlocks(nrows, ncols, chunkPixels, above=above, below=below)
    if nrows == 0 or ncols == 0:
        assert plan == []
        return
    pixels = tilingstats.STATS_CHUNK_PIXELS if chunkPixels is None else chunkPixels
    height = max(1, min(max(nrows, 1), pixels // max(ncols, 1)))
    assert plan[0][0] == 0 and plan[-1][1] == nrows
    assert all(a[1] == b[0] for (a, b) in zip(plan, plan[1:]))             # in order, no gap, no overlap
    assert all(y1 - y0 == height for (y0, y1, _a, _b) in plan[:-1]) and 0 < plan[-1][1] - plan[-1][0] <= height
    for (y0, y1, hasAbove, hasBelow) in plan:
        assert hasAbove is (above and y0 > 0) and hasBelow is (below and y1 < nrows)


def test_row_blocks_of_the_gpu_tests():
    from pyshepseg_amd import labelsource
    assert labelsource.rowBlocks(NROWS, NCOLS, BLOCK * NCOLS, above=True, below=True) == [
        (0, 11, False, True), (11, 22, True, True), (22, 33, True, False)]
    assert labelsource.rowBlocks(7, 3, 0) == [(y, y + 1, False, False) for y in range(7)]


# ---- resolve ----------------------------------------------------------------------------------------------------------
class Resident(object):
    def __init__(self, maxSegId=None):
        self.outDev = (4096, 7, 9, 7 * 9 * 4)
        self.maxSegId = maxSegId


def test_resolve_accepts(tmp_path):
    from pyshepseg_amd import labelsource, neighbours, tiling
    seg = raster()
    r = labelsource.resolve(seg, None, Refused)
    assert r.seg is seg and r[1:] == (None, NROWS, NCOLS, None)
    assert labelsource.resolve(seg, np.int64(12), Refused).maxSegId == 12
    path = str(tmp_path / 'labels.npy')
    np.save(path, seg)
    r = labelsource.resolve(path, 3, Refused)
    assert isinstance(r.seg, np.memmap) and np.array_equal(r.seg, seg) and r[1:] == (None, NROWS, NCOLS, 3)
    tiled = tiling.TiledSegmentationResult()
    (tiled.segimg, tiled.maxSegId) = (seg, 41)
    r = labelsource.resolve(tiled, None, Refused, hint=True)
    assert r.seg is seg and r[1:] == (None, NROWS, NCOLS, 41)
    assert labelsource.resolve(tiled, 40, Refused, hint=True).maxSegId == 40        # a given maxSegId wins
    assert labelsource.resolve(Resident(), 5, Refused) == (None, 4096, 7, 9, 5)
    assert labelsource.resolve(Resident(8), None, Refused, hint=True) == (None, 4096, 7, 9, 8)
    merged = neighbours.MergedSegments()
    (merged.segimg, merged.maxSegId) = (seg, 6)
    r = labelsource.resolve(merged, None, Refused, merged=True, hint=True)
    assert r.seg is seg and r[1:] == (None, NROWS, NCOLS, 6)
    merged.outDev = (8192, 3, 4, 48)
    assert labelsource.resolve(merged, None, Refused, merged=True, hint=True) == (None, 8192, 3, 4, 6)
    assert labelsource.resolve(merged, None, Refused) == (None, 8192, 3, 4, None)      # outDev needs no rule


def test_resolve_without_hint_ignores_the_objects_maxsegid():
    from pyshepseg_amd import labelsource, tiling
    tiled = tiling.TiledSegmentationResult()
    (tiled.segimg, tiled.maxSegId) = (raster(), 41)
    assert labelsource.resolve(tiled, None, Refused).maxSegId is None
    assert labelsource.resolve(Resident(8), None, Refused).maxSegId is None
    tiled.maxSegId = -1
    with pytest.raises(Refused, match=r"^maxSegId must be a non-negative integer \(got -1\)$"):
        labelsource.resolve(tiled, None, Refused, hint=True)


TEXTS = {'float labels': GENERIC, 'int32 labels': GENERIC, '3-D labels': GENERIC, 'no raster': GENERIC,
         'negative maxSegId': "maxSegId must be a non-negative integer (got -1)",
         'fractional maxSegId': "maxSegId must be a non-negative integer (got 2.5)",
         'maxSegId too large': "maxSegId 4294967294 is too large"}


@pytest.mark.parametrize('name', sorted(TEXTS))
@pytest.mark.parametrize('flags', [dict(), dict(merged=True, hint=True)])
def test_resolve_refuses_as_the_callers_class(name, flags):
    from pyshepseg_amd import labelsource
    args = REFUSALS[name]
    assert set(args) <= {'segfile', 'maxSegId'}
    with pytest.raises(Refused) as e:
        labelsource.resolve(args['segfile'], args.get('maxSegId'), Refused, **flags)
    assert type(e.value) is Refused and str(e.value) == TEXTS[name]


def test_every_raster_refusal_of_the_shapes_is_covered():
    assert sorted(TEXTS) == sorted(k for (k, v) in REFUSALS.items() if set(v) <= {'segfile', 'maxSegId'})


def test_resolve_merged_segments_without_outdev():
    from pyshepseg_amd import labelsource, neighbours
    merged = neighbours.MergedSegments()
    with pytest.raises(Refused) as e:
        labelsource.resolve(merged, None, Refused, merged=True)
    assert str(e.value) == "the MergedSegments holds no recoded raster: neither outDev nor segimg"
    merged.segimg = raster()
    for m in (merged, neighbours.MergedSegments()):
        with pytest.raises(Refused) as e:
            labelsource.resolve(m, None, Refused, merged=False)
        assert str(e.value) == GENERIC


def test_a_bad_maxsegid_is_refused_before_a_bad_raster_and_after_an_empty_merge():
    from pyshepseg_amd import labelsource, neighbours
    with pytest.raises(Refused, match='^maxSegId 4294967294 is too large$'):
        labelsource.resolve(None, 0xFFFFFFFE, Refused)
    with pytest.raises(Refused, match='holds no recoded raster'):
        labelsource.resolve(neighbours.MergedSegments(), -1, Refused, merged=True)


def test_origin_and_chunk_pixels():
    from pyshepseg_amd import labelsource, tilingstats
    assert labelsource.checkOrigin((np.int64(3), 4), 5, 6, Refused) == (3, 4)
    assert labelsource.checkOrigin((2 ** 32 - 5, 2 ** 32 - 6), 5, 6, Refused) == (2 ** 32 - 5, 2 ** 32 - 6)
    for (origin, text) in ((3, "origin must be (row0, col0) (got 3)"), ((1, 2, 3), "origin must be (row0, col0) (got (1, 2, 3))"),
                           ((-1, 0), "origin must be two non-negative integers (got (-1, 0))"),
                           ((0, 1.5), "origin must be two non-negative integers (got (0, 1.5))"),
                           ((True, 0), "origin must be two non-negative integers (got (True, 0))"),
                           ((2 ** 32 - 4, 0), "origin (4294967292, 0) puts a 5 x 6 raster past coordinate 2^32"),
                           ((0, 2 ** 32 - 5), "origin (0, 4294967291) puts a 5 x 6 raster past coordinate 2^32")):
        with pytest.raises(Refused) as e:
            labelsource.checkOrigin(origin, 5, 6, Refused)
        assert str(e.value) == text
    assert labelsource.checkChunkPixels(None, Refused) == tilingstats.STATS_CHUNK_PIXELS
    assert labelsource.checkChunkPixels(np.int32(7), Refused) == 7
    for bad in (0, -3, 2.0, True, 'x'):
        with pytest.raises(Refused) as e:
            labelsource.checkChunkPixels(bad, Refused)
        assert str(e.value) == "chunkPixels must be a positive integer (got {!r})".format(bad)


def test_no_import_cycle_at_load():
    """the module loads in a fresh interpreter before any of its callers, and imports none of them"""
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import sys; from pyshepseg_amd import labelsource; "
            "print([m for m in ('neighbours', 'shapes', 'outlines', 'depths', 'utils') if 'pyshepseg_amd.' + m in sys.modules])")
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, check=True)
    assert out.stdout.strip() == '[]'


# ---- LabelSource ------------------------------------------------------------------------------------------------------
def inputs(tmp_path):
    seg = raster()
    wide = np.zeros((NROWS, 2 * NCOLS), dtype=np.uint32)
    wide[:, ::2] = seg
    path = str(tmp_path / 'labels.npy')
    np.save(path, seg)
    return (seg, {'array': seg, 'strided': wide[:, ::2], 'fortran': np.asfortranarray(seg), 'memmap': np.load(path, mmap_mode='r')})


@pytest.mark.parametrize('kind', ['array', 'strided', 'fortran', 'memmap'])
def test_blocks_upload_their_rows_and_halo_once(tmp_path, kind):
    from pyshepseg_amd import labelsource
    (seg, given) = inputs(tmp_path)
    assert kind != 'strided' or not given[kind].flags['C_CONTIGUOUS']
    c = FakeCtx()
    seen = []
    with labelsource.LabelSource(c, labels_of(given[kind])) as src:
        for (y0, y1, dseg, hasAbove, hasBelow) in src.blocks(BLOCK * NCOLS, above=True, below=True):
            want = seg[y0 - hasAbove:y1 + hasBelow].tobytes()
            assert c._L.uploads[-1] == (dseg.value, want) and ctypes.string_at(dseg.value, len(want)) == want
            seen.append((y0, y1, hasAbove, hasBelow))
            assert len(c._L.uploads) == len(seen)
    assert seen == [(0, 11, False, True), (11, 22, True, True), (22, 33, True, False)]
    assert sorted(c._L.freed) == sorted(c._L.allocated) and not c._L.live


def test_resident_labels_are_addressed_in_place():
    from pyshepseg_amd import labelsource
    c = FakeCtx()
    base = 1 << 20
    with labelsource.LabelSource(c, labels_of(devSeg=base, shape=(NROWS, NCOLS))) as src:
        got = [(y0, y1, dseg.value) for (y0, y1, dseg, _a, _b) in src.blocks(BLOCK * NCOLS, above=True, below=True)]
        assert got == [(0, 11, base), (11, 22, base + 4 * 10 * NCOLS), (22, 33, base + 4 * 21 * NCOLS)]
        assert [d.value for (_y0, _y1, d, _a, _b) in src.blocks(BLOCK * NCOLS)] == [base + 4 * y * NCOLS for y in (0, 11, 22)]
        assert src.whole().value == base
    assert c._L.uploads == [] and c._L.allocated == []


def test_aligned_scratch():
    from pyshepseg_amd import labelsource
    c = FakeCtx()
    with labelsource.LabelSource(c, labels_of(devSeg=1 << 20, shape=(NROWS, NCOLS))) as src:
        for (offset, nbytes) in ((0, 64), (4, 64), (12, 1000), (8, 16)):
            dseg = ctypes.c_void_p((1 << 20) + offset)
            dout = src.alignedScratch(dseg, nbytes)
            (base, size) = c._L._room(dout.value, nbytes)
            assert dout.value % 16 == (base + offset) % 16 and dout.value - base == offset and size >= nbytes + 16
        assert len(c._L.allocated) == 2         # one buffer, grown once
    assert sorted(c._L.freed) == sorted(c._L.allocated)


def test_exit_frees_everything_once_after_an_exception_too():
    from pyshepseg_amd import labelsource
    c = FakeCtx()
    with pytest.raises(ZeroDivisionError):
        with labelsource.LabelSource(c, labels_of(raster())) as src:
            for (y0, _y1, dseg, _a, _b) in src.blocks(BLOCK * NCOLS, below=True):
                src.alignedScratch(dseg, 4 * (12 - y0) * NCOLS)
                if y0:
                    1 / 0
    assert len(c._L.allocated) >= 2 and sorted(c._L.freed) == sorted(c._L.allocated) and not c._L.live


def test_label_max():
    from pyshepseg_amd import labelsource
    seg = raster()
    top = int(seg.max())
    c = FakeCtx()
    with labelsource.LabelSource(c, labels_of(seg)) as src:           # block by block: every block goes up for it
        assert src.labelMax(Refused, BLOCK * NCOLS) == (top, 0.75)
        assert (c._L.maxCalls, len(c._L.uploads)) == (3, 3)
    c = FakeCtx()
    with labelsource.LabelSource(c, labels_of(seg)) as src:           # whole: the one upload serves both
        dseg = src.whole()
        assert src.labelMax(Refused) == (top, 0.25) and src.whole() is dseg
        assert (c._L.maxCalls, len(c._L.uploads)) == (1, 1) and c._L.uploads[0][1] == seg.tobytes()
    c = FakeCtx()
    held = np.ascontiguousarray(seg)
    with labelsource.LabelSource(c, labels_of(devSeg=held.ctypes.data, shape=seg.shape)) as src:      # resident: one reduction
        assert src.labelMax(Refused, BLOCK * NCOLS) == (top, 0.25)
        assert (c._L.maxCalls, c._L.uploads) == (1, [])
    c = FakeCtx()
    with labelsource.LabelSource(c, labels_of(np.zeros((0, 5), dtype=np.uint32))) as src:
        assert src.whole() is None and src.labelMax(Refused) == (0, 0.0) and src.labelMax(Refused, 7) == (0, 0.0)
    seg[20, 3] = 0xFFFFFFFE
    with labelsource.LabelSource(FakeCtx(), labels_of(seg)) as src:
        with pytest.raises(Refused, match='^label 4294967294 is too large$'):
            src.labelMax(Refused, BLOCK * NCOLS)


# ---- mapBlocks --------------------------------------------------------------------------------------------------------
def stamp(ncols, calls, keep=lambda y0: True):
    """a library call that writes y0 + 1 into every pixel of its block's output"""
    def call(y0, y1, dseg, dout):
        block = np.full((y1 - y0) * ncols, y0 + 1, dtype=np.uint32)
        ctypes.memmove(dout, block.ctypes.data, block.nbytes)
        calls.append((y0, y1, dseg.value, dout.value))
        return keep(y0)
    return call


def test_map_blocks_into_an_array_and_a_file(tmp_path):
    from pyshepseg_amd import labelsource
    want = np.repeat(np.array([1, 12, 23], dtype=np.uint32), BLOCK)[:, None] * np.ones(NCOLS, dtype=np.uint32)
    for outfile in (None, str(tmp_path / 'out.npy')):
        c = FakeCtx()
        calls = []
        with labelsource.LabelSource(c, labels_of(raster())) as src:
            out = labelsource.mapBlocks(src, BLOCK * NCOLS, stamp(NCOLS, calls), np.uint32, outfile=outfile)
        assert [k[:2] for k in calls] == [(0, 11), (11, 22), (22, 33)] and c._L.downloads == 3
        assert all(dout % 16 == dseg % 16 for (_y0, _y1, dseg, dout) in calls)
        got = out if outfile is None else np.load(outfile)
        assert (out is None) == (outfile is not None) and got.dtype == np.uint32 and np.array_equal(got, want)
        assert not c._L.live


def test_map_blocks_pixels_of_four_bytes(tmp_path):
    from pyshepseg_amd import labelsource

    def call(y0, y1, dseg, dout):
        block = np.full((y1 - y0, 5, 4), y0 + 1, dtype=np.uint8)
        ctypes.memmove(dout, block.ctypes.data, block.nbytes)
        return True
    seg = np.ones((7, 5), dtype=np.uint32)
    want = (np.arange(7, dtype=np.uint8) // 2 * 2 + 1)[:, None, None] * np.ones((5, 4), dtype=np.uint8)
    for outfile in (None, str(tmp_path / 'rgba.npy')):
        with labelsource.LabelSource(FakeCtx(), labels_of(seg)) as src:
            out = labelsource.mapBlocks(src, 10, call, np.uint8, pixelShape=(4,), outfile=outfile)
        got = out if outfile is None else np.load(outfile)
        assert got.shape == (7, 5, 4) and got.dtype == np.uint8 and np.array_equal(got, want)


def test_map_blocks_a_block_the_call_does_not_want_stays_on_the_device(tmp_path):
    from pyshepseg_amd import labelsource
    c = FakeCtx()
    calls = []
    outfile = str(tmp_path / 'out.npy')
    with labelsource.LabelSource(c, labels_of(raster())) as src:
        labelsource.mapBlocks(src, BLOCK * NCOLS, stamp(NCOLS, calls, keep=lambda y0: y0 < 11), np.uint32, outfile=outfile)
    got = np.load(outfile)
    assert len(calls) == 3 and c._L.downloads == 1             # every block still ran
    assert np.all(got[:11] == 1) and not got[11:].any()        # (the file's unwritten rows read as 0)


def test_map_blocks_into_a_device_raster():
    from pyshepseg_amd import labelsource
    c = FakeCtx()
    calls = []
    held = np.zeros((NROWS, NCOLS), dtype=np.uint32)
    with labelsource.LabelSource(c, labels_of(devSeg=1 << 20, shape=(NROWS, NCOLS))) as src:
        out = labelsource.mapBlocks(src, BLOCK * NCOLS, stamp(NCOLS, calls), np.uint32, devOut=ctypes.c_void_p(held.ctypes.data))
    assert out is None and c._L.downloads == 0 and c._L.allocated == []
    assert calls == [(y, y + 11, (1 << 20) + 4 * y * NCOLS, held.ctypes.data + 4 * y * NCOLS) for y in (0, 11, 22)]
    assert np.array_equal(held[:, 0], np.repeat(np.array([1, 12, 23], dtype=np.uint32), BLOCK))


def test_map_blocks_closes_the_writer_on_failure(tmp_path, monkeypatch):
    from pyshepseg_amd import labelsource, tiling
    made = []
    real = tiling._NpyRowWriter

    class Writer(real):
        def __init__(self, *args, **kw):
            real.__init__(self, *args, **kw)
            made.append(self)
    monkeypatch.setattr(tiling, '_NpyRowWriter', Writer)

    def call(y0, y1, dseg, dout):
        if y0:
            raise RuntimeError('the library failed')
        return True
    c = FakeCtx()
    with pytest.raises(RuntimeError, match='the library failed'):
        with labelsource.LabelSource(c, labels_of(raster())) as src:
            labelsource.mapBlocks(src, BLOCK * NCOLS, call, np.uint32, outfile=str(tmp_path / 'out.npy'))
    assert len(made) == 1 and made[0].fd is None
    assert sorted(c._L.freed) == sorted(c._L.allocated) and not c._L.live


def test_map_blocks_of_an_empty_raster(tmp_path):
    from pyshepseg_amd import labelsource
    for shape in ((0, 5), (5, 0)):
        with labelsource.LabelSource(FakeCtx(), labels_of(np.zeros(shape, dtype=np.uint32))) as src:
            out = labelsource.mapBlocks(src, None, None, np.uint32)
            assert out.shape == shape
            labelsource.mapBlocks(src, None, None, np.uint8, pixelShape=(4,), outfile=str(tmp_path / 'empty.npy'))
            assert np.load(str(tmp_path / 'empty.npy')).shape == shape + (4,)
