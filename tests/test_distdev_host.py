"""The steps the multi-rank device paths share (pyshepseg_amd/distdev.py), on the host: device scratch, the padded
all-gather of records, the resident histogram, the column block's size, the first error of the ranks.  No GPU and
no library: the device allocator is replaced by recorders, the context and the communicator by fakes that record
what they are asked to copy and gather."""
import ctypes

import numpy as np
import pytest

from pyshepseg_amd import distdev, tiling


@pytest.fixture
def blocks(monkeypatch):
    """tiling._devAlloc / _devRelease as recorders (the real ones cache by (c.device, nbytes) in a module dict)"""
    rec = {'alloc': [], 'release': []}

    def alloc(c, nbytes):
        p = ctypes.c_void_p(0x1000 * (len(rec['alloc']) + 1))
        rec['alloc'].append((p.value, nbytes))
        return p

    def release(c, p, nbytes):
        rec['release'].append((p.value, nbytes))
    monkeypatch.setattr(tiling, '_devAlloc', alloc)
    monkeypatch.setattr(tiling, '_devRelease', release)
    return rec


class _FakeLib(object):
    def __init__(self, calls):
        self.calls = calls

    def shp_dev_copy(self, handle, dst, src, nbytes):
        self.calls.append(('copy', dst.value, src.value, nbytes))
        return 0

    def shp_dev_upload(self, handle, dst, src, nbytes):
        self.calls.append(('upload', dst.value, nbytes))
        return 0

    def shp_dev_download(self, handle, dst, src, nbytes):
        self.calls.append(('download', src.value, nbytes))
        return 0


class _FakeCtx(object):
    handle = None

    def __init__(self):
        self.calls = []
        self._L = _FakeLib(self.calls)

    def check(self, rc):
        assert rc == 0
        self.calls.append(('check',))


class _FakeComm(object):
    def __init__(self, rank, world):
        (self.rank, self.world, self.gathers) = (rank, world, [])

    def allgather_dev(self, send, recv, nbytes):
        self.gathers.append((send, recv, nbytes))


def test_scratch_releases_every_block_once(blocks):
    with distdev.Scratch(None) as s:
        a = s.alloc(100)
        b = s.alloc(0)
        assert isinstance(a, ctypes.c_void_p) and a.value != b.value
        assert blocks['release'] == []
    assert blocks['alloc'] == [(a.value, 100), (b.value, 0)]
    assert sorted(blocks['release']) == sorted(blocks['alloc'])


def test_scratch_releases_when_the_body_raises(blocks):
    boom = ValueError('boom')
    with pytest.raises(ValueError) as got:
        with distdev.Scratch(None) as s:
            s.alloc(64)
            s.alloc(32)
            raise boom
    assert got.value is boom
    assert sorted(blocks['release']) == sorted(blocks['alloc']) and len(blocks['alloc']) == 2


@pytest.mark.parametrize('raising', [False, True])
def test_scratch_kept_block_survives(blocks, raising):
    try:
        with distdev.Scratch(None) as s:
            a = s.alloc(48)
            kept = s.alloc(4096)
            assert s.keep(kept) is kept
            if raising:
                raise KeyError('late')
    except KeyError:
        assert raising
    assert blocks['release'] == [(a.value, 48)]


def _gather(blocks, rank, counts, count, item=16, **kw):
    (c, comm) = (_FakeCtx(), _FakeComm(rank, len(counts)))
    src = ctypes.c_void_p(0xABC000)
    with distdev.Scratch(c) as s:
        got = distdev.gatherRecords(s, c, comm, src, count, counts, item, **kw)
    return got, c, comm, src


def test_gather_records_nothing_travels(blocks):
    ((d_all, slot), c, comm, _src) = _gather(blocks, 1, [0, 0, 0], 0)
    assert (d_all, slot) == (None, 0)
    assert blocks['alloc'] == [] and c.calls == [] and comm.gathers == []


def test_gather_records_pads_to_the_largest_count(blocks):
    ((d_all, slot), c, comm, src) = _gather(blocks, 0, [3, 0, 5], 3)
    assert slot == 5
    assert [n for (_p, n) in blocks['alloc']] == [80, 240]
    (d_send, _n) = blocks['alloc'][0]
    assert d_all.value == blocks['alloc'][1][0]
    assert [x for x in c.calls if x[0] == 'copy'] == [('copy', d_send, src.value, 48)]
    assert comm.gathers == [(d_send, d_all.value, 80)]
    assert sorted(blocks['release']) == sorted(blocks['alloc'])


def test_gather_records_rank_without_records_takes_part(blocks):
    ((d_all, slot), c, comm, _src) = _gather(blocks, 1, [3, 0, 5], 0)
    assert slot == 5 and d_all is not None
    assert [x for x in c.calls if x[0] == 'copy'] == []
    assert [g[2] for g in comm.gathers] == [80]
    assert [n for (_p, n) in blocks['alloc']] == [80, 240]


def test_gather_records_world_of_one(blocks):
    ((d_all, slot), c, comm, src) = _gather(blocks, 0, [7], 7, inPlaceAlone=True)
    assert d_all is src and slot == 7
    assert blocks['alloc'] == [] and c.calls == [] and comm.gathers == []
    ((d_all, slot), c, comm, src) = _gather(blocks, 0, [7], 7)
    assert slot == 7 and d_all.value == blocks['alloc'][1][0]
    assert [n for (_p, n) in blocks['alloc']] == [112, 112]
    assert [x for x in c.calls if x[0] == 'copy'] == [('copy', blocks['alloc'][0][0], src.value, 112)]
    assert comm.gathers == [(blocks['alloc'][0][0], d_all.value, 112)]


def test_resident_hist_takes_a_device_histogram_as_it_is(blocks):
    c = _FakeCtx()
    with distdev.Scratch(c) as s:
        (d_hist, ns, h32) = distdev.residentHist(s, c, ('dev', 0x5000, 9))
    assert (d_hist.value, ns, h32) == (0x5000, 9, None)
    assert blocks['alloc'] == [] and blocks['release'] == [] and c.calls == []
    with distdev.Scratch(c) as s:
        (d_hist, ns, h32) = distdev.residentHist(s, c, ('dev', 0x5000, 9), host=True)
    assert h32.dtype == np.uint32 and h32.shape == (9,)
    assert [x for x in c.calls if x[0] != 'check'] == [('download', 0x5000, 36)]
    assert blocks['alloc'] == [] and blocks['release'] == []


def test_resident_hist_uploads_a_host_array(blocks):
    c = _FakeCtx()
    hist = np.array([0, 4, 2, 7, 1], dtype=np.int64)
    with distdev.Scratch(c) as s:
        (d_hist, ns, h32) = distdev.residentHist(s, c, hist)
        assert blocks['release'] == []
    assert ns == len(hist) and h32.dtype == np.uint32 and (h32 == hist).all()
    assert blocks['alloc'] == [(d_hist.value, 20)] and blocks['release'] == [(d_hist.value, 20)]
    assert [x for x in c.calls if x[0] != 'check'] == [('upload', d_hist.value, 20)]


@pytest.mark.parametrize('nInt,nFloat,ns,words', [(0, 1, 1, 1), (1, 0, 1, 1), (3, 2, 7, 28)])
def test_col_words(nInt, nFloat, ns, words):
    """4 bytes round up to one word; 8 bytes are one; 7 x (24 + 8) = 224 bytes are 28"""
    assert distdev.colWords(nInt, nFloat, ns) == ((nInt * 8 + nFloat * 4) * ns + 7) // 8 == words


class _Err(Exception):
    pass


def test_raise_first():
    with pytest.raises(_Err) as got:
        distdev.raiseFirst(_Err, [None, '', 'second rank', 'third rank'])
    assert str(got.value) == 'second rank'
    assert distdev.raiseFirst(_Err, [None, '', None]) is None
    assert distdev.raiseFirst(_Err, []) is None
