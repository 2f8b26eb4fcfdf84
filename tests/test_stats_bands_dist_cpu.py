"""calcPerSegmentStatsDistributedBands on the host path without a GPU: socket ranks with the oracle engine, which
offers the one-band methods only, so the call drives it entry by entry.  Every column against the one-band
distributed call of its entry (same process, the same driver with one entry) and against the oracle on the gathered
mosaic, bit for bit; the oracle is what keeps the first comparison honest."""
import os

import numpy as np
import pytest

from conftest import ROOT

import dist_cases
import dist_worker_stats_bands as W

WORKER = os.path.join(ROOT, 'tests', 'dist_worker_stats_bands.py')
(NR, NC, TILE, OV) = (330, 260, 96, 32)


def _image(oracle, tmp_path):
    img = oracle.synthimg(31, 3, NR, NC)
    img[:, :4, :] = 65535                       # entry 0's null value, in every band
    img[1, 100:180, 50:120] = 1234              # entry 2's null value, in the band it shares with entry 0
    np.save(tmp_path / 'img.npy', img)
    return img


def _entryColumns(fast, ic, fc, k):
    """the columns of entry k out of the combined ones, in the entry's order: [(is int, column)]"""
    from pyshepseg_amd import tilingstats
    first = sum(len(sel) for (_b, sel) in W.ENTRIES[:k])
    cols = []
    for row in fast[first:first + len(W.ENTRIES[k][1])]:
        isInt = row[tilingstats.STATSEL_COLTYPE] == tilingstats.STAT_DTYPE_INT
        cols.append((isInt, (ic if isInt else fc)[row[tilingstats.STATSEL_COLARRAYINDEX]]))
    return cols


@pytest.mark.parametrize('world', [2, 3])
def test_bands_equal_one_band_calls_and_oracle(world, tmp_path, oracle):
    from pyshepseg_amd import tilingstats
    img = _image(oracle, tmp_path)
    dist_cases.runRanks(world, [WORKER, str(tmp_path), str(TILE), str(OV)], tmp_path, 600,
                        extra_env={'OMP_NUM_THREADS': '1', 'SHEPSEG_SHARD': 'rows'})
    parts = [np.load(tmp_path / ('rank%d.npz' % r)) for r in range(world)]
    mosaic = np.zeros((NR, NC), dtype=np.uint32)
    for q in parts:
        (lo, hi) = (int(q['outLo']), int(q['outHi']))
        mosaic[lo:hi] = np.maximum(mosaic[lo:hi], q['out'])
    S = int(parts[0]['maxSegId'])
    assert {name for (_b, sel) in W.ENTRIES for (_c, name, *_p) in sel} == {
        'min', 'max', 'mean', 'stddev', 'median', 'mode', 'percentile', 'pixcount'}
    held = [set(np.unique(q['out'])) - {0} for q in parts]
    strad = set()
    for a in range(world):
        for b in range(a + 1, world):
            strad |= held[a] & held[b]
    assert len(strad) > 0
    nPix = int(np.isin(mosaic, list(strad)).sum())
    for r in range(world):
        st = np.load(tmp_path / ('bands%d.npz' % r))
        (ic, fc, fast) = (st['ic'], st['fc'], st['fast'])
        (nInt, nFloat) = tilingstats.makeBandStatsSelection(W.ENTRIES)[2:]
        assert ic.shape == (nInt, S + 1) and ic.dtype == np.int64
        assert fc.shape == (nFloat, S + 1) and fc.dtype == np.float32
        assert str(st['path']) == 'host' and int(st['bands']) == 2
        assert int(st['straddlers']) == len(strad) and int(st['straddler_pixels']) == nPix
        # the ids once (4 bytes) and one int64 value per distinct band, as the oracle engine's gatherFlagged gives them
        assert int(st['exchange_bytes']) == nPix * (4 + 2 * 8)
        for (k, (b, sel)) in enumerate(W.ENTRIES):
            assert int(st['straddlers%d' % k]) == len(strad) and int(st['straddler_pixels%d' % k]) == nPix
            (wic, wfc) = oracle.segstats(mosaic, np.ascontiguousarray(img[b - 1]), sel, W.NULLS[k], -9999, max_seg_id=S)
            (ownFast, _ni, _nf) = tilingstats.makeFastStatsSelection(list(range(len(sel))), sel)
            for ((isInt, col), own, s) in zip(_entryColumns(fast, ic, fc, k), ownFast, sel):
                idx = own[tilingstats.STATSEL_COLARRAYINDEX]
                (one, want) = (st['ic%d' % k][idx], wic[idx]) if isInt else (st['fc%d' % k][idx], wfc[idx])
                if isInt:
                    assert np.array_equal(col, one), (r, k, s)
                    assert np.array_equal(col, want), (r, k, s)
                else:
                    assert np.array_equal(col.view(np.int32), one.view(np.int32)), (r, k, s)
                    assert np.array_equal(col.view(np.int32), want.view(np.int32)), (r, k, s)
        # one entry through the several-band front end: its columns again
        assert np.array_equal(st['icS'], st['ic1'])
        assert np.array_equal(st['fcS'].view(np.int32), st['fc1'].view(np.int32))


def test_entries_differ_where_their_nulls_differ(tmp_path, oracle):
    """the test above cannot pass by ignoring the per-entry null values: entries 0 and 2 read one band and count
    different pixels"""
    img = _image(oracle, tmp_path)
    seg = np.ones((NR, NC), dtype=np.uint32)
    n0 = oracle.segstats(seg, np.ascontiguousarray(img[1]), [('n', 'pixcount')], W.NULLS[0], -9999, max_seg_id=1)[0]
    n2 = oracle.segstats(seg, np.ascontiguousarray(img[1]), [('n', 'pixcount')], W.NULLS[2], -9999, max_seg_id=1)[0]
    assert int(n0[0][1]) != int(n2[0][1])


@pytest.mark.parametrize('world', [2, 3])
def test_bad_arguments_raise_on_every_rank(world, tmp_path, oracle):
    """empty list, duplicate column name, band out of range, null list of the wrong length: every rank raises
    before any collective and goes on (a stranded rank would run into the launcher's time limit).  Then the one-band
    call with a histogram entry lowered by one: PyShepSegStatsError on every rank, and the next call works."""
    _image(oracle, tmp_path)
    errs = dist_cases.runRanks(world, [WORKER, str(tmp_path), str(TILE), str(OV), 'errors'], tmp_path, 600,
                               extra_env={'OMP_NUM_THREADS': '1', 'SHEPSEG_SHARD': 'rows'})
    for (r, e) in enumerate(errs):
        for (what, _kw) in W.BAD_ARGUMENTS:
            assert 'rank %d, %s:' % (r, what) in e, (r, what, e[-2000:])
        assert 'rank %d, %s:' % (r, W.STALE_HISTOGRAM) in e, (r, e[-2000:])
