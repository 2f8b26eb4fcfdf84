"""The SHEPSEG_* knob matrix of tests/test_gpu_knob_paths.py and its cases.

Importable without a GPU (tests/test_knob_inventory.py reads MATRIX).  Every setting runs in a fresh
child process (tests/knob_worker.py): the library reads these knobs once per process.  run_case()
is the GPU side of a case, expected() the oracle's; both return dicts of arrays compared exactly."""
import numpy as np

import clump_shape_cases
import prim_cases
import segtable_cases
from seg_cases import (STATS_SEL, cut_components, fixed_centres, many_sources_one_target, oracle_tiled,
                       stats_band, synth_tile, uniform_region)

STATS_DTYPES = ('uint8', 'uint16', 'int16', 'int32', 'uint32')
TILED = ('tiled4',)
SMALL = ('tile256', 'tile1000', 'many_sources')
# clump_shapes4 / 8: every shape of tests/clump_shape_cases.py but many_big, whose walks reach every step of the
# depth-first cut replay (under dfs_pool_1 on the walker whose bitmap lives in global memory); clump_many_big: more
# cut components than one-walker workgroups are launched, so the counter hands out the rest
CLUMP = ('clump_cut4', 'clump_cut8', 'clump_uniform', 'clump_shapes4', 'clump_shapes8')
MANY_BIG = ('clump_many_big',)

# (name, environment of the child, cases that reach the code the setting changes)
MATRIX = [
    ('scan_two_launch', {'SHEPSEG_SCAN_ONE': '0'},
     ('tile', 'tiled4', 'stats_sort_int32', 'stats_sort_uint8', 'subset', 'tables', 'prim_scan', 'prim_sort')),
    ('csr_pixel_sort', {'SHEPSEG_CSR_RUNS': '0'}, ('tables',)),
    ('sort_wide', {'SHEPSEG_SORT_WIDE': '1'}, tuple('stats_sort_' + d for d in STATS_DTYPES) + ('prim_sort',)),
    ('small_no_lists', {'SHEPSEG_SMALL_LISTS': '0'}, SMALL),
    ('small_one_level_barrier', {'SHEPSEG_SMALL_BAR2': '0'}, SMALL),
    ('small_blocks_1', {'SHEPSEG_SMALL_BLOCKS': '1'}, SMALL),
    ('small_blocks_24', {'SHEPSEG_SMALL_BLOCKS': '24'}, SMALL),
    ('small_poll_1', {'SHEPSEG_SMALL_POLL': '1'}, ('tile256',)),
    ('small_max_1', {'SHEPSEG_SMALL_MAX': '1'}, TILED),
    ('dfs_oldwalk', {'SHEPSEG_DFS_OLDWALK': '1'}, CLUMP + TILED),
    ('dfs_pool_1', {'SHEPSEG_DFS_POOL': '1'}, CLUMP + TILED),
    ('dfs_pool_64', {'SHEPSEG_DFS_POOL': '64'}, CLUMP + TILED),
    ('dfs_per_wg_1', {'SHEPSEG_DFS_PER_WG': '1'}, CLUMP + MANY_BIG + TILED),
    ('dfs_per_wg_3', {'SHEPSEG_DFS_PER_WG': '3'}, CLUMP + MANY_BIG + TILED),
    ('own_streams', {'SHEPSEG_SHARED_STREAMS': '0'}, TILED),
    ('walk_streams_1', {'SHEPSEG_WALK_STREAMS': '1'}, TILED),
    ('tile_order_rowmajor', {'SHEPSEG_TILE_ORDER': 'rowmajor'}, TILED),
    ('fill_max_1', {'SHEPSEG_FILL_MAX': '1'}, TILED),
]

TABLES_CASE = ('ids_65537', 'uint16', 3)       # (segtable_cases generator, dtype, nb): S >= 65 536


def device_tables(seg, img, max_seg_id):
    """spectra (buildSegmentSpectra), the raw CSR of shp_segment_locations (offsets of ids 0 .. S + 1,
    pixel indices grouped by id, the null segment first) and makeSegSize of one raster, on the device"""
    from pyshepseg_amd import _lib, shepseg
    seg = np.ascontiguousarray(seg, dtype=np.uint32)
    (nr, nc) = seg.shape
    off = np.zeros(max_seg_id + 2, dtype=np.uint32)
    pix = np.empty(seg.size, dtype=np.uint32)
    c = _lib.ctx()
    c.check(c._L.shp_segment_locations(c.handle, _lib.ptr(seg), nr, nc, max_seg_id, _lib.ptr(off), _lib.ptr(pix)))
    out = {'off': off, 'pix': pix, 'size': shepseg.makeSegSize(seg)}
    if img is not None:
        out['spectra'] = shepseg.buildSegmentSpectra(seg, img, max_seg_id)
    return out


def expected_tables(seg, img, max_seg_id, oracle):
    """the same tables by the oracle and numpy: a stable argsort groups the pixels"""
    cnt = np.bincount(seg.ravel(), minlength=max_seg_id + 1)
    out = {'off': np.r_[0, np.cumsum(cnt)].astype(np.uint32),
           'pix': np.argsort(seg.ravel(), kind='stable').astype(np.uint32),
           'size': np.bincount(seg.ravel()).astype(np.uint32)}
    if img is not None:
        out['spectra'] = oracle.build_segment_spectra(seg, img, max_seg_id)
    return out


TILED_ARGS = dict(seed=7, nb=4, nr=900, nc=1100, tile=384, ov=96, ms=40, workers=4)


def _tile_inputs(oracle, name):
    if name in ('tile256', 'tile1000'):
        img, cen = synth_tile(oracle, 5, 1024, 1024, k=60)
        return img, cen, int(name[4:])
    if name == 'many_sources':
        img, cen = many_sources_one_target()
        return img, cen, 10
    img, cen = synth_tile(oracle, 3, 300, 400)
    return img, cen, 25


def _msd(cen):
    from pyshepseg_amd import shepseg
    return float(shepseg.autoMaxSpectralDiff(shepseg.KMeansModel(cen), 'auto', 50))


def _clump_shapes(name, clump):
    """a clump_shapes4 / clump_shapes8 / clump_many_big case: clump(cl, four) -> (labels, next id) on its shapes,
    the outputs keyed by shape"""
    four = name != 'clump_shapes8'
    out = {}
    for shape in (('many_big',) if name == 'clump_many_big' else clump_shape_cases.MODEL_SHAPES):
        seg, nxt = clump(clump_shape_cases.make(shape), four)
        out[shape + '/seg'] = seg
        out[shape + '/next'] = np.array([nxt])
    return out


def _subset_inputs():
    rng = np.random.RandomState(11)
    base = rng.permutation(np.arange(1, 20 * 18 + 1)).reshape(20, 18).astype(np.uint32)
    seg = np.kron(base, np.ones((70, 80), dtype=np.uint32))[:1350, :1400]
    seg[rng.rand(*seg.shape) < 0.01] = 0
    mask = (rng.rand(1150, 1250) > 0.2).astype(np.uint8)
    return seg, mask


def run_case(name, oracle, tmpdir):
    """the GPU side of a case (in the child)"""
    import os
    from pyshepseg_amd import shepseg
    if name in ('tile', 'tile256', 'tile1000', 'many_sources'):
        img, cen, ms = _tile_inputs(oracle, name)
        msd = 1e9 if name == 'many_sources' else _msd(cen)
        r = shepseg.doShepherdSegmentation(img, kmeansObj=shepseg.KMeansModel(cen), minSegmentSize=ms,
                                           maxSpectralDiff=msd)
        return {'seg': r.segimg, 'counts': np.array([r.singlePixelsEliminated, r.smallSegmentsEliminated])}
    if name == 'tiled4':
        from pyshepseg_amd import tiling
        a = TILED_ARGS
        ras = tiling.DeviceRaster.synth(a['seed'], a['nb'], a['nr'], a['nc'])
        try:
            cen = fixed_centres(oracle.synthimg(a['seed'], a['nb'], a['nr'], a['nc']), 20)
            cfg = tiling.SegmentationConcurrencyConfig(concurrencyType=tiling.CONC_THREADS, numWorkers=a['workers'])
            r = tiling.doTiledShepherdSegmentation(ras, None, tileSize=a['tile'], overlapSize=a['ov'],
                                                   minSegmentSize=a['ms'], kmeansObj=shepseg.KMeansModel(cen),
                                                   concurrencyCfg=cfg)
        finally:
            ras.free()
        return {'seg': r.segimg, 'hist': r.hist, 'max': np.array([r.maxSegId])}
    if name.startswith('stats_sort_'):
        from pyshepseg_amd import tilingstats
        seg, band, null = stats_band(oracle, name[len('stats_sort_'):])
        os.environ['SHEPSEG_STATS_PATCH'] = '0'          # the sort path (read on every call)
        try:
            r = tilingstats.calcPerSegmentStatsTiled(band, 1, seg, STATS_SEL, imgNullVal=null)
        finally:
            del os.environ['SHEPSEG_STATS_PATCH']
        return {k: r.columns[k] for k in ('mn', 'mx', 'med', 'mode', 'p80', 'n', 'mean', 'sd')}
    if name == 'subset':
        from pyshepseg_amd import subset
        seg, mask = _subset_inputs()
        src = os.path.join(tmpdir, 'subset_seg.npy')
        np.save(src, seg)
        r = subset.subsetImage(src, os.path.join(tmpdir, 'subset_out.npy'), 150, 200, 1250, 1150, maskImage=mask)
        return {'seg': r.segimg, 'orig': r.origSegIds, 'hist': r.hist}
    if name.startswith('clump_shapes') or name in MANY_BIG:
        return _clump_shapes(name, lambda cl, four: shepseg.clump(cl, 0, fourConnected=four))
    if name in CLUMP:
        cl = uniform_region() if name == 'clump_uniform' else cut_components()
        seg, nxt = shepseg.clump(cl, 0, fourConnected=name != 'clump_cut8')
        return {'seg': seg, 'next': np.array([nxt])}
    if name == 'tables':
        return device_tables(*segtable_cases.make(*TABLES_CASE))
    if name == 'prim_scan':
        return prim_cases.knob_scan_run()
    if name == 'prim_sort':
        return prim_cases.knob_sort_run()
    raise KeyError(name)


def expected(name, oracle):
    """the oracle's result of a case (in the parent)"""
    if name in ('tile', 'tile256', 'tile1000', 'many_sources'):
        img, cen, ms = _tile_inputs(oracle, name)
        msd = 1e9 if name == 'many_sources' else _msd(cen)
        w = oracle.segment_tile(img, cen, ms, msd, None, True)
        return {'seg': w['segimg'], 'counts': np.array([w['singlePixelsEliminated'], w['smallSegmentsEliminated']])}
    if name == 'tiled4':
        a = TILED_ARGS
        img = oracle.synthimg(a['seed'], a['nb'], a['nr'], a['nc'])
        cen = fixed_centres(img, 20)
        want, mx, hist = oracle_tiled(oracle, img, cen, a['tile'], a['ov'], a['ms'], _msd(cen), None, True)
        return {'seg': want, 'hist': hist, 'max': np.array([mx])}
    if name.startswith('stats_sort_'):
        seg, band, null = stats_band(oracle, name[len('stats_sort_'):])
        ic, fc = oracle.segstats(seg, band, STATS_SEL, null_val=null)
        out = {k: ic[i] for i, k in enumerate(['mn', 'mx', 'med', 'mode', 'p80', 'n'])}
        out['mean'], out['sd'] = fc[0], fc[1]
        return out
    if name == 'subset':
        seg, mask = _subset_inputs()
        want, worig, whist = oracle.subset_recode(seg, 150, 200, 1250, 1150, mask, 1024)
        return {'seg': want, 'orig': worig, 'hist': whist}
    if name.startswith('clump_shapes') or name in MANY_BIG:
        return _clump_shapes(name, lambda cl, four: oracle.clump(cl, 0, four, 1))
    if name in CLUMP:
        cl = uniform_region() if name == 'clump_uniform' else cut_components()
        seg, nxt = oracle.clump(cl, 0, name != 'clump_cut8', 1)
        return {'seg': seg, 'next': np.array([nxt])}
    if name == 'tables':
        return expected_tables(*segtable_cases.make(*TABLES_CASE), oracle)
    if name == 'prim_scan':             # the numpy models of tests/prim_cases.py: no oracle
        return prim_cases.knob_scan_expected()
    if name == 'prim_sort':
        return prim_cases.knob_sort_expected()
    raise KeyError(name)


def same(got, want):
    """exact equality; float columns compared by their bits"""
    if got.dtype.kind == 'f' or want.dtype.kind == 'f':
        return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(
            got.view(np.uint8), want.view(np.uint8))
    return np.array_equal(got, want)
