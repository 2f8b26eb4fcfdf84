"""Shared image builders and oracle compositions of the GPU tests (no GPU needed to import)."""
import numpy as np


def oracle_tiled(oracle, img, centres, tile, ov, minseg, msd, null, four, simple=False):
    """The tiled driver's result by the oracle: every tile segmented on its own, then stitched."""
    nr, nc = img.shape[1:]
    tiles, ntc, ntr = oracle.get_tiles(nr, nc, tile, ov)
    local = {}
    for (c, r), (x, y, xs, ys) in tiles.items():
        sub = np.ascontiguousarray(img[:, y:y + ys, x:x + xs])
        local[(c, r)] = oracle.segment_tile(sub, centres, minseg, msd, null, four)['segimg']
    return oracle.stitch_tiles(local, tiles, ntc, ntr, nr, nc, ov, simple=simple)


def fixed_centres(img, k, null=None):
    """k spectra picked evenly along the raster (non-null pixels): a deterministic k-means model
    that needs no fit, so a test exercises only the stages after it."""
    x = img.reshape(img.shape[0], -1).T
    if null is not None:
        x = x[(x != null).all(axis=1)]
    return np.ascontiguousarray(x[np.linspace(0, x.shape[0] - 1, k).astype(np.int64)], dtype=np.float64)


def synth_tile(oracle, seed, nr, nc, nb=3, k=30):
    """(img, centres) of a synthetic uint16 tile; segment counts grow with nr * nc (about 20 000
    segments survive the single-pixel stage at 1024 x 1024 with k = 30)."""
    img = oracle.synthimg(seed, nb, nr, nc)
    return img, fixed_centres(img, k)


def int16_nulls_tile(oracle, seed, nr, nc, nb=4, null=-999):
    """a multi-band int16 tile with negative values and a null rectangle plus scattered null pixels"""
    img = (oracle.synthimg(seed, nb, nr, nc).astype(np.int32) - 1500).astype(np.int16)
    rng = np.random.RandomState(seed)
    img[:, nr // 3:nr // 3 + 40, nc // 4:nc // 2] = null
    img[:, rng.rand(nr, nc) < 0.002] = null
    return img, fixed_centres(img, 25, null), null


def many_sources_one_target():
    """(img, centres): hundreds of 3-pixel blobs of distinct values on one uniform background, all of
    which merge into the same target in one pass (tests/test_gpu_tile.py::test_many_sources_one_target)."""
    rng = np.random.RandomState(12)
    nb, nr, nc = 3, 300, 400
    img = np.empty((nb, nr, nc), dtype=np.uint16)
    img[:] = np.array([20000, 30000, 40000], dtype=np.uint16)[:, None, None]
    for y in range(4, nr - 4, 6):
        for x in range(4, nc - 4, 7):
            v = np.array([20000, 30000, 40000]) + rng.randint(3000, 9000, size=nb)
            img[:, y, x:x + 3] = v[:, None].astype(np.uint16)
    return img, np.array([[20000., 30000., 40000.], [26000., 36000., 46000.]])


def cut_components(nr=700, nc=900):
    """cluster codes with components far above the depth-first cut's 10001-pixel cap and
    diagonal-only bridges (tests/test_gpu_tile.py::test_cut_components_both_connectivities)"""
    rng = np.random.RandomState(21)
    cl = np.ones((nr, nc), dtype=np.int32)
    yy, xx = np.mgrid[0:nr, 0:nc]
    for _i in range(14):
        cy, cx, ry, rx = rng.randint(50, nr - 50), rng.randint(50, nc - 50), rng.randint(40, 160), rng.randint(40, 200)
        cl[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1.0] = rng.randint(2, 5)
    cl[(yy + xx) % 97 == 0] = 5
    cl[rng.rand(nr, nc) < 0.01] = 0
    return cl


def uniform_region():
    """one component whose bounding box does not fit the replay's LDS bitmap
    (tests/test_gpu_tile.py::test_uniform_region_global_replay)"""
    cl = np.full((1200, 1100), 3, dtype=np.int32)
    cl[400:420, 300:900] = 0
    return cl


def stats_band(oracle, dtype, nr=161, nc=273):
    """(seg, band, null) of tests/test_gpu_stats.py::test_stats_patch_path_dtypes ('rows' labels), for
    every band type the statistics take, 32-bit ones over their full range"""
    seg = ((np.arange(nr)[:, None] // 6) * 100 + np.arange(nc)[None, :] // 9 + 1).astype(np.uint32)
    seg[-2:] = 0
    base = oracle.synthimg(23, 1, nr, nc)[0].astype(np.int64)
    if dtype == 'uint8':
        band = (base >> 5).astype(np.uint8)
    elif dtype == 'uint16':
        band = base.astype(np.uint16)
    elif dtype == 'int16':
        band = (base - 32768).astype(np.int16)
    elif dtype == 'int32':
        band = ((base - 2720) * 2500000).astype(np.int32)
        band[::3, ::2] = band[0, 0]
    else:
        band = (base * 1200000).astype(np.uint32)
        band[1::3, ::2] = np.uint32(0xFFFFFFFF)
    return seg, band, int(band[3, 5])


STATS_SEL = [('mn', 'min'), ('mx', 'max'), ('mean', 'mean'), ('sd', 'stddev'), ('med', 'median'),
             ('mode', 'mode'), ('p80', 'percentile', 80), ('n', 'pixcount')]
