"""GPU: every form of the cluster assignment kernel (kmeans.h k_assign<NB, DT, RECT>) against the oracle's
km.predict, and against an independent exact-integer minimiser.

  NB     the templated band counts 1..8, 10, 12 and the run-time form (nb 9, 11, 17, 33)
  DT     uint8, int16, uint16, int32, uint32
  RECT   false: applySpectralClusters (int32 labels of a host image, grid-stride loop over the pixels)
         true:  shp_assign_rects_dev (uint16 raster-wide cluster map, rectangles of a device raster)

Null handling: none, the dtype's min or max in every band, a value in one band only (a pixel is null when
any band holds the null value), and a value outside the dtype's range (never matches).  The centres are
integers and hold exactly tied pairs -- a duplicated centre, and two centres 2 apart with pixels on their
midpoint -- so that "first minimum wins" decides labels.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NB_TEMPLATED = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12)
NB_RUNTIME = (9, 11, 17, 33)
DTYPES = ('uint8', 'int16', 'uint16', 'int32', 'uint32')
NULLS = ('none', 'min', 'max', 'one_band', 'outside')
VMAX = 1 << 22          # |value| bound of the 32-bit images: every distance term stays an exact float64 integer

# launch_assign: the pinned staging holds m2c (k x nb doubles) and |c|^2 (k doubles) after 64 bytes of
# other use, and 512 more are kept free: it accepts k * (nb + 1) * 8 + 64 + 512 <= SHP_PINNED_BYTES
SHP_PINNED_BYTES = 1 << 20


def max_k(nb):
    return min(65534, (SHP_PINNED_BYTES - 64 - 512) // (8 * (nb + 1)))


@pytest.fixture(scope='module')
def shepseg():
    from pyshepseg_amd import shepseg as m
    from pyshepseg_amd import _lib
    assert _lib.lib().shp_device_count() > 0, 'no GPU: the HIP path cannot run'
    return m


def _null_value(dtype, mode):
    info = np.iinfo(dtype)
    return {'none': None, 'min': int(info.min), 'max': int(info.max), 'one_band': int(info.min) + 1,
            'outside': int(info.max) + 1 if info.min < 0 else -1}[mode]


def make_case(nb, dtype, mode, nr=67, nc=131, k=24, seed=0):
    """(img, centres, null): integer centres with exact ties, pixels at centres, on tied midpoints and
    random; null pixels planted as the mode says"""
    rng = np.random.RandomState(seed * 1000 + nb * 10 + DTYPES.index(dtype))
    info = np.iinfo(dtype)
    lo, hi = max(int(info.min), -VMAX), min(int(info.max), VMAX)
    base = rng.randint(lo + 2, hi - 2, size=(k - 3, nb)).astype(np.int64)
    # ties: centre 2 duplicated at the end; centres t+1 and t (t+1 = t + 2 in every band) -- the
    # later index the "lower" one
    t = base[5] - 1
    cen = np.vstack([base, t + 2, t, base[2]]).astype(np.float64)
    assert cen.shape == (k, nb)
    n = nr * nc
    pick = rng.randint(0, k, size=n)
    px = cen[pick].astype(np.int64)
    mid = rng.rand(n) < 0.2
    px[mid] = t + 1                                        # equidistant from centres k-3 and k-2
    rnd = rng.rand(n) < 0.5
    px[rnd] = rng.randint(lo, hi + 1, size=(int(rnd.sum()), nb))
    img = np.ascontiguousarray(px.T.reshape(nb, nr, nc)).astype(dtype)
    null = _null_value(dtype, mode)
    if mode in ('min', 'max'):
        sel = rng.rand(nr, nc) < 0.03
        img[:, sel] = null
    elif mode == 'one_band':
        sel = np.flatnonzero(rng.rand(n) < 0.03)
        img.reshape(nb, n)[sel % nb, sel] = null
    return img, cen, null


def exact_check(img, cen, got, null):
    """the label is an exact minimiser of the squared distance (int64 arithmetic) wherever the exact gap
    to the runner-up exceeds the rounding bound of the kernel's float64 evaluation; where every term of
    that evaluation is an integer below 2^53 the label is the FIRST exact minimiser (ties included)"""
    nb = img.shape[0]
    x = img.reshape(nb, -1).T.astype(np.int64)
    c = cen.astype(np.int64)
    assert np.array_equal(c.astype(np.float64), cen)
    isnull = np.zeros(x.shape[0], dtype=bool) if null is None else (x == null).any(axis=1)
    g = got.ravel()
    assert (g[isnull] == 0).all()
    x, g = x[~isnull], g[~isnull]
    d = ((x[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)             # exact: |x - c| < 2^23 per band
    order = np.argsort(d, axis=1, kind='stable')
    first = order[:, 0]
    gap = d[np.arange(len(d)), order[:, 1]] - d[np.arange(len(d)), first]
    # the kernel evaluates |c|^2 + sum_b fma(x_b, -2 c_b, .): nb + 1 roundings of terms no larger than
    # mag = |c|^2 + 2 sum_b |x_b c_b|, each within 2^-53 of it
    mag = (c ** 2).sum(axis=1)[None, :] + 2 * (np.abs(x)[:, None, :] * np.abs(c)[None, :, :]).sum(axis=2)
    bound = (nb + 2) * 2.0 ** -52 * mag.max(axis=1).astype(np.float64)
    clear = gap > 2 * bound
    assert np.array_equal(g[clear], first[clear] + 1)
    exact = mag.max(axis=1) < (1 << 53)
    assert np.array_equal(g[exact], first[exact] + 1)
    return int(exact.sum()), int((gap[exact] == 0).sum())


@pytest.mark.parametrize('nb', NB_TEMPLATED + NB_RUNTIME)
def test_apply_clusters_every_form(nb, shepseg, oracle):
    nties = 0
    for dtype in DTYPES:
        for mode in NULLS:
            img, cen, null = make_case(nb, dtype, mode)
            got = shepseg.applySpectralClusters(shepseg.KMeansModel(cen), img, null)
            want = oracle.kmeans_assign(img, cen, null)
            assert got.dtype == np.int32 and np.array_equal(got, want), (dtype, mode)
            nexact, ties = exact_check(img, cen, got, null)
            assert nexact == got.size - int((want == 0).sum()), (dtype, mode)
            nties += ties
    assert nties > 0


def test_apply_clusters_full_32bit_range(shepseg, oracle):
    """full-range 32-bit values (0xFFFFFFFF, -2^31) and centres beyond 2^31, where the float64 terms round"""
    rng = np.random.RandomState(3)
    for dtype in ('int32', 'uint32'):
        info = np.iinfo(dtype)
        for nb in (1, 4, 9):
            img = rng.randint(info.min, int(info.max) + 1, size=(nb, 83, 97), dtype=np.int64).astype(dtype)
            img[:, 0, :3] = np.array([info.min, info.max, 0])
            cen = rng.uniform(info.min, info.max, size=(40, nb))
            cen[39] = cen[7]
            got = shepseg.applySpectralClusters(shepseg.KMeansModel(cen), img, None)
            assert np.array_equal(got, oracle.kmeans_assign(img, cen, None)), (dtype, nb)


def _assign_rects(img, rects, cen, null, fill=0xEEEE):
    """shp_assign_rects_dev of a device copy of img; returns the downloaded uint16 cluster map"""
    from pyshepseg_amd import tiling, _lib
    (nb, nr, nc) = img.shape
    ras = tiling.DeviceRaster.fromArray(img)
    c = _lib.ctx()
    d = ctypes.c_void_p()
    c.check(c._L.shp_dev_alloc(c.handle, nr * nc * 2, ctypes.byref(d)))
    try:
        c.check(c._L.shp_dev_memset(c.handle, d, fill & 0xFF, nr * nc * 2))
        rects = np.ascontiguousarray(rects, dtype=np.int32)
        cen = np.ascontiguousarray(cen, dtype=np.float64)
        c.check(c._L.shp_assign_rects_dev(
            c.handle, ctypes.c_void_p(ras.ptr), _lib.SHP_DTYPES[img.dtype], nb, nr, nc, _lib.ptr(rects),
            rects.shape[0], _lib.ptr(cen), cen.shape[0], int(null is not None), 0 if null is None else int(null),
            d))
        got = np.empty((nr, nc), dtype=np.uint16)
        c.check(c._L.shp_dev_download(c.handle, _lib.ptr(got), d, got.nbytes))
    finally:
        c.check(c._L.shp_dev_free(c.handle, d))
        ras.free()
    return got


def _rects(nr, nc):
    # raster edges (first / last row and column), 1 pixel wide or tall, one pixel, a block in the middle
    return np.array([[0, 0, nc, 1], [0, nr - 1, nc, 1], [0, 1, 1, nr - 2], [nc - 1, 1, 1, nr - 2],
                     [1, 1, 1, 1], [5, 3, 40, 9], [nc - 300, 20, 259, 30], [7, 40, 1, 20]], dtype=np.int32)


@pytest.mark.parametrize('nb', NB_TEMPLATED + NB_RUNTIME)
def test_assign_rects_every_form(nb, shepseg, oracle):
    nr, nc = 67, 331
    rects = _rects(nr, nc)
    touched = np.zeros((nr, nc), dtype=bool)
    for (x, y, w, h) in rects:
        touched[y:y + h, x:x + w] = True
    for dtype in DTYPES:
        for mode in NULLS:
            # k = 300: labels above 255 in the uint16 map
            img, cen, null = make_case(nb, dtype, mode, nr=nr, nc=nc, k=300)
            want = oracle.kmeans_assign(img, cen, null)
            got = _assign_rects(img, rects, cen, null)
            assert np.array_equal(got[touched], want[touched].astype(np.uint16)), (dtype, mode)
            assert (got[~touched] == 0xEEEE).all(), (dtype, mode)
            assert want[touched].max() > 255


def test_largest_k(shepseg, oracle):
    """nb = 1: k = max_k(1) = 65 500 centres (0, 1, ..., 65 499) fill the pinned staging; every uint16 pixel's
    label is then min(v, 65 499) + 1 in both outputs.  k + 1 is refused, and the context still works."""
    from pyshepseg_amd import _lib
    k = max_k(1)
    assert k == 65500
    cen = np.arange(k, dtype=np.float64)[:, None]
    rng = np.random.RandomState(9)
    img = rng.randint(0, 65536, size=(1, 64, 1031)).astype(np.uint16)
    img[0, 0, :6] = [0, 1, 65498, 65499, 65500, 65535]
    want = np.minimum(img[0].astype(np.int64), k - 1) + 1
    got = shepseg.applySpectralClusters(shepseg.KMeansModel(cen), img, None)
    assert np.array_equal(got, want)
    sub = np.ascontiguousarray(img[:, :2, :])
    assert np.array_equal(oracle.kmeans_assign(sub, cen, None), want[:2])
    nr, nc = img.shape[1:]
    got16 = _assign_rects(img, np.array([[0, 0, nc, nr]]), cen, None)
    assert np.array_equal(got16, want.astype(np.uint16))
    cen1 = np.arange(k + 1, dtype=np.float64)[:, None]
    with pytest.raises(_lib.ShepsegHipError):
        shepseg.applySpectralClusters(shepseg.KMeansModel(cen1), img, None)
    with pytest.raises(_lib.ShepsegHipError):
        _assign_rects(img, np.array([[0, 0, nc, nr]]), cen1, None)
    # the context still works
    small = np.array([[100.0], [60000.0]])
    got = shepseg.applySpectralClusters(shepseg.KMeansModel(small), img, None)
    assert np.array_equal(got, oracle.kmeans_assign(img, small, None))


@pytest.mark.parametrize('nb', [3, 9], ids=['templated_nb3', 'runtime_nb9'])
def test_assign_grid_stride(nb, shepseg, oracle):
    """2049 x 2049 pixels: more than the 4 194 304 one sweep of the capped grid covers (4096 workgroups x
    256 threads x 4 pixels), so the grid-stride loop runs a second time"""
    img, cen, null = make_case(nb, 'uint16', 'max', nr=2049, nc=2049, k=20)
    assert img.shape[1] * img.shape[2] > 4096 * 256 * 4
    got = shepseg.applySpectralClusters(shepseg.KMeansModel(cen), img, null)
    assert np.array_equal(got, oracle.kmeans_assign(img, cen, null))
