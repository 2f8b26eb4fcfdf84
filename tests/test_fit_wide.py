"""The k-means fit over each pixel type's full range: int32 samples of both signs, uint32 samples above 2^31,
int16 samples of both signs (tests/fit_wide_cases.py), against tests/golden/kmeans_fit_wide.npz = sklearn 0.24.2's
KMeans and the reference's fitSpectralClusters with one OpenMP thread (oracle/refgen/gen_golden_fit_wide.py).
At these magnitudes a distance is up to 1e10: one float32 ulp of a stored bracket end is 1024, the exact replay
of the shifts decides far more comparisons than on 16-bit imagery, and |x|^2 reaches 1.8e19 per band.
CPU: the oracle's restatement and the host's diagonal centres.  GPU: every entry and knob of the HIP fit.  Every
comparison is of n_iter_, labels_ and the centres' bits; there are no tolerances."""
import os
import re

import numpy as np
import pytest

import fit_wide_cases as fw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NROWS, NIMAGES, NSMOOTH = 24, 6, 2


@pytest.fixture(scope='module')
def wide():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'kmeans_fit_wide.npz')) as z:
        g = {k: z[k] for k in z.files}
    assert (int(g['nrows']), int(g['nimages']), int(g['nsmooth'])) == (NROWS, NIMAGES, NSMOOTH)
    return g


def _want(g, p):
    return g[p + 'centres'], g[p + 'labels'], int(g[p + 'n_iter'])


def _row_case(g, i):
    p = 'r%02d_' % i
    (nb, k, n, levels, seed) = (int(v) for v in g[p + 'recipe'])
    xs = fw.lattice(str(g[p + 'dtype']), (n, nb), levels, seed)
    assert fw.crc(xs) == int(g[p + 'crc']), 'the sample generator no longer makes the sample the golden was made from'
    assert g[p + 'init'].shape == (k, nb)
    return xs, g[p + 'init'], _want(g, p)


def _smooth_case(g, i, oracle):
    p = 's%02d_' % i
    (nb, synth_seed, noise_seed) = (int(v) for v in g[p + 'recipe'])
    xs = fw.smooth(oracle.synthimg(synth_seed, nb, 300, 300), str(g[p + 'dtype']), nb, noise_seed)
    assert fw.crc(xs) == int(g[p + 'crc']), 'the sample generator no longer makes the sample the golden was made from'
    init = fw.smooth_init(xs)
    assert np.array_equal(init, g[p + 'init'])
    return xs, init, _want(g, p)


def _image_case(g, i):
    p = 'i%02d_' % i
    return g[p + 'img'], int(g[p + 'k']), (int(g[p + 'null']) if int(g[p + 'has_null']) else None), g[p + 'init'], _want(g, p)


def _check(got, want, what):
    """got: a KMeansModel or (centres, labels, n_iter); want: (centres, labels, n_iter)"""
    if not isinstance(got, tuple):
        got = (got.cluster_centers_, got.labels_, got.n_iter_)
    assert got[2] == want[2], '%s: n_iter %d, reference %d' % (what, got[2], want[2])
    assert np.array_equal(got[1], want[1]), '%s: %d labels differ' % (what, int((np.asarray(got[1]) != want[1]).sum()))
    assert np.array_equal(np.ascontiguousarray(got[0]).view(np.uint64), want[0].view(np.uint64)), '%s: centres differ' % what


# ---- not GPU ---------------------------------------------------------------------------------------------------------

def test_golden_covers_what_it_must(wide):
    """the case list itself: the types and signs, the long runs, nb = 1, k = 64 with a populated last cluster,
    k > 64, and at least two thirds of the row cases decided by ties"""
    rows = [(str(wide['r%02d_dtype' % i]),) + tuple(int(v) for v in wide['r%02d_recipe' % i]) for i in range(NROWS)]
    n_iter = [int(wide['r%02d_n_iter' % i]) for i in range(NROWS)]
    assert {r[0] for r in rows} == {'int32', 'uint32', 'int16'}
    for i in range(NROWS):
        xs = _row_case(wide, i)[0]
        if xs.dtype == np.uint32:
            assert xs.max() > 2 ** 31
        else:
            assert xs.min() < 0 < xs.max()
    assert sum(t >= 48 for t in n_iter) >= 2
    assert any(r[1] == 1 for r in rows) and any(r[2] >= 65 for r in rows)
    assert any(r[2] == 64 and (wide['r%02d_labels' % i] == 63).any() for (i, r) in enumerate(rows))
    assert any(r[0] == 'uint32' and r[2] <= 64 and t >= 48 for (r, t) in zip(rows, n_iter))
    assert 3 * sum(int(wide['r%02d_lloyd_equal' % i]) == 0 for i in range(NROWS)) >= 2 * NROWS
    kinds = {(wide['i%02d_img' % i].dtype.name, bool(wide['i%02d_has_null' % i])) for i in range(NIMAGES)}
    assert kinds >= {('int32', False), ('uint32', False), ('int16', True), ('int16', False)}
    for i in range(NIMAGES):
        (img, _k, null, _init, _w) = _image_case(wide, i)
        assert 2 <= img.shape[0] <= 6
        x = img.reshape(img.shape[0], -1).astype(np.float64)
        if null is not None:
            x = x[:, (x != null).all(axis=0)]
        assert ((x.max(axis=1) - x.min(axis=1)) > 0.5 * (float(np.iinfo(img.dtype).max) - np.iinfo(img.dtype).min)).all()


@pytest.mark.parametrize('i', range(NROWS))
def test_oracle_elkan_equals_reference_rows(i, wide, oracle):
    (xs, init, want) = _row_case(wide, i)
    (*got, near) = oracle.kmeans_fit_elkan_near_ties(xs.astype(np.float64), init)
    _check(tuple(got), want, 'oracle')
    assert near == int(wide['r%02d_near_ties' % i])                 # as the generator counted
    assert near > 0 or init.shape[0] > 64, 'a case with k <= 64 must hold a near tie of the bounds'
    (c, l, n) = oracle.kmeans_fit(xs.astype(np.float64), init, algorithm='full')
    lloyd_equal = n == want[2] and np.array_equal(l, want[1]) and np.array_equal(c.view(np.uint64), want[0].view(np.uint64))
    assert lloyd_equal == bool(wide['r%02d_lloyd_equal' % i])       # as the generator recorded: ties decide (or do not)


@pytest.mark.parametrize('i', range(NSMOOTH))
def test_oracle_elkan_equals_reference_smooth(i, wide, oracle):
    (xs, init, want) = _smooth_case(wide, i, oracle)
    assert int(xs.max()) - int(xs.min()) > 0.99 * 2 ** 32
    _check(oracle.kmeans_fit(xs.astype(np.float64), init, algorithm='elkan'), want, 'oracle')


@pytest.mark.parametrize('i', range(NIMAGES))
def test_host_diagonal_centres_equal_reference(i, wide, oracle):
    """the reference's wrapped bandMax - bandMin in a signed sample type, and its cast of what leaves the type"""
    from pyshepseg_amd import shepseg as host
    (img, k, null, init, want) = _image_case(wide, i)
    xs = host._sample_rows(img, 100, null)
    got = host.diagonalClusterCentres(xs, k)
    assert got.dtype == img.dtype
    assert np.array_equal(got.astype(np.float64), init)
    (xs2, minmax) = host._sample_rows(img, 100, null, wantMinMax=True)
    assert np.array_equal(host.diagonalClusterCentres(xs2, k, minmax).astype(np.float64), init)
    _check(oracle.kmeans_fit(xs.astype(np.float64), init, algorithm='elkan'), want, 'oracle')


# ---- GPU -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shepseg():
    from pyshepseg_amd import shepseg as m
    from pyshepseg_amd import _lib
    assert _lib.lib().shp_device_count() > 0, 'no GPU: the HIP path cannot run'
    return m


SETTINGS = ((), ('SHEPSEG_FIT_ALGO', 'elkan'), ('SHEPSEG_ELK_TABLE', '1'), ('SHEPSEG_ELK_UNFUSED', '1'),
            ('SHEPSEG_FIT_CHECK_DIGITS', '1'), ('SHEPSEG_FIT_SHARDS', '3'))


@pytest.mark.gpu
@pytest.mark.parametrize('setting', SETTINGS, ids=lambda s: '='.join(s) or 'default')
@pytest.mark.parametrize('i', range(NROWS))
def test_device_typed_rows_equal_reference(i, setting, wide, shepseg, monkeypatch):
    """shp_kmeans_fit_typed: the sample goes down in its pixel type"""
    (xs, init, want) = _row_case(wide, i)
    if setting:
        monkeypatch.setenv(*setting)
    km = shepseg._fit(xs, init)
    if setting == ('SHEPSEG_FIT_ALGO', 'elkan'):
        assert km.fit_path_ == 'elkan'
    _check(km, want, 'typed rows')


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(NROWS))
def test_device_float64_rows_equal_reference(i, wide, shepseg):
    """shp_kmeans_fit: the same values as float64 rows, the entry that never goes through the typed conversion"""
    (xs, init, want) = _row_case(wide, i)
    _check(shepseg._fit(xs.astype(np.float64), init), want, 'float64 rows')


@pytest.mark.gpu
@pytest.mark.parametrize('planar', ['1', '0'])
@pytest.mark.parametrize('i', range(NIMAGES))
def test_device_image_fit_equals_reference(i, planar, wide, shepseg, monkeypatch):
    """fitSpectralClusters: nulls dropped and the diagonal centres made inside the library (planar entry), or on
    the host (SHEPSEG_FIT_PLANAR=0); both against the reference's model"""
    (img, k, null, _init, want) = _image_case(wide, i)
    monkeypatch.setenv('SHEPSEG_FIT_PLANAR', planar)
    _check(shepseg.fitSpectralClusters(img, k, 100, null, True), want, 'planar entry' if planar == '1' else 'row entry')


def _smallest_margin(xs, centres):
    """the smallest relative gap between a sample's two nearest centres, in the guard's own scale
    (second - best) / (best + second + |x|^2 + max |c|^2), in extended precision"""
    x = xs.astype(np.longdouble)
    c = centres.astype(np.longdouble)
    d = ((x[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    d.sort(axis=1)
    scale = d[:, 0] + d[:, 1] + (x * x).sum(axis=1) + (c * c).sum(axis=1).max()
    return float(((d[:, 1] - d[:, 0]) / scale).min())


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(NSMOOTH))
def test_device_smooth_rows_stay_on_fast_path(i, wide, shepseg, oracle):
    """no lattice, no ties: the guard (FIT_TIE_EPS, relative) must stay quiet at 32-bit magnitudes too, and the
    fast path's expanded distances |c|^2 - 2 x.c must still order the centres as the reference's do"""
    (xs, init, want) = _smooth_case(wide, i, oracle)
    km = shepseg._fit(xs, init)
    margin = _smallest_margin(xs, want[0])
    print('smooth case %d: path %s, smallest relative margin against the final centres %.3g' % (i, km.fit_path_, margin))
    _check(km, want, 'smooth rows')
    assert km.fit_path_ == 'lloyd', 'the guard fired; smallest relative margin %.3g' % margin
    _check(shepseg._fit(xs.astype(np.float64), init), want, 'smooth float64 rows')


def _recomputed(capfd):
    found = re.findall(r'(\d+) comparisons recomputed exactly', capfd.readouterr().err)
    assert found, 'no trace line'
    return int(found[-1])                       # the counts run since the start of the fit


@pytest.mark.gpu
def test_device_exact_recomputation_is_exercised(wide, shepseg, capfd, monkeypatch):
    """the bracket of a bound is a float32 ulp of d + S wide (up to 1024 here) plus 1e-9 (d + S) on either side:
    inside it elk2_exact decides.  Every lattice case with k <= 64 holds comparisons `upper > lower bound` whose
    sides are within 2^-31 of each other, relative (the generator keeps a case only if the oracle's restatement of
    the reference's iteration counts one, near_ties): each of them lies inside the bracket whatever float32 the
    device stored, so the fit must recompute at least that many bounds exactly, and more than none."""
    monkeypatch.setenv('SHEPSEG_FIT_TRACE', '1')
    monkeypatch.setenv('SHEPSEG_FIT_ALGO', 'elkan')
    (report, none) = ([], [])
    for i in range(NROWS):
        (xs, init, want) = _row_case(wide, i)
        if init.shape[0] > 64:
            continue                             # k > 64 keeps the exact table: nothing is recomputed
        capfd.readouterr()
        km = shepseg._fit(xs, init)
        count = _recomputed(capfd)
        near = int(wide['r%02d_near_ties' % i])
        report.append('r%02d %s nb=%d k=%d n=%d n_iter=%d: %d (near ties of the bounds in the reference\'s iteration: %d)' % (
            i, xs.dtype.name, xs.shape[1], init.shape[0], len(xs), want[2], count, near))
        _check(km, want, 'traced fit')
        if count == 0 or count < near:
            none.append(report[-1])
    # for comparison: a 16-bit sample of tests/test_fit_elkan.py (int16 rows in 0..4000)
    rng = np.random.RandomState(20000 + 60)
    cent = rng.randint(0, 4000, size=(40, 6))
    xs = (cent[rng.randint(0, 40, size=20000)] + rng.randint(-3, 4, size=(20000, 6))).astype(np.int16)
    capfd.readouterr()
    shepseg._fit(xs, shepseg.diagonalClusterCentres(xs, 60).astype(np.float64))
    report.append('16-bit twin int16 nb=6 k=60 n=20000: %d' % _recomputed(capfd))
    with capfd.disabled():
        print('\ncomparisons recomputed exactly:\n  ' + '\n  '.join(report))
    assert not none, 'none, or fewer than the near ties, recomputed exactly on: ' + '; '.join(none)


def _first_row_case(g, dtype, min_iter, max_k=64):
    for i in range(NROWS):
        if str(g['r%02d_dtype' % i]) == dtype and int(g['r%02d_n_iter' % i]) >= min_iter and int(g['r%02d_recipe' % i][1]) <= max_k:
            return i
    raise AssertionError('no such case')


@pytest.mark.gpu
@pytest.mark.parametrize('max_iter', [1, 8, 9, 16, 17, 33])
def test_device_iteration_limit_at_wide_range(max_iter, wide, shepseg, oracle, monkeypatch):
    """the edges of ELK_BATCH = 8 and ELK2_REPLAY = 16 on a uint32 sample that runs 48 iterations or more"""
    (xs, init, want) = _row_case(wide, _first_row_case(wide, 'uint32', 48))
    assert want[2] >= 48
    ref = oracle.kmeans_fit(xs.astype(np.float64), init, max_iter=max_iter, algorithm='elkan')
    assert ref[2] == max_iter
    _check(shepseg._fit(xs, init, max_iter=max_iter), ref, 'default')
    monkeypatch.setenv('SHEPSEG_FIT_ALGO', 'elkan')
    km = shepseg._fit(xs, init, max_iter=max_iter)
    assert km.fit_path_ == 'elkan'
    _check(km, ref, 'elkan')


@pytest.mark.gpu
@pytest.mark.parametrize('n', [255, 257, 1023, 1024, 1025])
def test_device_chunk_edges_at_wide_range(n, wide, shepseg, oracle, monkeypatch):
    """the 256-sample chunks of k_elk2_*, the 1024 of ELK2_VCHUNK and the 4 x 256 of FIT_RPT, on int32 rows"""
    (xs, init, _want_full) = _row_case(wide, _first_row_case(wide, 'int32', 48))
    xs = np.ascontiguousarray(xs[:n])
    ref = oracle.kmeans_fit(xs.astype(np.float64), init, algorithm='elkan')
    _check(shepseg._fit(xs, init), ref, 'default')
    monkeypatch.setenv('SHEPSEG_FIT_ALGO', 'elkan')
    km = shepseg._fit(xs, init)
    assert km.fit_path_ == 'elkan'
    _check(km, ref, 'elkan')
