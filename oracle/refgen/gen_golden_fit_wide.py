"""Golden vectors for the fit over each pixel type's full range: tests/golden/kmeans_fit_wide.npz.

    OMP_NUM_THREADS=1 /opt/conda/bin/python3.9 oracle/refgen/gen_golden_fit_wide.py

Inputs (tests/fit_wide_cases.py): int32 samples of both signs, uint32 samples with values above 2^31 and int16
samples of both signs, on a lattice that spans the whole type (exact distance ties decide labels); rasters of the
same kind, with and without a null value, where the reference takes its wrapped bandMax - bandMin in a signed
type; and two smooth 32-bit samples.  Expected outputs, all from the REFERENCE stack with one OpenMP thread
(the only reproducible setting):
  row and smooth cases   sklearn 0.24.2's KMeans(n_clusters=k, init=init, n_init=1).fit(xs)
  image cases            the reference's shepseg.fitSpectralClusters(img, k, 100, null, True)
A row case is kept only if the oracle's Elkan restatement equals the reference bit for bit (one that does not is
a bug of oracle/shepseg_oracle.c, to be fixed there first); whether the Lloyd restatement does is printed and
stored.  A row case with k <= 64 is kept only if the reference's iteration, as the oracle restates it, makes at
least one comparison `upper > lower bound` whose sides are within 2^-31 of each other (oracle.kmeans_fit_elkan_near_ties,
"near ties"): the HIP fit brackets a bound by a float32 widened by 1e-9 on either side and has to recompute it
exactly there, so such a sample exercises elk2_exact whatever the device does; the count is stored.  
Row and smooth samples are stored as recipe + crc32 and rebuilt by tests/fit_wide_cases.py (which this script
imports, so that both make them with the same code): the 24 row samples alone are 789000 values and compress to
about 510 KB, above the largest fixture of tests/golden (stitch_3x4_8conn.npz, 421835 bytes), which this file
must not exceed.  Images are stored as arrays.  Build container only (refenv.py)."""
import os
import sys
import warnings
import numpy as np
warnings.filterwarnings('ignore')
import refenv                                   # noqa: E402
from refenv import shepseg                      # noqa: E402
from sklearn.cluster import KMeans              # noqa: E402
from oracle import oracle                       # noqa: E402

assert os.environ.get('OMP_NUM_THREADS') == '1', 'run with OMP_NUM_THREADS=1'
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import fit_wide_cases as fw                     # noqa: E402


def same(a, b):
    return a[2] == b[2] and np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))


def reference_rows(xs, init):
    km = KMeans(n_clusters=init.shape[0], init=init, n_init=1).fit(xs)
    return (np.asarray(km.cluster_centers_, dtype=np.float64), np.asarray(km.labels_, dtype=np.int32), int(km.n_iter_))


def store(out, p, res, init):
    out[p + 'init'] = init
    out[p + 'centres'] = res[0]
    out[p + 'labels'] = res[1]
    out[p + 'n_iter'] = np.int32(res[2])


out = {}
# ---- row cases -------------------------------------------------------------------------------------------------------
specs = fw.ROWS
print('row cases: sklearn %s KMeans against the oracle' % __import__('sklearn').__version__)
print('%-4s %-7s %3s %3s %6s %6s %5s %7s %9s %s' % ('case', 'dtype', 'nb', 'k', 'n', 'levels', 'seed', 'n_iter', 'near ties', 'Lloyd restatement equals reference'))
(kept, differ, long_runs) = (0, 0, 0)
for (j, (dt, nb, k, n, lv, *named)) in enumerate(specs):
    # the seed the case names, or up to 8 candidate seeds: with k <= 64, ones whose iteration holds a near tie of the bounds (below); of the
    # candidates the first on which a tie decides the result, failing that the first
    (pick, tried) = (None, 0)
    for seed in (named or range(1000 + 200 * j, 1200 + 200 * j)):
        xs = fw.lattice(dt, (n, nb), lv, seed)
        init = shepseg.diagonalClusterCentres(xs, k).astype(np.float64)
        (*elk, near) = oracle.kmeans_fit_elkan_near_ties(xs.astype(np.float64), init)
        if k <= 64 and near == 0:
            continue                             # nothing here that a float32 bracket of a bound cannot decide
        ref = reference_rows(xs, init)
        if not same(elk, ref):
            print('     %s nb=%d k=%d n=%d seed %d: the oracle\'s Elkan restatement DIFFERS from the reference: not kept' % (dt, nb, k, n, seed))
            continue
        if k == 64 and not (ref[1] == 63).any():
            continue                             # the k = 64 cases are there for a populated last cluster
        lloyd = same(oracle.kmeans_fit(xs.astype(np.float64), init, algorithm='full'), ref)
        tried += 1
        if pick is None or not lloyd:
            pick = (seed, xs, init, ref, lloyd, near)
        if not lloyd or tried == 8:
            break
    if pick is None:
        raise SystemExit('no seed for %r' % ((dt, nb, k, n, lv),))
    (seed, xs, init, ref, lloyd, near) = pick
    p = 'r%02d_' % kept
    out[p + 'recipe'] = np.array([nb, k, n, lv, seed], dtype=np.int64)
    out[p + 'dtype'] = np.array(dt)
    out[p + 'crc'] = fw.crc(xs)
    out[p + 'lloyd_equal'] = np.int32(lloyd)
    out[p + 'near_ties'] = np.int64(near)
    store(out, p, ref, init)
    print('r%02d  %-7s %3d %3d %6d %6d %5d %7d %9d %s' % (kept, dt, nb, k, n, lv, seed, ref[2], near, ('no', 'yes')[lloyd]))
    kept += 1
    differ += not lloyd
    long_runs += ref[2] >= 48
out['nrows'] = np.int32(kept)
print('%d row cases, %d of them (%.0f%%) decided by ties (Lloyd restatement differs), %d with n_iter >= 48' % (
    kept, differ, 100. * differ / kept, long_runs))
assert 3 * differ >= 2 * kept and long_runs >= 2

# ---- image cases -----------------------------------------------------------------------------------------------------
IMAGES = (('int32', 3, 70, 90, 7, 20, None, 0.0), ('uint32', 2, 75, 80, 12, 30, None, 0.0),
          ('int16', 4, 80, 75, 9, 15, -32768, 0.2), ('int16', 6, 60, 70, 5, 40, None, 0.0),
          ('uint32', 5, 64, 72, 6, 24, 4294967295, 0.15), ('int32', 2, 96, 70, 20, 64, -2147483648, 0.1))
print('image cases: the reference\'s fitSpectralClusters(img, k, 100, null, True)')
for (i, (dt, nb, nr, nc, lv, k, null, share)) in enumerate(IMAGES):
    img = fw.lattice_image(dt, nb, nr, nc, lv, 2000 + i, null, share)
    km = shepseg.fitSpectralClusters(img, k, 100, null, True)
    ref = (np.asarray(km.cluster_centers_, dtype=np.float64), np.asarray(km.labels_, dtype=np.int32), int(km.n_iter_))
    x = np.transpose(img, (1, 2, 0)).reshape(nr * nc, nb)
    if null is not None:
        x = x[(x != null).all(axis=1)]
    init = shepseg.diagonalClusterCentres(x, k).astype(np.float64)
    span = (x.max(axis=0).astype(np.float64) - x.min(axis=0)) / (float(np.iinfo(dt).max) - np.iinfo(dt).min)
    assert span.min() > 0.5
    wrapped = bool(((x.max(axis=0) - x.min(axis=0)).astype(np.float64) != x.max(axis=0).astype(np.float64) - x.min(axis=0)).any())
    elk = same(oracle.kmeans_fit(x.astype(np.float64), init, algorithm='elkan'), ref)
    lloyd = same(oracle.kmeans_fit(x.astype(np.float64), init, algorithm='full'), ref)
    assert elk, 'the oracle differs from the reference on image case %d' % i
    p = 'i%02d_' % i
    out[p + 'img'] = img
    out[p + 'k'] = np.int32(k)
    out[p + 'has_null'] = np.int32(null is not None)
    out[p + 'null'] = np.int64(0 if null is None else null)
    store(out, p, ref, init)
    print('i%02d  %-7s nb=%d %dx%d k=%d null=%s rows=%d n_iter=%d bandMax-bandMin wrapped: %s  Lloyd restatement equals reference: %s' % (
        i, dt, nb, nr, nc, k, null, x.shape[0], ref[2], ('no', 'yes')[wrapped], ('no', 'yes')[lloyd]))
out['nimages'] = np.int32(len(IMAGES))

# ---- smooth cases ----------------------------------------------------------------------------------------------------
SMOOTH = (('uint32', 4, 60, 31), ('int32', 3, 61, 32))
print('smooth cases: 16-bit synthimg rows scaled to 32 bits plus low noise bits, 16 centres = sample rows + 0.375')
for (i, (dt, nb, sseed, nseed)) in enumerate(SMOOTH):
    xs = fw.smooth(oracle.synthimg(sseed, nb, 300, 300), dt, nb, nseed)
    init = fw.smooth_init(xs)
    ref = reference_rows(xs, init)
    elk = same(oracle.kmeans_fit(xs.astype(np.float64), init, algorithm='elkan'), ref)
    lloyd = same(oracle.kmeans_fit(xs.astype(np.float64), init, algorithm='full'), ref)
    assert elk, 'the oracle differs from the reference on smooth case %d' % i
    p = 's%02d_' % i
    out[p + 'recipe'] = np.array([nb, sseed, nseed], dtype=np.int64)
    out[p + 'dtype'] = np.array(dt)
    out[p + 'crc'] = fw.crc(xs)
    store(out, p, ref, init)
    print('s%02d  %-7s nb=%d n=%d min=%d max=%d n_iter=%d  Lloyd restatement equals reference: %s' % (
        i, dt, nb, xs.shape[0], xs.min(), xs.max(), ref[2], ('no', 'yes')[lloyd]))
out['nsmooth'] = np.int32(len(SMOOTH))
out['stack'] = np.array(refenv.STACK)
path = os.path.join(ROOT, 'tests', 'golden', 'kmeans_fit_wide.npz')
np.savez_compressed(path, **out)
print('wrote tests/golden/kmeans_fit_wide.npz: %d bytes' % os.path.getsize(path))
