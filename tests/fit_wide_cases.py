"""Samples of tests/golden/kmeans_fit_wide.npz: k-means samples and rasters that span the whole range of a
32-bit or 16-bit pixel type.  The golden stores each sample's recipe and crc32 and the reference's result, not
the sample (numpy's legacy RandomState stream is frozen); oracle/refgen/gen_golden_fit_wide.py and
tests/test_fit_wide.py both build the samples here."""
import zlib

import numpy as np

# the lattice row cases, (dtype, nb, k, n, levels): five per type, one-band samples among them; then k = 64 (the
# widest fused form), k > 64 (the table form), and few levels in many bands, where ties are most frequent.  The
# levels are ones at which samples with a near tie of the Elkan bounds (the generator's condition for k <= 64)
# turn up within a few dozen seeds.  Two name their seed: samples on which the LAST shift that elk2_exact
# replays decides the result (a bound recomputed one shift short moves labels and n_iter), found on the CPU with a
# model of the bracket's decisions built into a scratch copy of the oracle.
ROWS = (('int32', 3, 16, 8000, 7), ('int32', 2, 30, 8000, 25), ('int32', 6, 60, 14000, 5), ('int32', 1, 30, 4000, 300),
        ('int32', 4, 25, 10000, 40),
        ('uint32', 3, 12, 8000, 9), ('uint32', 2, 30, 8000, 25), ('uint32', 6, 60, 14000, 5), ('uint32', 5, 20, 6000, 7),
        ('uint32', 4, 25, 10000, 300),
        ('int16', 3, 12, 8000, 9), ('int16', 2, 30, 8000, 25), ('int16', 6, 60, 14000, 5), ('int16', 1, 30, 4000, 300),
        ('int16', 4, 25, 10000, 40),
        ('uint32', 3, 64, 7000, 9), ('int32', 4, 64, 7000, 11, 36007), ('int32', 2, 70, 7000, 14), ('uint32', 5, 65, 7000, 7),
        ('int16', 3, 96, 7000, 20), ('int16', 5, 40, 7000, 6), ('uint32', 4, 48, 7000, 6), ('int32', 5, 33, 7000, 5, 39014),
        ('uint32', 6, 50, 7000, 4))


def lattice(dtype, shape, levels, seed):
    """values lo + q//2 + randint(0, levels) * q with q = (hi - lo) // (levels + 1): `levels` distinct values
    per band from one end of the type to the other, so exact distance ties decide labels"""
    dt = np.dtype(dtype)
    (lo, hi) = (int(np.iinfo(dt).min), int(np.iinfo(dt).max))
    q = (hi - lo) // (levels + 1)
    v = lo + q // 2 + np.random.RandomState(seed).randint(0, levels, size=shape).astype(np.int64) * q
    assert v.min() >= lo and v.max() <= hi
    return v.astype(dt)


def lattice_image(dtype, nb, nr, nc, levels, seed, null=None, null_share=0.0):
    img = lattice(dtype, (nb, nr, nc), levels, seed)
    if null is not None:
        rng = np.random.RandomState(seed + 1)
        hit = rng.random_sample((nb, nr, nc)) < null_share / nb
        img[hit] = null
    return img


def smooth(synth, dtype, nb, noise_seed, noise_bits=5):
    """16-bit synthimg-like rows (every 5th pixel of a 300 x 300 raster) stretched over the whole 32-bit range, plus
    noise_bits random low bits: no lattice, no midpoint ties.  synth: the (nb, 300, 300) uint16 raster"""
    dt = np.dtype(dtype)
    rows = synth.reshape(nb, -1).T[::5].astype(np.int64)
    noise = np.random.RandomState(noise_seed).randint(0, 1 << noise_bits, size=rows.shape)
    scale = ((1 << 32) - (1 << noise_bits)) // int(rows.max() - rows.min())      # stretched over the whole type
    v = (rows - rows.min()) * scale + noise + int(np.iinfo(dt).min)
    assert v.min() >= np.iinfo(dt).min and v.max() <= np.iinfo(dt).max
    return v.astype(dt)


def smooth_init(xs, k=16):
    """distinct sample rows shifted by 0.375: no cluster starts empty, no integer midpoint ties"""
    u = np.unique(xs, axis=0)
    return u[np.linspace(0, len(u) - 1, k).astype(np.int64)].astype(np.float64) + 0.375


def crc(a):
    return np.int64(zlib.crc32(np.ascontiguousarray(a).tobytes()))
