"""Timings of the subset recode on row shards (distributed.deviceSubset; pyshepseg_amd/csrc/subset.h), on a
device-resident N x N raster of 8 x 8 block labels (shp_dev_block_labels) and the window (100, 100, N - 200,
N - 200) visited in 1024-pixel tiles:

  one GPU     shp_subset_recode_dev of the whole window;
  W = 1, 2, 4 row shards played one after the other on ONE GPU (each rank a context of its own; shard
              boundaries 3 rows past r * N / W, so every boundary cuts a row of subset tiles):
              shp_dsubset_local_dev per rank (synchronised), the exchange played as device copies into one
              gathered buffer and its bytes, shp_dsubset_merge_dev per rank (recoding its rows of the window).
              The stacked rows, origSegIds and summed histograms are checked against the one-GPU result.

    python tools/perf_subset_dist.py [N=16000] [REPS=3]"""
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from pyshepseg_amd import distributed, _lib  # noqa: E402

TILE = 1024
MARGIN = 100


def alloc(c, nbytes):
    p = ctypes.c_void_p()
    c.check(c._L.shp_dev_alloc(c.handle, max(int(nbytes), 16), ctypes.byref(p)))
    return p


def main(N, REPS):
    c = _lib.Context()
    L = c._L
    d_seg = alloc(c, N * N * 4)
    S = ctypes.c_uint32(0)
    c.check(L.shp_dev_block_labels(c.handle, N, N, 8, 8, d_seg, ctypes.byref(S)))
    S = S.value
    (tlx, tly, xs, ys) = (MARGIN, MARGIN, N - 2 * MARGIN, N - 2 * MARGIN)
    npx = xs * ys
    d_out = alloc(c, npx * 4)
    cap = S + 1
    (orig1, hist1) = (np.zeros(cap, np.uint32), np.zeros(cap, np.uint32))
    nn = ctypes.c_uint32(0)
    best = 1e30
    for _r in range(REPS):
        t0 = time.perf_counter()
        c.check(L.shp_subset_recode_dev(c.handle, d_seg, N, N, tlx, tly, xs, ys, None, TILE, S, d_out,
                                        _lib.ptr(orig1), _lib.ptr(hist1), cap, ctypes.byref(nn)))
        best = min(best, time.perf_counter() - t0)
    m1 = nn.value
    want = np.empty((ys, xs), np.uint32)
    c.check(L.shp_dev_download(c.handle, _lib.ptr(want), d_out, want.nbytes))
    print('%d x %d labels (8 x 8 blocks), %d segments; window %d x %d px, %d ids; one-GPU shp_subset_recode_dev: '
          '%.2f ms (%.0f GB/s at 13 B per window pixel)' % (N, N, S, xs, ys, m1, 1e3 * best,
                                                            13.0 * npx / best / 1e9))
    for W in (1, 2, 4):
        cuts = [0] + [r * N // W + 3 for r in range(1, W)] + [N]
        rr = [(cuts[r], cuts[r + 1]) for r in range(W)]
        pcs = [_lib.Context() for _r in range(W)]
        (tl, tm, tx) = ([1e30] * W, [1e30] * W, 1e30)
        for _rep in range(REPS):
            pairs = []
            for (r, (lo, hi)) in enumerate(rr):
                (p, n, bad) = (ctypes.c_void_p(), ctypes.c_int64(0), ctypes.c_int(0))
                t0 = time.perf_counter()
                pcs[r].check(L.shp_dsubset_local_dev(pcs[r].handle, ctypes.c_void_p(d_seg.value + lo * N * 4), hi - lo,
                                                     N, lo, S, tlx, tly, xs, ys, TILE, None, ctypes.byref(p),
                                                     ctypes.byref(n), ctypes.byref(bad)))
                tl[r] = min(tl[r], time.perf_counter() - t0)
                assert bad.value == 0
                pairs.append((p.value, n.value))
            slot = max(n for (_p, n) in pairs)
            d_all = alloc(c, W * slot * 8)
            t0 = time.perf_counter()
            for (r, (p, n)) in enumerate(pairs):
                # a rank's slot: its n keys, then its n ids (the copy of its pairs into the send buffer)
                c.check(L.shp_dev_copy(c.handle, ctypes.c_void_p(d_all.value + r * slot * 8), ctypes.c_void_p(p),
                                       n * 8))
            c.check(L.shp_sync(c.handle))
            tx = min(tx, time.perf_counter() - t0)
            cnts = np.array([n for (_p, n) in pairs], np.uint32)
            hcap = int(cnts.sum()) + 1
            hcap += hcap % 2
            histSum = np.zeros(hcap, np.int64)
            d_hist = alloc(c, hcap * 4)
            for (r, (lo, hi)) in enumerate(rr):
                (a, b) = distributed.subsetHeldRows((lo, hi), tly, ys)
                orig = np.zeros(hcap, np.uint32)
                nm = ctypes.c_uint32(0)
                t0 = time.perf_counter()
                pcs[r].check(L.shp_dsubset_merge_dev(pcs[r].handle, d_all, slot, W, _lib.ptr(cnts),
                                                     ctypes.c_void_p(d_seg.value + lo * N * 4), hi - lo, N, lo, S,
                                                     tlx, tly, xs, ys, TILE, None,
                                                     ctypes.c_void_p(d_out.value + a * xs * 4), d_hist,
                                                     _lib.ptr(orig), hcap, ctypes.byref(nm)))
                tm[r] = min(tm[r], time.perf_counter() - t0)
                h = np.zeros(hcap, np.uint32)
                c.check(L.shp_dev_download(c.handle, _lib.ptr(h), d_hist, h.nbytes))
                histSum += h
                assert nm.value == m1 and np.array_equal(orig[:m1 + 1], orig1[:m1 + 1]), (W, r)
            assert np.array_equal(histSum[:m1 + 1], hist1[:m1 + 1].astype(np.int64)), W
            c.check(L.shp_dev_free(c.handle, d_hist))
            c.check(L.shp_dev_free(c.handle, d_all))
        got = np.empty((ys, xs), np.uint32)
        c.check(L.shp_dev_download(c.handle, _lib.ptr(got), d_out, got.nbytes))
        assert np.array_equal(got, want), W
        print('W=%d shards %s: local per rank %s ms (max %.2f); exchange as device copies %.3f ms, %d pairs, '
              '%.2f MB; merge per rank %s ms (max %.2f); result == one GPU'
              % (W, rr, ' '.join('%.2f' % (1e3 * t) for t in tl), 1e3 * max(tl), 1e3 * tx, int(cnts.sum()),
                 8.0 * cnts.sum() / 1e6, ' '.join('%.2f' % (1e3 * t) for t in tm), 1e3 * max(tm)))
        for pc in pcs:
            pc.close()
    c.check(L.shp_dev_free(c.handle, d_out))
    c.check(L.shp_dev_free(c.handle, d_seg))
    c.close()


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 16000, int(sys.argv[2]) if len(sys.argv) > 2 else 3)
