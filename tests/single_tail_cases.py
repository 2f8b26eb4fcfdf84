"""Tiles for the later passes of the single-pixel stage (csrc/elim_single.h k_single_tail), built so that the stage
runs many passes: a k x k block carries a 2 x 2 periodic pattern of four clusters, so each of its pixels is a
one-pixel clump in either connectivity, and it sits in a field of large uniform regions (a 3 x 3 board of three more
clusters), so the passes peel it one ring at a time.  Pixel values are a cluster's centre plus a few counts of noise:
the nearest neighbouring pixel is then not always the same one, and the rings split among the field's regions.

CASES names, per case, the tile, the block, the bands, the pixel type and the connectivity; model() is the reference's
loop (shepseg.py:572-736) in plain Python with the figures the census test asserts; run as a script it is the GPU
tests' child: python tests/single_tail_cases.py CASE OUT.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINSEG = 4            # below every segment left after the stage: the small-segment stage merges nothing
MSD = 100.0
TAIL_THREADS = 1024   # csrc/elim_single.h: k_single_tail's one workgroup; a longer list takes several rounds per thread

# per pixel type: (centre of cluster m in band b) = base + step * m + 3 * b; the 32-bit steps make one band's squared
# difference between far clusters pass 2^63, so the reference's int64 dSqr wraps
LEVELS = {
    'uint8': (20, 30), 'int16': (-12000, 4000), 'uint16': (1000, 9000),
    'int32': (-1800000000, 600000000), 'uint32': (1000, 600000000),
}
NOISE = 3
K = 7                 # clusters 0-3: the pattern; 4-6: the field

# name: (rows, cols, block (row, col, k) or None = patterned all over, bands, pixel type, four-connected, noise,
#        null pixels (row, col, rows, cols) or None)
CASES = {
    'k3':        (17, 19, (6, 7, 3), 6, 'uint16', True, True, None),
    'k8':        (33, 31, (11, 9, 8), 1, 'uint8', False, True, None),
    'k40':       (64, 61, (12, 10, 40), 6, 'uint16', True, True, None),
    'k40_eight': (64, 61, (12, 10, 40), 9, 'int16', False, True, None),
    'k36':       (57, 64, (10, 14, 36), 8, 'uint8', True, True, None),
    'k36_u32':   (57, 64, (10, 14, 36), 9, 'uint32', False, True, None),
    'all_over':  (40, 40, None, 6, 'uint16', True, True, None),
    'corner':    (24, 20, (0, 0, 8), 8, 'int32', True, True, None),
    'corner_br': (24, 20, (16, 12, 8), 6, 'uint16', False, True, None),
    'nulls':     (33, 31, (11, 9, 8), 6, 'uint16', False, True, (13, 6, 4, 3)),
    'one_null':  (33, 31, (11, 9, 8), 6, 'uint16', True, True, (14, 8, 1, 1)),
    'ties':      (33, 31, (11, 9, 8), 6, 'uint16', False, False, None),
    'flat_i32':  (33, 31, (11, 9, 8), 1, 'int32', True, False, None),
    'wrap_u32':  (33, 31, (11, 9, 8), 8, 'uint32', True, True, None),
}
NULLVAL = 0


def centres_of(nb, dtype):
    base, step = LEVELS[dtype]
    return np.array([[base + step * m + 3 * b for b in range(nb)] for m in range(K)], dtype=np.float64)


def build(name):
    """(img (bands, rows, cols), centres, null value or None, four-connected)"""
    (nr, nc, block, nb, dtype, four, noise, nulls) = CASES[name]
    r, c = np.mgrid[0:nr, 0:nc]
    clus = 4 + ((r * 3) // nr + (c * 3) // nc) % 3
    pat = 2 * (r % 2) + (c % 2)
    if block is None:
        clus = pat.copy()
        clus[nr // 2, nc // 2 + 1] = clus[nr // 2, nc // 2]      # a run of three: the one clump the peeling starts from
    else:
        (r0, c0, k) = block
        inb = (r >= r0) & (r < r0 + k) & (c >= c0) & (c < c0 + k)
        clus = np.where(inb, pat, clus)
    cen = centres_of(nb, dtype)
    rng = np.random.RandomState(sum(map(ord, name)))
    img = cen[clus].transpose(2, 0, 1).astype(np.int64)
    if noise:
        img += rng.randint(-NOISE, NOISE + 1, size=img.shape)
    if nulls is not None:
        (y, x, h, w) = nulls
        img[:, y:y + h, x:x + w] = NULLVAL
    return np.ascontiguousarray(img.astype(dtype)), cen, (NULLVAL if nulls is not None else None), four


def model(img, seg, four):
    """The reference's eliminateSinglePixels on (img, seg) in place.  Returns a dict: 'passes' = per pass that merged
    something (single pixels at its start, merged); 'total'; and whether any chosen target was segment 0, any minimum
    was shared by neighbours of two segments, any dSqr came out negative."""
    (nb, nr, nc) = img.shape
    im = img.astype(np.int64)
    size = np.bincount(seg.ravel(), minlength=int(seg.max()) + 1).astype(np.int64)
    out = {'passes': [], 'total': 0, 'target0': False, 'tie': False, 'negative': False}
    while True:
        cand = [(i, j) for (i, j) in zip(*np.nonzero(size[seg] == 1))]
        todo = []
        for (i, j) in cand:
            mind, best, bestseg = -1, None, None
            for ii in range(max(i - 1, 0), min(i + 1, nr - 1) + 1):
                for jj in range(max(j - 1, 0), min(j + 1, nc - 1) + 1):
                    if four and ii != i and jj != j:
                        continue
                    if size[seg[ii, jj]] > 1:
                        with np.errstate(over='ignore'):
                            d = int(((im[:, i, j] - im[:, ii, jj]) ** 2).sum())       # int64, wraps
                        out['negative'] |= d < 0
                        if mind >= 0 and d == mind and seg[ii, jj] != bestseg:
                            out['tie'] = True
                        if mind < 0 or d < mind:
                            mind, best, bestseg = d, (ii, jj), seg[ii, jj]
            if best is not None:
                todo.append((i, j, seg[best]))
        if not todo:
            break
        out['passes'].append((len(cand), len(todo)))
        for (i, j, t) in todo:
            out['target0'] |= int(t) == 0
            size[seg[i, j]] = 0
            seg[i, j] = t
            size[t] += 1
        out['total'] += len(todo)
    return out


def main():
    (name, outp) = sys.argv[1:3]
    sys.path.insert(0, ROOT)
    from pyshepseg_amd import shepseg
    img, cen, nullv, four = build(name)
    r = shepseg.doShepherdSegmentation(img, minSegmentSize=MINSEG, maxSpectralDiff=MSD, imgNullVal=nullv,
                                       fourConnected=four, kmeansObj=shepseg.KMeansModel(cen))
    np.savez(outp, seg=r.segimg, max_seg_id=int(r.segimg.max()), singles=int(r.singlePixelsEliminated),
             small=int(r.smallSegmentsEliminated))


if __name__ == '__main__':
    main()
