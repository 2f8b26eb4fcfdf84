"""The 'packed' raster of tests/test_walk_batch_packed_census.py and tests/test_gpu_walk_batch_packed.py, what the
tests know about it without a GPU, and the child process that segments it.

By default a replay job is sized by its work (csrc/clump.h dfs_job_blocks): a tile of n components above the
depth-first cut's cap, of sum_px pixels together and max_px the largest, gets
    U = min(DFS_MAX_BLOCKS, ceil(n / DFS_WAVES))                          workgroups when n <= DFS_PACK_MIN,
    clamp(ceil(ceil(sum_px / (max_px * DFS_FILL)) / DFS_WAVES), 1, U)     otherwise,
and the components beyond its walkers are pulled from the job's counter.  packed_blocks() restates that;
census() gives it the component sizes of every tile window (clump_shape_cases.cut_components on the oracle's
cluster codes).

The raster is one row of five tile windows (tile 512, overlap 64).  Vertical stripes over the whole height: in
each of the first four windows one wide stripe (112, 70, 112, 91 columns: 57 344, 35 840, 57 344, 46 592 pixels)
and 16 to 18 stripes of 21 columns (10 752 pixels, just above the cap), plus the 64 columns of the next window's
wide stripe that the overlap shows; the last window holds 12 stripes of 48 columns and keeps a walker per
component.  Spectra, outliers and noise as in tests/walk_batch_worker.py.

As a program: walk_batch_packed.py OUT.npz FOUR WORKERS packed -- tests/walk_batch_worker.py's main() on this
raster and tiling."""
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import walk_batch_worker as wbw  # noqa: E402

NR, NC = 512, 2368
TILE, OVERLAP = 512, 64
NTILES = 5
WIDE = (112, 70, 112, 91)   # the wide stripe of each of the first four windows
NARROW, LAST = 21, 48
DFS_WAVES = 8               # csrc/clump.h
DFS_MAX_BLOCKS = 256        # csrc/clump.h
DFS_PACK_MIN = 2 * DFS_WAVES    # csrc/clump.h
DFS_FILL = 0.75             # csrc/clump.h (tests/test_walk_batch_packed_census.py compares it with the header)

_census = {}


def image_packed():
    """(img, centres) of the raster described above"""
    step = TILE - OVERLAP
    widths = []
    for w in WIDE:
        widths += [w] + [NARROW] * ((step - w) // NARROW)
    widths += [LAST] * ((NC - step * len(WIDE)) // LAST)
    assert sum(widths) == NC
    cl = np.repeat(1 + np.arange(len(widths)) % 2, widths)[None, :].repeat(NR, axis=0).astype(np.int32)
    rng = np.random.RandomState(35)
    flip = rng.rand(NR, NC) < 0.03
    cl[flip] = rng.randint(1, 6, size=int(flip.sum()))
    img = wbw.BASE[cl].transpose(2, 0, 1) + rng.randint(-40, 41, size=(3, NR, NC))
    return np.ascontiguousarray(np.clip(img, 1, 65535).astype(np.uint16)), wbw.BASE[1:].astype(np.float64)


def census(oracle, four):
    """per tile window in sorted tile-key order: the sizes of its components above the cap"""
    import clump_shape_cases
    if bool(four) not in _census:
        img, centres = image_packed()
        tiles, _ntc, _ntr = oracle.get_tiles(NR, NC, TILE, OVERLAP)
        sizes = []
        for k in sorted(tiles):
            (x, y, xs, ys) = tiles[k]
            sub = np.ascontiguousarray(img[:, y:y + ys, x:x + xs])
            cl = oracle.kmeans_assign(sub, centres).astype(np.int32)
            sizes.append([n for (*_box, n) in clump_shape_cases.cut_components(cl, four)])
        _census[bool(four)] = sizes
    return _census[bool(four)]


def unpacked_blocks(n, per_wg=DFS_WAVES):
    """a workgroup per `per_wg` components: every job under SHEPSEG_DFS_PER_WG, the small ones without"""
    return min(DFS_MAX_BLOCKS, -(-n // per_wg))


def packed_blocks(sizes, fill=DFS_FILL):
    """workgroups of the replay job of a tile with these component sizes, SHEPSEG_DFS_PER_WG not set"""
    n, u = len(sizes), unpacked_blocks(len(sizes))
    if n <= DFS_PACK_MIN:
        return u
    walkers = math.ceil(float(sum(sizes)) / (float(max(sizes)) * fill))
    return max(1, min(u, -(-walkers // DFS_WAVES)))


if __name__ == '__main__':
    wbw.TILE, wbw.OVERLAP = TILE, OVERLAP
    wbw.IMAGES['packed'] = image_packed
    wbw.main()
