"""The definition of the segment-neighbour table in numpy, and the label rasters the tests put through it.

Two pixels are adjacent when they are E or S neighbours (8-connected: SE and SW as well); every adjacent pair
with labels a != b, both non-zero, adds 1 to the border length of (a, b) and of (b, a).  The table is CSR over
the ids 0 .. maxSegId."""
import numpy as np

EXAMPLE = np.array([[1, 1, 2], [1, 3, 2], [0, 3, 3]], dtype=np.uint32)
EXAMPLE_OFFSETS = [0, 0, 2, 4, 6]
EXAMPLE_NEIGHBOURS = [2, 3, 1, 3, 1, 2]
EXAMPLE_LENGTHS = {True: [1, 2, 1, 2, 2, 2], False: [2, 4, 2, 4, 4, 4]}


def reference_neighbours(seg, fourConnected=True, maxSegId=None):
    """(offsets int64 [maxSegId + 2], neighbours uint32, borderLengths int64)"""
    seg = np.asarray(seg)
    assert seg.ndim == 2 and seg.dtype == np.uint32
    if maxSegId is None:
        maxSegId = int(seg.max()) if seg.size else 0
    pairs = [(seg[:, :-1], seg[:, 1:]), (seg[:-1], seg[1:])]
    if not fourConnected:
        pairs += [(seg[:-1, :-1], seg[1:, 1:]), (seg[:-1, 1:], seg[1:, :-1])]
    a = np.concatenate([p[0].ravel() for p in pairs]).astype(np.uint64)
    b = np.concatenate([p[1].ravel() for p in pairs]).astype(np.uint64)
    keep = (a != b) & (a != 0) & (b != 0)
    (a, b) = (a[keep], b[keep])
    (u, cnt) = np.unique(np.concatenate([(a << np.uint64(32)) | b, (b << np.uint64(32)) | a]), return_counts=True)
    offsets = np.zeros(maxSegId + 2, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount((u >> np.uint64(32)).astype(np.int64), minlength=maxSegId + 1))
    return (offsets, (u & np.uint64(0xFFFFFFFF)).astype(np.uint32), cnt.astype(np.int64))


def random_labels(shape, top, seed):
    """uniform labels 0 .. top"""
    return np.random.default_rng(seed).integers(0, top + 1, size=shape, dtype=np.uint32)


OFF_GRID_SHAPES = [(1, 1), (1, 257), (257, 1), (2, 2), (33, 65), (65, 129)]


def every_pixel_its_own():
    return np.arange(1, 70 * 130 + 1, dtype=np.uint32).reshape(70, 130)


def half_planes():
    seg = np.ones((300, 300), dtype=np.uint32)
    seg[150:] = 2
    return seg


def stripes():
    seg = np.empty((257, 300), dtype=np.uint32)
    seg[:, 0::2] = 1
    seg[:, 1::2] = 2
    return seg


def hot_segment():
    seg = np.ones((300, 300), dtype=np.uint32)
    (ys, xs) = np.meshgrid(np.arange(1, 300, 2), np.arange(1, 300, 2), indexing='ij')
    seg[ys, xs] = np.arange(2, 2 + ys.size, dtype=np.uint32).reshape(ys.shape)
    return seg


SPARSE_IDS = np.array([0, 5, 70000, 1 << 20], dtype=np.uint32)
SPARSE_MAX = (1 << 20) + 3


def sparse_ids():
    return SPARSE_IDS[np.random.default_rng(5).integers(0, 4, size=(90, 140))]


def enclosed_by_zeros():
    seg = np.zeros((40, 70), dtype=np.uint32)
    seg[10:20, 10:30] = 3          # touches nothing but zeros
    seg[25:35, 40:50] = 1
    seg[25:35, 50:66] = 2          # 1 and 2 touch each other
    return seg
