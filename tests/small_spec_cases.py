"""Rasters and the CPU census of the pass-loop instance tests (csrc/elim_small.h k_small_loop<NB, CONN, DIAG>):
tests/test_small_spec_census.py pins on the CPU what tests/test_gpu_small_spec.py relies on.

A case is one synthetic tile (oracle.synthimg, centres picked along the raster), its band count, connectivity and
minSegmentSize, and the instance its pass loop must take (the order of shp_small_loop_instances: generic, 6 bands
4- and 8-connected, 10 bands 4- and 8-connected).  What a find does depends on the pairs (pixel, neighbour) of a
source, target size x 4 or x 8: up to 128 several sources share a batch, up to 256 a batch still takes them (a
wavefront per source when the pass has few sources), above 256 a wavefront handles one source.  The merge step
relabels with a thread per source up to target 16 and a wavefront per source above.  A pass at some target in a range
is proven by the oracle alone: the elimination goes through the targets in ascending order, so the run with
minSegmentSize = hi + 1 eliminates more segments than the run with minSegmentSize = lo exactly when a pass with a
target in lo .. hi merged something."""
import numpy as np

import seg_cases

GENERIC, B6_C4, B6_C8, B10_C4, B10_C8 = range(5)
NR, NC = 300, 333           # one tile window, neither a multiple of 64

# (id, bands, four-connected, minSegmentSize, instance)
CASES = [
    ('b6_c4', 6, True, 70, B6_C4),
    ('b6_c8', 6, False, 40, B6_C8),
    ('b10_c4', 10, True, 70, B10_C4),
    ('b10_c8', 10, False, 40, B10_C8),
    ('b3_c4', 3, True, 70, GENERIC),
    ('b9_c8', 9, False, 40, GENERIC),
]
# the size-table scan: minSegmentSize above 256 turns the per-size lists off; the larger tile gives the first
# pass more than SMALL_BALANCED_MAX sources (the unbalanced branch), the late passes have few (the balanced one)
SCAN = ('b6_c4_scan', 6, True, 260, B6_C4)
SCAN_NR, SCAN_NC = 900, 1000
SMALL_BALANCED_MAX = 2048   # csrc/elim_small.h

_tiles = {}
_runs = {}


def tile(oracle, nb, scan=False):
    """(img, centres, maxSpectralDiff) of the case's raster"""
    key = (nb, scan)
    if key not in _tiles:
        from pyshepseg_amd import shepseg
        (nr, nc) = (SCAN_NR, SCAN_NC) if scan else (NR, NC)
        img, centres = seg_cases.synth_tile(oracle, 40 + nb, nr, nc, nb=nb, k=24)
        msd = float(shepseg.autoMaxSpectralDiff(shepseg.KMeansModel(centres), 'auto', 50))
        _tiles[key] = (img, centres, msd)
    return _tiles[key]


def oracle_run(oracle, nb, four, minseg, scan=False):
    """the oracle's result for the case's raster at `minseg` (computed once)"""
    key = (nb, bool(four), minseg, scan)
    if key not in _runs:
        img, centres, msd = tile(oracle, nb, scan)
        _runs[key] = oracle.segment_tile(img, centres, minseg, msd, None, four)
    return _runs[key]


def eliminated(oracle, nb, four, minseg, scan=False):
    return int(oracle_run(oracle, nb, four, minseg, scan)['smallSegmentsEliminated'])


def pair_ranges(four, minseg):
    """target ranges (lo, hi) by what a find does there: <= 128 pairs, 129 .. 256, above"""
    nq = 4 if four else 8
    return [(2, 128 // nq), (128 // nq + 1, 256 // nq), (256 // nq + 1, minseg - 1)]
