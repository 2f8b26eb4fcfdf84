"""Helpers of the multi-rank output-stage tests (no tests here): an oracle engine that also serves
distributed.writeOutputDistributed (numpy), and a host simulation of the one-GPU driver's overview writes --
k_overview_window's index formula, tile by tile in chain (row-major) order, a later block over an earlier one."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from dist_oracle_engine import OracleEngine  # noqa: E402


class OutputOracleEngine(OracleEngine):
    """OracleEngine plus the output stage's engine methods, in numpy"""

    def outputRows(self, y0, y1):
        assert self.outLo <= y0 <= y1 <= self.outHi, (y0, y1, self.outLo, self.outHi)
        return self.out[y0 - self.outLo:y1 - self.outLo].copy()

    def overviewRects(self, table, npacked):
        flat = self.out.ravel()
        out = np.zeros(npacked, dtype=np.uint32)
        for (src0, rs, cs, nr, nc, dst0) in np.asarray(table, dtype=np.int64).tolist():
            idx = src0 + np.arange(nr)[:, None] * rs + np.arange(nc)[None, :] * cs
            assert idx.min() >= 0 and idx.max() < flat.size
            out[dst0:dst0 + nr * nc] = flat[idx].ravel()
        return out


def layerShape(nRows, nCols, lvl):
    return ((nRows + lvl - 1) // lvl, (nCols + lvl - 1) // lvl)


def simulateOverview(mosaic, tileInfo, overlapSize, lvl):
    """(layer, owner): the overview layer the one-GPU driver writes from ``mosaic`` at ``lvl`` and, per layer
    pixel, the row-major index of the last tile that wrote it (-1: none)"""
    from pyshepseg_amd import tiling
    (nRows, nCols) = mosaic.shape
    (ovh, ovw) = layerShape(nRows, nCols, lvl)
    layer = np.zeros((ovh, ovw), dtype=np.uint32)
    owner = np.full((ovh, ovw), -1, dtype=np.int64)
    o = lvl // 2
    for row in range(tileInfo.nrows):
        for col in range(tileInfo.ncols):
            (xpos, ypos, xs, ys) = tileInfo.getTile(col, row)
            (top, bottom, left, right, xout, yout) = tiling.trimmedWindow(tileInfo, col, row, xpos, ypos, xs, ys,
                                                                          overlapSize)
            (w, h) = (right - left, bottom - top)
            nsr = (h - o + lvl - 1) // lvl if h > o else 0
            nsc = (w - o + lvl - 1) // lvl if w > o else 0
            for r in range(nsr):
                dr = yout // lvl + r
                if dr >= ovh:
                    continue
                dc = xout // lvl + np.arange(nsc)
                keep = dc < ovw
                layer[dr, dc[keep]] = mosaic[yout + o + r * lvl, (xout + o + np.arange(nsc) * lvl)[keep]]
                owner[dr, dc[keep]] = row * tileInfo.ncols + col
    return layer, owner
