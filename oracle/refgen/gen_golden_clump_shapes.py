"""tests/golden/clump_shapes.npz from the UNMODIFIED reference: its clump() on the shapes of
tests/clump_shape_cases.py (which this script imports, so that the tests build the same inputs), both
connectivities.

    cd oracle/refgen && /opt/conda/bin/python3.9 gen_golden_clump_shapes.py

Per (shape, connectivity) the file holds the next id ('<shape>/<4|8>/next') and the SHA-256 of the uint32 label
image's bytes in row order ('<shape>/<4|8>/sha256', 32 bytes); the shapes themselves are recipes, not data.  The
label images of percolation, lattice3 and rect_widths (4-connected) and of percolation8 (8-connected) are stored
whole ('<shape>/<4|8>/labels') so that a mismatch there can be located; compressed, the file stays below the
largest fixture of tests/golden.  Build container only (refenv.py)."""
import hashlib
import os
import sys

import numpy as np

import refenv  # noqa: F401
from refenv import shepseg

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import clump_shape_cases as cs  # noqa: E402

WHOLE = {('percolation', True), ('lattice3', True), ('rect_widths', True), ('percolation8', False)}

out = {}
for name in cs.SHAPES:
    cl = np.array(cs.make(name))
    for four in (True, False):
        seg, nxt = shepseg.clump(cl, shepseg.SEGNULLVAL, fourConnected=four, clumpId=shepseg.MINSEGID)
        seg = np.ascontiguousarray(seg, dtype=np.uint32)
        key = '%s/%d/' % (name, 4 if four else 8)
        out[key + 'next'] = np.int64(nxt)
        out[key + 'sha256'] = np.frombuffer(hashlib.sha256(seg.tobytes()).digest(), dtype=np.uint8)
        if (name, four) in WHOLE:
            out[key + 'labels'] = seg
        print(key, int(nxt), seg.shape)
path = os.path.join(ROOT, 'tests', 'golden', 'clump_shapes.npz')
np.savez_compressed(path, **out)
print(refenv.STACK, os.path.getsize(path), 'bytes')
