"""Child process of tests/test_gpu_knob_paths.py: runs the named cases under the knobs of its own
environment and writes every output array to an .npz file.
Usage: knob_worker.py OUT.npz TMPDIR CASE [CASE ...]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import knob_cases  # noqa: E402
from oracle import oracle  # noqa: E402


def main():
    out, tmpdir, cases = sys.argv[1], sys.argv[2], sys.argv[3:]
    arrays = {}
    for name in cases:
        for k, v in knob_cases.run_case(name, oracle, tmpdir).items():
            arrays['%s/%s' % (name, k)] = np.asarray(v)
    np.savez(out, **arrays)


if __name__ == '__main__':
    main()
