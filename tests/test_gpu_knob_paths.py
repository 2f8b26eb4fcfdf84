"""The kernel paths the SHEPSEG_* knobs select, against the oracle (matrix: tests/knob_cases.py).

The library reads these knobs once per process, so every setting runs in a fresh child process
(tests/knob_worker.py), one child at a time.  A child that ends abnormally fails its setting, and every
later setting fails without being started."""
import os
import subprocess
import sys

import numpy as np
import pytest

import knob_cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

WORKER = os.path.join(ROOT, 'tests', 'knob_worker.py')
_abnormal = []          # the first child that crashed or timed out


@pytest.fixture(scope='module')
def want(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = knob_cases.expected(name, oracle)
        return cache[name]
    return get


@pytest.mark.parametrize('setting,env,cases', knob_cases.MATRIX, ids=[m[0] for m in knob_cases.MATRIX])
def test_knob_setting_matches_oracle(setting, env, cases, want, tmp_path):
    if _abnormal:
        pytest.fail('not started: child %s ended abnormally' % _abnormal[0])
    out = str(tmp_path / 'out.npz')
    child_env = dict(os.environ, **env)
    timeout = 120 + 60 * len(cases)
    try:
        p = subprocess.run([sys.executable, WORKER, out, str(tmp_path)] + list(cases), env=child_env,
                           cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _abnormal.append('%s (timeout after %d s)' % (setting, timeout))
        pytest.fail('child %s timed out after %d s' % (setting, timeout))
    if p.returncode < 0 or p.returncode in (134, 139):
        _abnormal.append('%s (exit %d)' % (setting, p.returncode))
    assert p.returncode == 0, 'child %s (%s) exit %d:\n%s' % (setting, env, p.returncode, p.stderr[-3000:])
    with np.load(out) as got:
        for name in cases:
            for k, w in want(name).items():
                key = '%s/%s' % (name, k)
                assert key in got.files, key
                assert knob_cases.same(got[key], np.asarray(w)), '%s: %s differs from the oracle' % (setting, key)


def test_large_tile_recursive_scan(oracle):
    """A window above 8192 x 8192 pixels: its pixel-count scans take scan_exclusive's two-launch, recursive
    branch with default knobs (more than 8192 blocks of 8192 items), and the lazy block offsets its
    consumers read come from that recursion."""
    from pyshepseg_amd import shepseg
    nr, nc = 8200, 8200
    rng = np.random.RandomState(5)
    cl = np.kron(rng.randint(1, 9, size=(nr // 8 + 1, nc // 8 + 1)), np.ones((8, 8), dtype=np.int64))
    cl = np.ascontiguousarray(cl[:nr, :nc], dtype=np.int32)
    cl[rng.rand(nr, nc) < 0.02] = 0
    assert nr * nc > 8192 * 8192
    seg, nxt = shepseg.clump(cl, 0, fourConnected=True)
    oseg, onxt = oracle.clump(cl, 0, True, 1)
    assert nxt == onxt
    assert np.array_equal(seg, oseg)
