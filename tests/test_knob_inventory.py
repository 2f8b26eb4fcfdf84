"""CPU: every SHEPSEG_* knob the project reads is accounted for -- in the knob matrix of
tests/test_gpu_knob_paths.py, in a named existing test, or in the list of diagnostics and process
plumbing -- and every knob that is not a diagnostic is in the README's knob table."""
import glob
import os
import re

from conftest import ROOT

# knob -> the test that sets it (its file must name the knob)
TESTED_ELSEWHERE = {
    'SHEPSEG_STATS_PATCH': 'tests/test_gpu_stats.py::test_stats_patch_path_dtypes',
    'SHEPSEG_CLUSTER_MAP': 'tests/test_gpu_tiling.py::test_knobs_off_paths_match',
    'SHEPSEG_STREAM_INPUT': 'tests/test_gpu_tiling.py::test_streamed_input_and_output_match_the_per_tile_path',
    'SHEPSEG_ELK_TABLE': 'tests/test_fit_elkan.py',
    'SHEPSEG_ELK_UNFUSED': 'tests/test_fit_elkan.py',
    'SHEPSEG_FIT_ALGO': 'tests/test_fit_elkan.py',
    'SHEPSEG_FIT_SHARDS': 'tests/test_fit_elkan.py',
    'SHEPSEG_FIT_CHECK_DIGITS': 'tests/test_fit_elkan.py',
    'SHEPSEG_FIT_PLANAR': 'tests/test_gpu_tile.py',
    'SHEPSEG_STITCH': 'tests/test_gpu_distributed.py',
    'SHEPSEG_SHARD': 'tests/test_distributed_cpu.py',
    'SHEPSEG_CHAIN_ORDER': 'tests/test_distributed_cpu.py',
}

# timing and trace output, and knobs that give wrong labels by design (never parity-tested)
DIAGNOSTICS = {
    'SHEPSEG_DFS_STATS', 'SHEPSEG_SMALL_TIMING', 'SHEPSEG_FIT_TIMING', 'SHEPSEG_FIT_TRACE', 'SHEPSEG_IO_TIMING',
    'SHEPSEG_CHAIN_TIMING', 'SHEPSEG_REGROW_LOG', 'SHEPSEG_FIT_SHARD_ONLY',
    'SHEPSEG_DBG_SKIP_DFS', 'SHEPSEG_DBG_SKIP_SMALL',
}

# where and how the process runs, not which kernel path computes the labels
PLUMBING = {
    'SHEPSEG_LIBPATH', 'SHEPSEG_DEVICE', 'SHEPSEG_COMM', 'SHEPSEG_COMM_DIR', 'SHEPSEG_LAUNCH_NONCE',
    'SHEPSEG_FORCE_DIST', 'SHEPSEG_FIT_SHARDED', 'SHEPSEG_DEVCACHE_GB', 'SHEPSEG_STREAM_ROWS',
    'SHEPSEG_STREAM_READERS', 'SHEPSEG_STREAM_WRITERS',
}


def _read(path):
    with open(path) as f:
        return f.read()


def knobs_read():
    found = set()
    for p in glob.glob(os.path.join(ROOT, 'pyshepseg_amd', 'csrc', '*')):
        found |= set(re.findall(r'getenv\(\s*"(SHEPSEG_[A-Z0-9_]+)"', _read(p)))
    for p in glob.glob(os.path.join(ROOT, 'pyshepseg_amd', '*.py')):
        found |= set(re.findall(r'environ(?:\.get\(\s*|\[\s*)[\'"](SHEPSEG_[A-Z0-9_]+)[\'"]', _read(p)))
        found |= set(re.findall(r'getenv\(\s*[\'"](SHEPSEG_[A-Z0-9_]+)[\'"]', _read(p)))
    return found


def matrix_knobs():
    import knob_cases
    return {k for _name, env, _cases in knob_cases.MATRIX for k in env}


def test_every_knob_is_accounted_for_once():
    found = knobs_read()
    assert 'SHEPSEG_SCAN_ONE' in found and 'SHEPSEG_TILE_ORDER' in found and 'SHEPSEG_LIBPATH' in found
    groups = {'matrix': matrix_knobs(), 'tested elsewhere': set(TESTED_ELSEWHERE), 'diagnostics': DIAGNOSTICS,
              'plumbing': PLUMBING}
    for k in sorted(found):
        where = [g for g, s in groups.items() if k in s]
        assert len(where) == 1, '%s is in %s: a knob belongs to exactly one group' % (k, where or 'no group')
    stale = set().union(*groups.values()) - found
    assert not stale, 'knobs listed but no longer read: %s' % sorted(stale)


def test_tested_elsewhere_names_real_tests():
    for k, t in TESTED_ELSEWHERE.items():
        path, _, name = t.partition('::')
        src = _read(os.path.join(ROOT, path))
        assert k in src, '%s does not set %s' % (path, k)
        if name:
            assert re.search(r'def %s\(' % name, src), t


def test_non_diagnostic_knobs_are_documented():
    readme = _read(os.path.join(ROOT, 'README.md'))
    table = set()
    for row in re.findall(r'^\|([^|\n]*)\|', readme, flags=re.M):    # the first cell of every table row
        names = re.findall(r'`(SHEPSEG_[A-Z0-9_]+|_[A-Z0-9_]+)`', row)
        for n in names:                                               # `SHEPSEG_X_ROWS` / `_READERS`: X_READERS
            table.add(n if n.startswith('SHEPSEG_') else names[0].rsplit('_', 1)[0] + n)
    missing = sorted(k for k in knobs_read() - DIAGNOSTICS if k not in table)
    assert not missing, 'not in the README knob table: %s' % missing
