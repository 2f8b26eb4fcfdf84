"""CPU: the walker batcher (pyshepseg_amd/csrc/walkbatch.h) driven by a host-only program with a fake launch
(tests/native/walkbatch_host.cpp), built with ThreadSanitizer -- or AddressSanitizer + UBSan where that runtime
cannot start.  The program has its own main: nothing is preloaded and nothing is loaded into Python.  It asserts
that every job ran exactly once, that no batch mixes classes or exceeds the job, block and residency caps, that
the batch after a held launch carries all pending jobs of its class, that a launch error reaches exactly its
batch and a per-job failure only its job, that the workgroup counters hold the sum over the submitted jobs and
the largest launch, that in rounds of unequal workgroup counts a replay above the block cap runs once and alone
while the leader that skips it still takes every job that fits, and it ends within its own 30-s alarm."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'native', 'walkbatch_host.cpp')
PROBE = 'int main() { return 0; }\n'


def _compiler():
    for cxx in (os.environ.get('CXX'), 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def _usable(cxx, flags, tmp_path):
    """the sanitizer links and its runtime starts on this machine"""
    probe = tmp_path / 'probe.cpp'
    probe.write_text(PROBE)
    exe = str(tmp_path / 'probe')
    if subprocess.run([cxx] + flags + ['-o', exe, str(probe)], capture_output=True).returncode != 0:
        return False
    return subprocess.run([exe], capture_output=True).returncode == 0


def test_walk_batcher_under_sanitizer(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no C++ compiler')
    for flags in (['-fsanitize=thread'], ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']):
        if _usable(cxx, flags + ['-pthread'], tmp_path):
            break
    else:
        pytest.skip('the toolchain has neither ThreadSanitizer nor AddressSanitizer')
    exe = str(tmp_path / 'walkbatch_host')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-pthread'] + flags + ['-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, '%s\n%s' % (' '.join(flags), p.stderr[-4000:])
    assert p.stdout.strip() == 'ok'
    print('sanitizer:', ' '.join(flags))
