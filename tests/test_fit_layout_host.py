"""CPU: the k-means fit's buffer layouts (pyshepseg_amd/csrc/fit_layout.h) checked by a host-only program
(tests/native/fit_layout_host.cpp) built with AddressSanitizer + UBSan.  The program has its own main: nothing is
preloaded and nothing is loaded into Python.  Over shapes that reach both Elkan forms, k on either side of 64,
nb above 64 and the benchmark's samples, and max_iter from 0 to the lazy form's limit, it asserts that the regions
of each buffer are disjoint and inside the total, that float64 / 64-bit regions are 8-aligned and the float32
brackets 256-aligned, that every total is the formula the allocation has always had, and that the sharded
E-step's in-place all-gather (world * ceil(n / world) words) fits the gap behind the first label array for every
world size of 2..64."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, 'tests', 'native', 'fit_layout_host.cpp')
PROBE = 'int main() { return 0; }\n'
FLAGS = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


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


def test_fit_layouts_under_sanitizer(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip('no C++ compiler')
    if not _usable(cxx, FLAGS, tmp_path):
        pytest.skip('the toolchain lacks AddressSanitizer')
    exe = str(tmp_path / 'fit_layout_host')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g'] + FLAGS + ['-o', exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-4000:]
    assert p.stdout.strip() == 'ok'
