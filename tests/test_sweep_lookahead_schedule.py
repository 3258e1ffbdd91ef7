"""The index schedule of the two-trip look-ahead loop of the merged sweep (stainlib_amd/csrc/sweep_lookahead.hpp), on the CPU: the
driver instantiates on the host with counting functors, tests/sweep_lookahead_schedule.cpp drives it over ranges around the trip edges
and compares every lane's sequence of (first reader, arithmetic, end of trip) events with the loop it replaced.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_lookahead_wave_sweep_index_schedule(tmp_path):
    cxx = _host_compiler()
    assert cxx is not None, "no host C++ compiler found (set CXX)"
    exe = str(tmp_path / "sweep_lookahead_schedule")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas",os.path.join(HERE, "sweep_lookahead_schedule.cpp"), "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout + cc.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout
