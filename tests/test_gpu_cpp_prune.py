"""The C++ pruner (include/rvseg_segmenter.hpp: rvseg::RandomForestPrune) compiled with g++ against librvseg.so and run
on the golden forest_single.dat: tests/cpp/prune_test.cpp checks the run against the energies the library reports for its
states and that prune() leaves the best state's trees on the context."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_prune(tmp_path, golden_dir):
    exe = str(tmp_path / "prune")
    lib_dir = os.path.join(ROOT, "rovinasemanticsegmentation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prune_test.cpp"), "-o", exe,
                           "-L", lib_dir, "-lrvseg", "-lpthread", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe, os.path.join(golden_dir, "forest_single.dat")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "prune ok" in r.stdout
    assert r.stdout.count("iteration: ") == 9 and " temp: " in r.stdout
