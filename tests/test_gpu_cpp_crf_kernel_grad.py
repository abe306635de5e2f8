"""The kernel-parameter gradient through the C++ facade (rvseg::DenseCRF::gradient(.., &kernel_grad) and kernelGradient in
include/rvseg_segmenter.hpp), compiled with g++ against librvseg.so and compared with the C ABI's doubles rounded to fp32
(tests/cpp/crf_kernel_grad_test.cpp)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_crf_kernel_grad(tmp_path):
    exe = str(tmp_path / "crf_kernel_grad")
    lib_dir = os.path.join(ROOT, "rovinasemanticsegmentation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "crf_kernel_grad_test.cpp"), "-o", exe,
                           "-L", lib_dir, "-lrvseg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "crf kernel grad ok" in r.stdout
