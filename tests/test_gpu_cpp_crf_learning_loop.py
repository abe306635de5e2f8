"""The dense_learning recipe through the C++ facade (rvseg::DenseCRF2D, rvseg::CRFEnergy, rvseg::minimizeLBFGS in
include/rvseg_segmenter.hpp), compiled with g++ against librvseg.so (tests/cpp/crf_learning_loop_test.cpp).  The parameters it
learns are compared bit for bit with those of the same loop over the path that sets a fresh model for every evaluation
(crf_loop_cases.reference_loop), which this test runs and writes to tmp_path."""
import os
import subprocess

import pytest

from crf_loop_cases import reference_loop, scene

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("cpp") / "crf_learning_loop")
    lib_dir = os.path.join(ROOT, "rovinasemanticsegmentation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "crf_learning_loop_test.cpp"), "-o", path,
                           "-L", lib_dir, "-lrvseg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-pthread"])
    return path


@pytest.mark.parametrize("objective", ["iou", "loglikelihood"])
def test_cpp_crf_learning_loop(gpu_ctx_factory, exe, tmp_path, objective):
    import rovinasemanticsegmentation_amd as rv
    im, gt, f, L = scene()
    obj = rv.IntersectionOverUnion(gt) if objective == "iou" else rv.LogLikelihood(gt, 0.01)
    want = reference_loop(rv, gpu_ctx_factory(), obj, im, f, L)
    for name, a in (("im", im), ("gt", gt), ("f", f), ("L", L), ("want", want)):
        a.tofile(str(tmp_path / (name + ".bin")))
    r = subprocess.run([exe, str(tmp_path), objective], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "crf learning loop ok" in r.stdout
