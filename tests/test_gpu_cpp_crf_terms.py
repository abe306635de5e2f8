"""The dense_learning recipe through the C++ facade (rvseg::DenseCRF2D / rvseg::DenseCRF in include/rvseg_segmenter.hpp),
compiled with g++ against librvseg.so and compared bit for bit with the restatement (tests/cpp/crf_terms_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import crf_restate as R
from test_gpu_crf_terms import dense_learning_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_dense_learning_recipe(tmp_path, oracle, golden_dir):
    from rovinasemanticsegmentation_amd import _capi as capi
    exe = str(tmp_path / "crf_terms")
    lib_dir = os.path.join(ROOT, "rovinasemanticsegmentation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "crf_terms_test.cpp"), "-o", exe,
                           "-L", lib_dir, "-lrvseg", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    im, W, H, N, L, feat, m, kp_bil = dense_learning_inputs(golden_dir)
    M = L.shape[0]
    params = tmp_path / "params.bin"
    params.write_bytes(np.int32(M).tobytes() + L.tobytes() + m.tobytes() + kp_bil.tobytes())
    out = tmp_path / "out.bin"
    r = subprocess.run([exe, os.path.join(golden_dir, "im2.ppm"), str(params), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "crf terms ok" in r.stdout
    raw = out.read_bytes()
    Q = np.frombuffer(raw[:N * M * 4], np.float32).reshape(N, M)
    mp = np.frombuffer(raw[N * M * 4:], np.int8)
    fg = capi.crf_features_gaussian(W, H, 3, 3)
    fb = capi.crf_features_bilateral(W, H, 80, 80, 13, 13, 13, im)
    want = R.crf_terms(oracle, R.logistic_unary(L, feat),
                       [(fg, R.POTTS, [1.0], R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, np.ones(2, np.float32)),
                        (fb, R.MATRIX, m, R.DIAG_KERNEL, R.NORMALIZE_SYMMETRIC, kp_bil)], 5)
    assert np.array_equal(Q, want)
    assert np.array_equal(mp, oracle.labels(want, M, 3))
