"""The external-semantics calls of the C++ Segmenter facade (include/rvseg_segmenter.hpp: Config::external_semantics,
externalRequest, processFramesExternal) compiled with g++ against librvseg.so: one small case, compared with the C ABI's
own output through the Python binding (which test_gpu_external.py pins to the oracle)."""
import os
import subprocess

import numpy as np
import pytest

import external_cases as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_external_semantics(tmp_path, gpu_ctx_factory):
    exe = str(tmp_path / "external")
    lib_dir = os.path.join(ROOT, "rovinasemanticsegmentation_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "external_semantics_test.cpp"), "-o", exe,
                           "-L", lib_dir, "-lrvseg", "-lpthread", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, layers = 160, 120, (3, 5)
    N, S = W * H, sum(layers)
    rgb, depth = X.frames(2, W, H)
    rgb, depth = rgb[:1], depth[:1]
    dist = X.log_softmax_distributions(29, 1, layers, H, W)
    (tmp_path / "rgb.u8").write_bytes(rgb.tobytes())
    (tmp_path / "depth.u16").write_bytes(depth.tobytes())
    (tmp_path / "dist.f32").write_bytes(dist.tobytes())
    out_path = str(tmp_path / "out.bin")
    r = subprocess.run([exe, str(tmp_path / "rgb.u8"), str(tmp_path / "depth.u16"), str(tmp_path / "dist.f32"), out_path],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "external ok" in r.stdout
    raw = np.fromfile(out_path, np.uint8)
    assert raw.size == N * 12 + N * S * 4 + N * 2
    xyz, marg, lab = raw[:N * 12], raw[N * 12:N * 12 + N * S * 4], raw[N * 12 + N * S * 4:]

    fx = np.float32(525.0) * np.float32(W) / np.float32(640.0)     # the calibration the C++ program builds, in its float arithmetic
    one = np.float32(1)
    calib = np.array([one / fx, 0, -(np.float32(W) / np.float32(2)) / fx, 0, one / fx, -(np.float32(H) / np.float32(2)) / fx, 0, 0, 1,
                      0, 0, 1, -1, 0, 0, 0, -1, 0, 0.1, -0.2, 0.6], np.float32)
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=3, label_mode=X.LABEL_CRF, unknown_label=(2, 4))
    ctx.external_layers_set(layers)
    assert ctx.rectify_depth(depth, calib).tobytes() == xyz.tobytes()
    want = ctx.segment_external(rgb, depth, calib, dist)
    assert want["marginals"].tobytes() == marg.tobytes()
    assert want["labels"].tobytes() == lab.tobytes()
    # and the C ABI's output is the oracle's
    want_marg, want_lab = X.expected(rgb, depth, calib[None], dist, layers, W, H, X.LABEL_CRF, (2, 4))
    assert np.array_equal(want["marginals"].view(np.uint32), want_marg.view(np.uint32))
    assert np.array_equal(want["labels"].reshape(want_lab.shape), want_lab)
