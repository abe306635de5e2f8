"""The class-weighted split objective's host-side rules alone under the host sanitizers: tests/cpp/train_prior_host_test.cpp
(its own main) over csrc/train_host.h (the weight formula, the weighted entropy against fp32 values worked out by hand,
the refusals of a prior), built with g++ -fsanitize=address,undefined and run directly, exactly as train_host_test.cpp is.
No GPU, no library, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_train_prior_host_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "train_prior_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "rovinasemanticsegmentation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "train_prior_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "train prior host ok" in r.stdout
