"""The boosting rules of the host alone under the host sanitizers: tests/cpp/boost_host_test.cpp (its own main) over
csrc/train_host.h (boost_round: alpha, exp(alpha) and the stop rules; the round keys and uniform draws) and
csrc/forest_model.h (vote_label), built with g++ -fsanitize=address,undefined and run directly.  No GPU, no library,
nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_boost_host_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "boost_host_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-ffp-contract=off", "-I", os.path.join(ROOT, "rovinasemanticsegmentation_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "boost_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "boost host ok" in r.stdout
