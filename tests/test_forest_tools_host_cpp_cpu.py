"""The forest tools' host rules alone under the host sanitizers: tests/cpp/forest_tools_host_test.cpp (its own main) over
csrc/forest_tools_host.h (the score formulas, the leaf order, the refit's head rules and serialisation) with
csrc/forest_model.cpp compiled in, built with g++ -fsanitize=address,undefined and run directly.  No GPU, no library,
nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_forest_tools_host_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "forest_tools_host_test")
    csrc = os.path.join(ROOT, "rovinasemanticsegmentation_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-ffp-contract=off", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "forest_tools_host_test.cpp"),
                           os.path.join(csrc, "forest_model.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "forest tools host ok" in r.stdout
