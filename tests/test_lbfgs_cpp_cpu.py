"""The minimiser alone under the host sanitizers: tests/cpp/lbfgs_test.cpp (its own main) and csrc/rvseg_lbfgs.cpp, built with
g++ -fsanitize=address,undefined and run directly.  No GPU, no library, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_lbfgs_under_sanitizers(tmp_path):
    exe = str(tmp_path / "lbfgs_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall",
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "lbfgs_test.cpp"),
                           os.path.join(ROOT, "rovinasemanticsegmentation_amd", "csrc", "rvseg_lbfgs.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "lbfgs ok" in r.stdout
