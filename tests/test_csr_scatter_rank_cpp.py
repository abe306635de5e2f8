"""tests/cpp/csr_scatter_rank_test.cpp: the chunk ranking of csr_scatter_kernel restated on the host (ballots as 64-bit
masks, the kernel's leader order), emitting the entries per vertex as the kernel did and rank-first as it does now -- the
same entries at the same positions.  Host only: built with the address and undefined-behaviour sanitizers and run
directly; no GPU and no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rank_first_emits_the_same_entries(tmp_path):
    exe = str(tmp_path / "csr_scatter_rank")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "csr_scatter_rank_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "csr scatter rank ok" in r.stdout and "DIFFERENT" not in r.stdout
    assert r.stdout.count("vertices  ok\n") == 3 * 6 * 8   # dimensions x sizes x kinds of rows
