"""The forest pruner's host rules alone under the host sanitizers: tests/cpp/prune_host_test.cpp (its own main) over
csrc/prune_host.h, built with g++ -fsanitize=address,undefined and run directly.  No GPU, no library, nothing loaded into
Python.  The program prints its trajectories (floats as bits); the same runs of tests/prune_restate.py on the votes it
prints must equal them line for line."""
import os
import struct
import subprocess

import numpy as np

import prune_restate as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def _f(word):
    return F32(struct.unpack("<f", struct.pack("<I", int(word, 16)))[0])


def _bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def test_cpp_prune_host_rules_under_sanitizers_and_against_the_restatement(tmp_path):
    exe = str(tmp_path / "prune_host_test")
    csrc = os.path.join(ROOT, "rovinasemanticsegmentation_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-Wall", "-ffp-contract=off", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "prune_host_test.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "prune host ok" in r.stdout
    lines = r.stdout.splitlines()
    votes = np.asarray([int(w) for w in next(l for l in lines if l.startswith("votes")).split()[1:]], np.uint8).reshape(5, 12)
    labels = np.asarray([int(w) for w in next(l for l in lines if l.startswith("labels")).split()[1:]], np.int32)
    agree = np.stack([(votes == votes[t]).sum(1) for t in range(5)]).astype(np.uint64)
    starts = [i for i, l in enumerate(lines) if l.startswith("run ")]
    assert len(starts) == 3
    for i in starts:
        w = lines[i].split()
        params = dict(energy=int(w[3]), seed=int(w[5]), start_temperature=_f(w[7]), end_temperature=_f(w[9]), alpha=_f(w[11]), inner_loops=int(w[13]),
                      p_exchange=_f(w[15]), p_remove=_f(w[16]), p_add=_f(w[17]))
        initial = [int(x) for x in lines[i + 1].split()[1:]]
        if params["energy"] == pr.COVER:
            run = pr.run(params, 5, initial, lambda s: pr.cover_energy(agree, 12, s))
        else:
            run = pr.run(params, 5, initial, lambda s: pr.error_energy(votes, labels, s))
        want = ["initial " + " ".join(map(str, initial)), ("kinds " + " ".join(map(str, run["step_kind"].tolist()))).rstrip()]
        want += ["trace %d %s %s %s %d" % (it, _bits(t), _bits(e), _bits(b), n) for it, t, e, b, n in run["trace"]]
        want += ["best %s %s" % (_bits(run["best_energy"]), " ".join(map(str, run["state"].tolist())))]
        got = [l.rstrip() for l in lines[i + 1:i + 1 + len(want)]]
        assert got == want, w[1]
        if w[1] != "none":
            assert len(set(run["step_kind"].tolist())) == 3, "the dumped runs take every branch"   # (a condition on the recipe)
