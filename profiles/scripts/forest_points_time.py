"""Times the calls that take the loaded forest over a host matrix of points (rvseg_forest_tools.hip, rvseg_prune.hip: all of
them go through for_each_chunk): forest_eval, forest_classify, forest_measure with the agreement counts, forest_refit and
forest_prune_energy (error energy).  One context of 6 features (patch_size_reduce 1), a 16-tree forest (16 lanes per
point) and a 4-tree forest (4 lanes per point) of 1024 leaves a tree and one layer of 8 classes, P = 65536 (one chunk)
and P = 4 x 65536.  Every call is warmed up and then timed --reps times with the host clock (each call ends in a
synchronise); the figure is the median.  One process, one measurement: run it several times for a spread.  Prints one
JSON line: ms per call, keyed "<trees>t/<P>/<call>"."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

try:
    import torch  # noqa: F401  (shares the HIP runtime with librvseg)
except Exception:
    pass
import rovinasemanticsegmentation_amd as rv
from rovinasemanticsegmentation_amd import synthetic

D, C = 6, 8


def median_ms(call, warmup, reps):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(times)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--points", type=int, nargs="+", default=[65536, 4 * 65536])
    args = ap.parse_args()
    X = synthetic.random_points(5, max(args.points), D)
    y = np.random.default_rng(6).integers(0, C, (X.shape[0], 1)).astype(np.int32)
    out = {}
    with rv.Context(width=64, height=48, patch_size=9, patch_size_reduce=1) as ctx:
        assert ctx.feature_length == D
        for T in (16, 4):
            ctx.forest_load(synthetic.make_forest_bytes(seed=T, n_trees=T, leaves_per_tree=1 << 10, max_depth=20, D=D, single_classes=C,
                                                        layer_classes=(C,)))
            state = list(range(T - 1))
            for P in args.points:
                Xp, yp = X[:P], y[:P]
                calls = {"eval": lambda: ctx.forest_eval(Xp),
                         "classify": lambda: ctx.forest_classify(Xp, 0),
                         "measure_agree": lambda: ctx.forest_measure(Xp, None, 0, want=("agree",)),
                         "refit": lambda: ctx.forest_refit(Xp, yp, [C]),
                         "prune_energy": lambda: ctx.forest_prune_energy(Xp, yp, state)}
                for name, call in calls.items():
                    out["%dt/%d/%s" % (T, P, name)] = median_ms(call, args.warmup, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
