"""Time of one single-layer rvseg_forest_train_prior call at the size of bench.py's forest_train extra (about 550 000
examples, 363 byte features and 3 float features, 8 classes, 4 trees, depth 30, min_split 50) with the unweighted or the
class-frequency-weighted objective.  One mode per process, so that two modes are compared in alternating fresh processes:

    python profiles/scripts/train_prior_time.py none
    python profiles/scripts/train_prior_time.py inverse_frequency

Prints one JSON line: the first call's time and the later calls' (a host clock around the call, which ends in a device
synchronise), and a checksum of the model so that runs of one mode can be seen to agree."""
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def training_set(P=550000, seed=5):
    rng = np.random.default_rng(seed)
    X = np.empty((P, 366), np.float32)
    X[:, :363] = rng.integers(0, 256, (P, 363), dtype=np.uint8)
    X[:, 363:] = rng.standard_normal((P, 3), dtype=np.float32) * 3
    y = ((X[:, 0] // 80) + 2 * (X[:, 5] // 120) + (X[:, 364] > 1)) % 8
    y[rng.random(P) < 0.55] = 0                      # class 0 about nine times as frequent as each other class
    noise = rng.random(P) < 0.1
    y[noise] = rng.integers(0, 8, int(noise.sum()))
    return X, y.astype(np.int32)


def main():
    mode = sys.argv[1]
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    try:
        import torch  # noqa: F401  (shares the HIP runtime with librvseg)
    except Exception:
        pass
    import rovinasemanticsegmentation_amd as rv
    X, y = training_set()
    prior = {"none": None, "inverse_frequency": "inverse_frequency"}[mode]
    times = []
    with rv.Context(multi_layer=0) as ctx:
        for _ in range(calls):
            t0 = time.perf_counter()
            model = ctx.forest_train(X, y, [8], class_prior=prior, num_trees=4, max_depth=30, min_split_examples=50, seed=1)
            times.append(round(time.perf_counter() - t0, 4))
    print(json.dumps({"mode": mode, "examples": int(X.shape[0]), "first_s": times[0], "later_s": times[1:], "model_bytes": len(model),
                      "model_crc32": zlib.crc32(model)}))


if __name__ == "__main__":
    main()
