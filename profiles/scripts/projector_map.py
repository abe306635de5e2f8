"""Timing of the projector on the headline local map (run on the GPU box): 32 sub-images of
640x480, a cloud of ~1.1 M points (frames 0, 8, 16, 24 of the synthetic sequence back-projected at full resolution, as
bench.py's local map), dual-layer model (8 + 9 classes), 10 CRF iterations.
  1. the projector alone: rvseg_project_cloud_device (clear + project + resolve, one launch group of 32 images);
  2. rvseg_process_map_poses_device end to end;
  3. what 2. replaces on the index-image interface: the host-to-device copy of the same 32 index images from page-locked
     memory followed by rvseg_process_map_device -- measured twice, the difference of the two medians is the spread the
     comparison has to respect.
HIP events on the stream, 3 warm-up calls, median of 20.  The posteriors are random numbers: no stage's run time depends on
their values.  Prints one JSON line per figure; with an argument, also writes them to <dir>/projector_map.json."""
import json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import rovinasemanticsegmentation_amd as rv
from rovinasemanticsegmentation_amd import synthetic

W, H, n = 640, 480, 32
N = W * H
REPS, WARM = 20, 3
dev = torch.device("cuda", 0)
out = []


def timed(step):
    for _ in range(WARM):
        step()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def emit(rec):
    print(json.dumps(rec), flush=True)
    out.append(rec)


rgb, depth = synthetic.make_batch(n, W, H)
calib = synthetic.make_calib(W, H)
shifts = [np.array([0.01 * i, -0.02 * i, 0.005 * i]) for i in range(n)]
xyz, col = [], []
for i in range(0, n, 8):
    pts, valid = synthetic.back_project(depth[i], calib, W, H)
    xyz.append((pts[valid] + shifts[i]).astype(np.float32))
    col.append(rgb[i].reshape(-1, 3)[valid].astype(np.float32) / np.float32(255.0))
xyz, col = np.concatenate(xyz), np.concatenate(col)
P = xyz.shape[0]
K = np.linalg.inv(np.asarray(calib, np.float64)[:9].reshape(3, 3)).astype(np.float32)
Ps = np.stack([rv.projection_matrix(K, calib, np.concatenate([np.eye(3), shifts[i][:, None]], 1).astype(np.float32)) for i in range(n)])

blob = synthetic.make_forest_bytes(seed=7, n_trees=4, leaves_per_tree=1 << 10, max_depth=20, single_classes=9, layer_classes=(8, 9))
ctx = rv.Context(multi_layer=1, use_dense_crf=1, dcrf_iterations=10, unknown_label=[7, 8])
ctx.forest_load(blob)
cc = ctx.forest_info()["class_counts"]
S = sum(cc)
s = torch.cuda.current_stream(dev).cuda_stream
d_xyz, d_col = torch.from_numpy(xyz).to(dev), torch.from_numpy(col).to(dev)
d_post = torch.randn((n, S * N), dtype=torch.float32, device=dev)
d_idx = torch.empty((n, H, W), dtype=torch.int32, device=dev)
d_lab = torch.empty((len(cc), P), dtype=torch.int8, device=dev)
d_lab2 = torch.empty((len(cc), P), dtype=torch.int8, device=dev)

med, best, worst = timed(lambda: ctx.project_cloud_device(Ps, P, d_xyz.data_ptr(), d_idx.data_ptr(), 0, s))
hits = int((d_idx >= 0).sum().item())
emit({"what": "rvseg_project_cloud_device (clear + project + resolve)", "images": n, "points": P, "index_hits": hits,
      "ms_median": round(med, 4), "ms_min": round(best, 4), "ms_max": round(worst, 4)})

med, best, worst = timed(lambda: ctx.process_map_poses_device(Ps, d_post.data_ptr(), P, d_xyz.data_ptr(), d_col.data_ptr(), d_lab.data_ptr(), 0, 0, s))
ctx.poll_status(True)
emit({"what": "rvseg_process_map_poses_device", "ms_median": round(med, 3), "ms_min": round(best, 3), "ms_max": round(worst, 3),
      "stages_ms": {k: round(v, 3) for k, v in ctx.last_timing().items()}})

h_idx = d_idx.cpu().pin_memory()
d_idx2 = torch.empty_like(d_idx)


def copy_and_call():
    d_idx2.copy_(h_idx, non_blocking=True)
    ctx.process_map_device(n, d_idx2.data_ptr(), d_post.data_ptr(), P, d_xyz.data_ptr(), d_col.data_ptr(), d_lab2.data_ptr(), 0, s)


runs = [timed(copy_and_call) for _ in range(2)]
ctx.poll_status(True)
emit({"what": "pinned H2D copy of the index images + rvseg_process_map_device (two runs)", "index_bytes": int(h_idx.numel() * 4),
      "ms_median": [round(r[0], 3) for r in runs], "ms_min": [round(r[1], 3) for r in runs], "ms_max": [round(r[2], 3) for r in runs],
      "spread_ms": round(abs(runs[0][0] - runs[1][0]), 3), "stages_ms": {k: round(v, 3) for k, v in ctx.last_timing().items()}})
med_copy, _, _ = timed(lambda: d_idx2.copy_(h_idx, non_blocking=True))
emit({"what": "pinned H2D copy of the index images alone", "ms_median": round(med_copy, 3)})
torch.cuda.synchronize(dev)
emit({"what": "labels of the poses path == labels of the index-image path", "equal": bool(torch.equal(d_lab, d_lab2))})
ctx.close()

if len(sys.argv) > 1:
    os.makedirs(sys.argv[1], exist_ok=True)
    json.dump(out, open(os.path.join(sys.argv[1], "projector_map.json"), "w"), indent=1)
