"""Timing of the external-semantics path (run on the GPU box):
  1. rectify_depth on 64 x 640x480 (14 B per pixel), beside labels_to_rgb on the same pixel count (4 B per pixel, the
     streaming yardstick of section 10), both as whole calls between HIP events.  Run the script under
     `rocprofv3 --kernel-trace --stats -- python profiles/scripts/external_frames.py kernels` for the kernels alone.
  2. rvseg_segment_external_device, 64 frames, layers (8, 9), 5 iterations, full resolution, against
     rvseg_segment_frames_device on the same frames; the distributions ARE that call's posteriors, so both run the same
     mean field.
HIP events on the stream, 3 warm-up steps, inputs rotating over buffer sets larger than the 256 MB last-level cache,
median of 21.  Prints one JSON line per figure; with a second argument, also writes them to <dir>/external_frames_<what>.json."""
import json, os, statistics, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import rovinasemanticsegmentation_amd as rv
from rovinasemanticsegmentation_amd import synthetic

W, H, n = 640, 480, 64
N = W * H
REPS, WARM = 21, 3
dev = torch.device("cuda", 0)
what = sys.argv[1] if len(sys.argv) > 1 else "all"
out = []


def timed(step, sets):
    """median / min ms of step(k) over REPS runs, k rotating over the buffer sets"""
    for k in range(WARM):
        step(k % sets)
    torch.cuda.synchronize(dev)
    ms = []
    for k in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(k % sets)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def emit(rec):
    print(json.dumps(rec), flush=True)
    out.append(rec)


rgb, depth = synthetic.make_batch(n, W, H, holes=True)
calib = synthetic.make_calib(W, H)
blob = synthetic.make_forest_bytes(seed=7, n_trees=4, leaves_per_tree=1 << 14, max_depth=30, single_classes=9, layer_classes=(8, 9))
s = torch.cuda.current_stream(dev).cuda_stream

if what in ("all", "kernels"):
    SETS = 3
    ctx = rv.Context(max_batch=n)
    ctx.forest_load(blob)
    d_depth = [torch.from_numpy(np.roll(depth, k, 0).view(np.int16).copy()).to(dev) for k in range(SETS)]
    d_xyz = [torch.empty((n, H, W, 3), dtype=torch.float32, device=dev) for _ in range(SETS)]
    med, best = timed(lambda k: ctx.rectify_depth_device(n, d_depth[k].data_ptr(), calib, d_xyz[k].data_ptr(), 0.5, 15.0, s), SETS)
    emit({"what": "rectify_depth_device call", "frames": n, "ms_median": round(med, 4), "ms_min": round(best, 4),
          "bytes": 14 * n * N, "tb_s": round(14 * n * N / med / 1e9, 3)})
    # the yardstick: labels_to_rgb over the same number of pixels (one layer of 64 frames = 19.7 Mpx)
    for l, c in enumerate((8, 9)):
        ctx.color_coding_set(l, [{"name": "c%d" % i, "color": [i, 2 * i, 3 * i], "label": i} for i in range(c)])
    d_lab = [torch.randint(0, 8, (n, H, W), dtype=torch.int8, device=dev) for _ in range(SETS)]
    d_col = [torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev) for _ in range(SETS)]
    med, best = timed(lambda k: ctx.labels_to_rgb_device(n, d_lab[k].data_ptr(), d_col[k].data_ptr(), layer=0, stream=s), SETS)
    emit({"what": "labels_to_rgb_device call (one layer)", "frames": n, "ms_median": round(med, 4), "ms_min": round(best, 4),
          "bytes": 4 * n * N, "tb_s": round(4 * n * N / med / 1e9, 3)})
    ctx.close()

if what in ("all", "frames"):
    SETS = 2
    layers, S = (8, 9), 17
    kw = dict(use_dense_crf=1, dcrf_iterations=5, label_mode=1, unknown_label=[7, 8], max_batch=n)
    ctx = rv.Context(**kw)
    ctx.forest_load(blob)
    ctx.external_layers_set(layers)
    d_rgb = [torch.from_numpy(np.roll(rgb, k, 0).copy()).to(dev) for k in range(SETS)]
    d_depth = [torch.from_numpy(np.roll(depth, k, 0).view(np.int16).copy()).to(dev) for k in range(SETS)]
    d_post = [torch.empty((n, S * N), dtype=torch.float32, device=dev) for _ in range(SETS)]
    d_marg = torch.empty((n, S * N), dtype=torch.float32, device=dev)
    d_lab = torch.empty((n, 2, N), dtype=torch.int8, device=dev)
    d_marg2 = torch.empty((n, S * N), dtype=torch.float32, device=dev)

    def forest_step(k):
        ctx.segment_frames_device(n, d_rgb[k].data_ptr(), d_depth[k].data_ptr(), calib, d_post[k].data_ptr(), d_marg.data_ptr(), d_lab.data_ptr(), s)

    def external_step(k):
        ctx.segment_external_device(n, d_rgb[k].data_ptr(), d_depth[k].data_ptr(), calib, d_post[k].data_ptr(), 1, d_marg2.data_ptr(), d_lab.data_ptr(), s)

    med, best = timed(forest_step, SETS)
    ctx.poll_status(True)
    st = ctx.last_timing()
    emit({"what": "segment_frames_device step (forest path)", "frames": n, "ms_median": round(med, 3), "ms_min": round(best, 3),
          "stages_ms": {k: round(v, 3) for k, v in st.items()}})
    for k in range(SETS):       # the posteriors of both buffer sets are the external distributions
        forest_step(k)
    torch.cuda.synchronize(dev)
    want = d_marg.clone()       # marginals of set SETS - 1
    med, best = timed(external_step, SETS)
    ctx.poll_status(True)
    st = ctx.last_timing()
    emit({"what": "segment_external_device step", "frames": n, "ms_median": round(med, 3), "ms_min": round(best, 3),
          "stages_ms": {k: round(v, 3) for k, v in st.items()}, "splat": ctx.last_schedule()["splat"]})
    external_step(SETS - 1)
    torch.cuda.synchronize(dev)
    emit({"what": "external marginals == forest-path marginals on the same posteriors", "equal": bool(torch.equal(want, d_marg2))})
    ctx.close()

if len(sys.argv) > 2:
    os.makedirs(sys.argv[2], exist_ok=True)
    json.dump(out, open(os.path.join(sys.argv[2], "external_frames_%s.json" % what), "w"), indent=1)
