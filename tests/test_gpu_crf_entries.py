"""The point-CRF entry points as callers see them: the five inference entries compute the same bits from the same
input (also when every one of them has to retry its lattice build at the safe capacity), the retry rebuilds every
term, zero terms are a plain softmax, bad arguments are refused with the entry's own status and text, and the stage
names of rvseg_last_timing and the fields of rvseg_last_schedule after each entry are the recorded ones.

Q and labels are compared with the CPU oracle.  The refusal texts, stage names and schedule fields are literals
recorded from the library as it was before the host orchestration of rvseg_crf.hip was unified."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, ITERS, W_POTTS = 600, 5, 3.0


def _inputs(seed, Cn, d, n=N):
    rng = np.random.default_rng(seed)
    U = (rng.random((n, Cn)) * 3).astype(np.float32)
    F = (rng.random((n, d)) * 6).astype(np.float32)
    return U, F


def _safe_log2(n, d):
    npad = (n + 3) // 4 * 4
    b = 0
    while (1 << b) < 2 * npad * (d + 1):
        b += 1
    return b


class _Dev:
    """Device copies of one input and fresh outputs (torch owns the memory)."""

    def __init__(self, torch, U, F):
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.U = torch.from_numpy(U).to(self.dev)
        self.F = torch.from_numpy(F).to(self.dev)
        self.n, self.Cn = U.shape
        self.d = F.shape[1]
        torch.cuda.synchronize(self.dev)

    def out(self):
        Q = self.torch.full((self.n, self.Cn), -7.0, dtype=self.torch.float32, device=self.dev)
        mp = self.torch.full((self.n,), -99, dtype=self.torch.int8, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        return Q, mp

    def get(self, t):
        self.torch.cuda.synchronize(self.dev)
        return t.cpu().numpy()


def _run_entry(rv, ctx, entry, U, F, D, mode, unknown, with_q=True):
    """One of the five entries on (U, F) -> (Q or None, labels)."""
    S = rv.NORMALIZE_SYMMETRIC
    Cn, d = U.shape[1], F.shape[1]
    if entry == "infer":
        return ctx.crf_infer(U, F, W_POTTS, ITERS, mode, unknown)
    if entry == "multi":
        return ctx.crf_infer_multi(U, [F], [W_POTTS], ITERS, mode, unknown)
    if entry == "terms":
        return ctx.crf_infer_terms(U, [(F, W_POTTS, rv.CONST_KERNEL, S, None)], ITERS, mode, unknown)
    Q, mp = D.out()
    q_ptr = Q.data_ptr() if with_q else 0
    if entry == "device":
        ctx.crf_infer_device(N, Cn, d, D.U.data_ptr(), True, D.F.data_ptr(), W_POTTS, ITERS, q_ptr, mp.data_ptr(), mode, unknown)
    else:
        assert entry == "terms_device"
        ctx.crf_infer_terms_device(N, Cn, [((D.F.data_ptr(), d), W_POTTS, rv.CONST_KERNEL, S, None)], D.U.data_ptr(), True, ITERS,
                                   q_ptr, mp.data_ptr(), mode, unknown)
    return (D.get(Q) if with_q else None), D.get(mp)


ENTRIES = ["infer", "multi", "device", "terms", "terms_device"]


# ---------------------------------------------------------------------------------------------
# 1. entry equivalence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity_log2", [0, 4])   # 4: 16 slots for 600 points -- every entry overflows and retries
@pytest.mark.parametrize("d", [2, 6])
@pytest.mark.parametrize("Cn", [2, 9, 11])          # the sequential path, a fused class count, an unfused one
def test_entries_agree_with_each_other_and_the_oracle(gpu_ctx_factory, oracle, Cn, d, capacity_log2):
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    U, F = _inputs(100 + 10 * Cn + d, Cn, d)
    want = oracle.crf_inference(U, F, W_POTTS, ITERS)
    ctx = gpu_ctx_factory(lattice_capacity_log2=capacity_log2)
    D = _Dev(torch, U, F)
    unknown = Cn - 1
    for mode in range(4):
        want_lab = oracle.labels(want, Cn, mode, unknown=unknown)
        for entry in ENTRIES:
            Q, mp = _run_entry(rv, ctx, entry, U, F, D, mode, unknown)
            assert np.array_equal(Q.view(np.uint32), want.view(np.uint32)), (entry, mode)
            assert np.array_equal(mp, want_lab), (entry, mode)
            if capacity_log2 == 4:
                assert ctx.last_schedule()["capacity_log2"] == _safe_log2(N, d), entry
        for entry in ("device", "terms_device"):   # labels only
            _, mp = _run_entry(rv, ctx, entry, U, F, D, mode, unknown, with_q=False)
            assert np.array_equal(mp, want_lab), (entry, mode, "labels only")


# ---------------------------------------------------------------------------------------------
# 2. the retry rebuilds every term
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [9, 11])
def test_retry_is_all_or_nothing(gpu_ctx_factory, oracle, Cn):
    import rovinasemanticsegmentation_amd as rv
    U, F6 = _inputs(200 + Cn, Cn, 6)
    _, F2 = _inputs(300 + Cn, Cn, 2)
    want = oracle.crf_inference_multi(U, [F6, F2], [3.0, 10.0], ITERS)
    ctx = gpu_ctx_factory(lattice_capacity_log2=4)
    S = rv.NORMALIZE_SYMMETRIC
    Q, mp = ctx.crf_infer_multi(U, [F6, F2], [3.0, 10.0], ITERS, 1, Cn - 1)
    assert np.array_equal(Q, want) and np.array_equal(mp, oracle.labels(want, Cn, 1, unknown=Cn - 1))
    assert ctx.last_schedule()["capacity_log2"] == _safe_log2(N, 2)   # the last lattice built: d = 2 at the safe capacity
    Q, mp = ctx.crf_infer_terms(U, [(F6, 3.0, rv.CONST_KERNEL, S, None), (F2, 10.0, rv.CONST_KERNEL, S, None)], ITERS, 1, Cn - 1)
    assert np.array_equal(Q, want) and np.array_equal(mp, oracle.labels(want, Cn, 1, unknown=Cn - 1))
    assert ctx.last_schedule()["capacity_log2"] == _safe_log2(N, 2)


# ---------------------------------------------------------------------------------------------
# 3. zero terms
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [2, 9, 11])
def test_zero_terms_is_the_softmax_of_the_unary(gpu_ctx_factory, oracle, Cn):
    U, _ = _inputs(400 + Cn, Cn, 2)
    want = oracle.exp_and_normalize(-U)
    ctx = gpu_ctx_factory()
    for Q, mp in (ctx.crf_infer_multi(U, [], [], 3), ctx.crf_infer_terms(U, [], 3)):
        assert np.array_equal(Q, want)
        assert np.array_equal(mp, oracle.labels(want, Cn, 3))


# ---------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------
BAD, DIM = "bad arguments", "feature dimension must be in [1,7]"
# what to change in a valid call -> the text of rvseg_last_error; the status is RVSEG_ERR_INVALID_ARG throughout
REFUSALS = {
    "infer": {"N=0": BAD, "C=0": BAD, "C=65": BAD, "d=0": DIM, "d=8": DIM, "iterations=-1": BAD, "label_mode=4": BAD,
              "unary=null": BAD},
    "multi": {"N=0": BAD, "C=0": BAD, "C=65": BAD, "d=0": DIM, "d=8": DIM, "iterations=-1": BAD, "label_mode=4": BAD,
              "unary=null": BAD, "n=9": BAD},
    "device": {"N=0": BAD, "C=0": BAD, "C=65": BAD, "d=0": BAD, "d=8": BAD, "iterations=-1": BAD, "label_mode=4": BAD,
               "unary=null": BAD, "outputs=null": BAD},
    "terms": {"N=0": BAD, "C=0": BAD, "C=65": BAD, "d=0": BAD, "d=8": BAD, "iterations=-1": BAD, "label_mode=4": BAD,
              "unary=null": BAD, "n=9": BAD},
    "terms_device": {"N=0": BAD, "C=0": BAD, "C=65": BAD, "d=0": BAD, "d=8": BAD, "iterations=-1": BAD, "label_mode=4": BAD,
                     "unary=null": BAD, "n=9": BAD, "outputs=null": BAD},
}


def _raw_call(rv, ctx, entry, change, U, F, D, Q, mp):
    """The entry's C function on a valid call with one argument changed; returns its status.  Q / mp: the outputs
    (numpy for the host entries, torch for the device ones), which a refused call must leave alone."""
    a = dict(N=N, C=U.shape[1], d=F.shape[1], iterations=ITERS, label_mode=1, n=1, unary=True, outputs=True)
    key, val = change.split("=")
    a[key] = False if val == "null" else int(val)
    L, h, vp = ctx.L, ctx.h, C.c_void_p
    host = entry in ("infer", "multi", "terms")
    unary = (U.ctypes.data if host else D.U.data_ptr()) if a["unary"] else None
    feat = F.ctypes.data if host else D.F.data_ptr()
    q_ptr = (Q.ctypes.data if host else Q.data_ptr()) if a["outputs"] else None
    m_ptr = (mp.ctypes.data if host else mp.data_ptr()) if a["outputs"] else None
    n = a["n"]
    if entry == "infer":
        return L.rvseg_crf_infer(h, a["N"], a["C"], a["d"], vp(unary), vp(feat), C.c_float(W_POTTS), a["iterations"], vp(q_ptr),
                                 vp(m_ptr), a["label_mode"], 0)
    if entry == "multi":
        ds = (C.c_int32 * n)(*([a["d"]] * n))
        ptrs = (C.c_void_p * n)(*([feat] * n))
        ws = (C.c_float * n)(*([W_POTTS] * n))
        return L.rvseg_crf_infer_multi(h, a["N"], a["C"], n, ds, ptrs, ws, vp(unary), a["iterations"], vp(q_ptr), vp(m_ptr),
                                       a["label_mode"], 0)
    if entry == "device":
        return L.rvseg_crf_infer_device(h, a["N"], a["C"], a["d"], vp(unary), 1, vp(feat), C.c_float(W_POTTS), a["iterations"],
                                        vp(q_ptr), vp(m_ptr), a["label_mode"], 0, None)
    w = np.array([W_POTTS], np.float32)
    arr = (rv.capi.RvsegCrfTerm * n)()
    for t in arr:
        t.d, t.features, t.compat_params = a["d"], feat, w.ctypes.data
        t.compat, t.kernel_type, t.normalization = rv.capi.COMPAT_POTTS, rv.CONST_KERNEL, rv.NORMALIZE_SYMMETRIC
    if entry == "terms":
        return L.rvseg_crf_infer_terms(h, a["N"], a["C"], n, arr, vp(unary), a["iterations"], vp(q_ptr), vp(m_ptr), a["label_mode"], 0)
    return L.rvseg_crf_infer_terms_device(h, a["N"], a["C"], n, arr, vp(unary), 1, a["iterations"], vp(q_ptr), vp(m_ptr),
                                          a["label_mode"], 0, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals(gpu_ctx_factory, entry):
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    U, F = _inputs(500, 9, 6)
    D = _Dev(torch, U, F)
    ctx = gpu_ctx_factory()
    host = entry in ("infer", "multi", "terms")
    for change, text in REFUSALS[entry].items():
        if host:
            Q, mp = np.full((N, 9), -7.0, np.float32), np.full(N, -99, np.int8)
        else:
            Q, mp = D.out()
        st = _raw_call(rv, ctx, entry, change, U, F, D, Q, mp)
        assert st == rv.capi.ERR_INVALID_ARG, (entry, change)
        assert ctx.L.rvseg_last_error(ctx.h).decode() == text, (entry, change)
        q, m = (Q, mp) if host else (D.get(Q), D.get(mp))
        assert np.all(q == -7.0) and np.all(m == -99), (entry, change)   # nothing ran
    # and the context goes on
    Q, mp = _run_entry(rv, ctx, entry, U, F, D, 1, 8)
    assert Q.shape == (N, 9) and np.all(np.isfinite(Q))


def test_lattice_entry_refusals(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    _, F = _inputs(501, 9, 6)
    ctx = gpu_ctx_factory()
    V = np.ones((N, 3), np.float32)

    def refused(call, text):
        with pytest.raises(rv.capi.RvsegError) as e:
            call()
        assert e.value.status == rv.capi.ERR_INVALID_ARG
        assert ctx.L.rvseg_last_error(ctx.h).decode() == text

    refused(lambda: ctx.lattice_filter(V), "no lattice built on this context")
    refused(lambda: ctx.lattice_neighbours(10, 6, N), "no lattice built on this context")
    M = C.c_int32()
    for n, d, text in ((0, 6, BAD), (N, 0, DIM), (N, 8, DIM)):
        st = ctx.L.rvseg_lattice_build(ctx.h, F.ctypes.data, n, d, None, None, None, 0, C.byref(M))
        assert st == rv.capi.ERR_INVALID_ARG and ctx.L.rvseg_last_error(ctx.h).decode() == text, (n, d)
    st = ctx.L.rvseg_lattice_build(ctx.h, None, N, 6, None, None, None, 0, C.byref(M))
    assert st == rv.capi.ERR_INVALID_ARG and ctx.L.rvseg_last_error(ctx.h).decode() == BAD
    refused(lambda: ctx.lattice_filter(V), "no lattice built on this context")   # none of those built one
    off, bary, keys, m = ctx.lattice_build(F)
    refused(lambda: ctx.lattice_build(F, keys_capacity=m - 1), "keys_out too small")
    assert ctx.lattice_build(F, keys_capacity=m)[3] == m
    refused(lambda: ctx.lattice_filter(np.ones((N, 65), np.float32)), BAD)
    assert ctx.lattice_filter(V).shape == (N, 3)


# ---------------------------------------------------------------------------------------------
# 5. + 6. stage names and schedule info after each entry
# ---------------------------------------------------------------------------------------------
def _info(ctx):
    return ctx.last_schedule()


def observe_entry(rv, torch, ctx, entry, Cn):
    U, F = _inputs(600 + Cn, Cn, 6)
    D = _Dev(torch, U, F)
    _run_entry(rv, ctx, entry, U, F, D, 1, Cn - 1)
    return list(ctx.last_timing()), _info(ctx)


def observe_frames(rv, ctx_factory):
    """2 frames of 160 x 120, two label layers (8 and 9 classes), 5-iteration CRF, through rvseg_segment_frames."""
    from rovinasemanticsegmentation_amd import synthetic
    Wd, Ht = 160, 120
    blob = synthetic.make_forest_bytes(seed=1, n_trees=4, leaves_per_tree=256, max_depth=12)
    rgb, depth = synthetic.make_batch(2, Wd, Ht, holes=True)
    ctx = ctx_factory(width=Wd, height=Ht, use_dense_crf=1, dcrf_iterations=5, label_mode=1, multi_layer=1)
    ctx.forest_load(blob)
    assert len(ctx.forest_info()["class_counts"]) == 2
    ctx.segment_frames(rgb, depth, synthetic.make_calib(Wd, Ht))
    assert ctx.poll_status(wait=True) == rv.capi.OK
    return list(ctx.last_timing()), _info(ctx)


def observe_cloud(rv, torch, ctx_factory):
    """A 500-point cloud fused from 2 index images, two label layers, 3-iteration CRF, through rvseg_process_map_device."""
    from rovinasemanticsegmentation_amd import synthetic
    dev = torch.device("cuda", 0)
    Wd, Ht, n, P = 160, 120, 2, 500
    blob = synthetic.make_forest_bytes(seed=5, n_trees=2, leaves_per_tree=64, max_depth=10)
    ctx = ctx_factory(width=Wd, height=Ht, multi_layer=1, use_dense_crf=1, dcrf_iterations=3, unknown_label=[7, 8])
    ctx.forest_load(blob)
    S = sum(ctx.forest_info()["class_counts"])
    rng = np.random.default_rng(2)
    idx = rng.integers(-1, P, (n, Ht, Wd)).astype(np.int32)
    post = rng.standard_normal((n, S * Wd * Ht)).astype(np.float32)
    xyz = (rng.random((P, 3)) * 4).astype(np.float32)
    crgb = rng.random((P, 3)).astype(np.float32)
    d_idx, d_post, d_xyz, d_crgb = (torch.from_numpy(a).to(dev) for a in (idx, post, xyz, crgb))
    d_lab = torch.full((2, P), -99, dtype=torch.int8, device=dev)
    torch.cuda.synchronize(dev)
    ctx.process_map_device(n, d_idx.data_ptr(), d_post.data_ptr(), P, d_xyz.data_ptr(), d_crgb.data_ptr(), d_lab.data_ptr(), 0)
    assert ctx.poll_status(wait=True) == rv.capi.OK
    torch.cuda.synchronize(dev)
    assert bool((d_lab != -99).all())
    return list(ctx.last_timing()), _info(ctx)


def _schedule(**kw):
    info = dict(splat="list-major", planner_fallback=0, csr_path=2, n_frames=1, points_per_frame=N, vertices=-1, longest_list=3,
                resident_blocks=0, resident_band=0, resident_chunk=0, capacity_log2=14)
    info.update(kw)
    return info


# Recorded.  C = 9 has a fused update (which also writes the labels), C = 11 runs the general loop; the host entries
# reset the stage timer after the build and label after "end", the device entries time the build and the labels.
# 600 points with d = 6 make ~4 040 vertices, more than 2^12 slots hold: these calls retried at the safe 2^14.
_FUSED, _GENERAL = ["softmax", "splat", "blur", "mf_update"], ["softmax", "splat", "blur", "slice"]
STAGES = {"frames": ["prep", "window_map", "normal_feature", "rf_frames", "upsample_pack", "softmax", "splat", "blur", "mf_update",
                     "lattice_build"],
          "cloud": ["fusion", "cloud_features", "lattice_build", "softmax", "splat", "blur", "mf_update"]}
SCHEDULE = {"frames": _schedule(csr_path=1, n_frames=2, points_per_frame=19200, vertices=379, longest_list=6795, capacity_log2=12),
            "cloud": _schedule(csr_path=1, points_per_frame=500, vertices=1596, longest_list=12, capacity_log2=12)}
for _entry in ENTRIES:
    _host = _entry in ("infer", "multi", "terms")
    STAGES[(_entry, 9)] = _FUSED if _host else ["lattice_build"] + _FUSED
    STAGES[(_entry, 11)] = _GENERAL if _host else ["lattice_build"] + _GENERAL + ["labels"]
    SCHEDULE[(_entry, 9)] = _schedule(vertices=4039)
    SCHEDULE[(_entry, 11)] = _schedule(vertices=4045)


@pytest.mark.parametrize("Cn", [9, 11])
@pytest.mark.parametrize("entry", ENTRIES)
def test_stage_names_and_schedule_after_an_entry(gpu_ctx_factory, entry, Cn):
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    names, info = observe_entry(rv, torch, gpu_ctx_factory(), entry, Cn)
    assert names == STAGES[(entry, Cn)]
    assert info == SCHEDULE[(entry, Cn)]


def test_stage_names_and_schedule_after_frames(gpu_ctx_factory):
    import rovinasemanticsegmentation_amd as rv
    names, info = observe_frames(rv, gpu_ctx_factory)
    assert names == STAGES["frames"]
    assert info == SCHEDULE["frames"]


def test_stage_names_and_schedule_after_a_cloud(gpu_ctx_factory):
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    names, info = observe_cloud(rv, torch, gpu_ctx_factory)
    assert names == STAGES["cloud"]
    assert info == SCHEDULE["cloud"]
