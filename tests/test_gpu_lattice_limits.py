"""The permutohedral lattice and the DenseCRF frame path at every capacity limit of the lattice code, against the CPU
oracle bit for bit.  Each case lands on a named side of a limit -- the vertex counts come from the oracle, in the bands of
synthetic.LATTICE_BANDS that the CPU suite pins (test_oracle_crf.py) -- and asserts the path it reached through
rvseg_last_schedule, with the expected path derived from those counts and the limits:

  MF_LDS_BYTES = 24 KB   mf_update_kernel: a frame's vertex values in LDS (Mf <= 512 for 9 classes, <= 768 for 8) or
                         sliced from L2
  LP_SET = 512           lattice_points_kernel: block-local key set, carried over 2 / 4 / 8 chunks of 256 points
  RES_MAX_OWNV = 640     resident_plan_kernel: vertices per resident block; past B x 640 the planner gives up and the
                         list-major walk does the splat
  CS_MCAP = 4096         counting-sort CSR (2^13 slots per frame at most); past it 2^16 slots and the radix-sort CSR
  capacity ladder        2^12 -> 2^13 -> 2^16 -> ... -> the per-frame worst case, chunk retries of the host entry
  1022 frames            per chunk (10-bit frame field of the launch-order sort key)
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from rovinasemanticsegmentation_amd import synthetic
from test_gpu_crf import LP_SET, distinct_vertices_per_block, lattice_points_chunks
from test_oracle_crf import band_params

pytestmark = pytest.mark.gpu

RES_MAX_OWNV = 640
RES_MAX_VERTS = 4096
CS_MCAP = 4096
FRAME_D = 6
_POOL = max(1, min(os.cpu_count() or 1, 16))
_oracle_cache = {}


def _forest():
    return synthetic.make_forest_bytes(seed=24, n_trees=3, leaves_per_tree=256, max_depth=12, single_classes=9, layer_classes=(8, 9))


def _frames(spec, W, H):
    """spec: (scene, index) per frame; ("none", index) is the flat frame's colour with no valid depth."""
    rgb = np.empty((len(spec), H, W, 3), np.uint8)
    depth = np.empty((len(spec), H, W), np.uint16)
    for k, (scene, i) in enumerate(spec):
        rgb[k], depth[k] = synthetic.make_frame(i, W, H, holes=True, scene="flat" if scene == "none" else scene)
        if scene == "none":
            depth[k] = 0
    return rgb, depth


def _oracle_frames(oracle, blob, kw, multi, spec, unknown):
    """Oracle (posteriors, marginals, labels) and lattice vertices of each frame of spec, cached across the cases."""
    key = (blob, tuple(sorted(kw.items())), multi, tuple(unknown))
    cache = _oracle_cache.setdefault(key, {})
    todo = [s for s in dict.fromkeys(spec) if s not in cache]
    if todo:
        forest = oracle.Forest(blob)
        p = oracle.default_params(**kw)
        calib = synthetic.make_calib(p.width, p.height)
        rgb, depth = _frames(todo, p.width, p.height)

        def one(k):
            post, marg, lab = oracle.segment_frame(p, forest, multi, rgb[k], depth[k], calib, label_mode=1, unknown=unknown)
            m = oracle.Lattice(oracle.frame_crf_features(p, rgb[k], oracle.cloud(p, depth[k], calib))).M
            return post, marg, lab, m

        with ThreadPoolExecutor(_POOL) as ex:
            for s, r in zip(todo, ex.map(one, range(len(todo)))):
                cache[s] = r
    return [cache[s] for s in spec]


def _assert_frames_exact(out, want, posteriors=True):
    for i, (post, marg, lab, _) in enumerate(want):
        if posteriors:
            assert np.array_equal(out["posteriors"][i], post), i
        assert np.array_equal(out["marginals"][i], marg), i
        assert np.array_equal(out["labels"][i].ravel(), lab), i


def _ceil_log2(v):
    b = 0
    while (1 << b) < v:
        b += 1
    return b


def _capacity_after_overflows(max_vertices, N, base=12):
    """rvseg_lattice.hip: lattice_raise_capacity raises the per-frame capacity (x8 per overflow, stopping at 2^13 on the way up,
    never past the worst case 2 N (d+1)) until a frame's region holds its vertices at load factor 1/2."""
    safe = _ceil_log2(2 * ((N + 3) // 4 * 4) * (FRAME_D + 1))
    cur = min(base, safe)
    while max_vertices > (1 << cur) // 2 and cur < safe:
        cur = min(cur + (min(3, 13 - cur) if cur < 13 else 3), safe)
    return cur


def _resident_pays(n_frames, N, vertices_per_frame_seen):
    """rvseg_lattice.hip: resident_pays."""
    vpf = vertices_per_frame_seen if vertices_per_frame_seen > 0 else 360
    return n_frames >= 2 and n_frames * N >= 6900000 + 4900 * vpf


def _planner_fallbacks(counts, B):
    """Frames the resident planner gives up on by vertex count: more than B blocks of RES_MAX_OWNV, or more than it plans."""
    return sum(1 for m in counts if m > B * RES_MAX_OWNV or m > RES_MAX_VERTS)


# ---- A. MF_LDS_BYTES: LDS and L2 slices of the mean-field update in one launch ------------------------------------------
@pytest.mark.parametrize("band,C,edge", [("mf_lds_c9", 9, 512), ("mf_lds_c8", 8, 768)])
def test_mf_update_lds_and_l2_slices_in_one_launch(gpu_ctx_factory, oracle, band, C, edge):
    """Two label layers (8 and 9 classes) over one lattice, two frames in one launch: one frame's vertex values fit the
    update kernel's 24 KB of LDS for the C-class layer, the other's are sliced from L2.  Under both schedules."""
    scene, _, W, H, frames = synthetic.lattice_band(band)
    kw = dict(band_params(oracle, band), dcrf_iterations=2)
    blob = _forest()
    spec = [(scene, i) for i in frames]
    want = _oracle_frames(oracle, blob, kw, 1, spec, [7, 8])
    counts = [w[3] for w in want]
    assert min(counts) <= edge < max(counts), counts      # both sides of the edge in one launch
    rgb, depth = _frames(spec, W, H)
    calib = synthetic.make_calib(W, H)
    for splat in (1, 2):
        ctx = gpu_ctx_factory(multi_layer=1, use_dense_crf=1, label_mode=1, unknown_label=[7, 8], max_batch=len(spec),
                              schedule=dict(splat=splat, resident_blocks=4), **kw)
        ctx.forest_load(blob)
        out = ctx.segment_frames(rgb, depth, calib)
        info = ctx.last_schedule()
        assert info["splat"] == ("resident" if splat == 2 else "list-major"), info
        assert info["planner_fallback"] == 0 and info["csr_path"] == 1 and info["vertices"] == sum(counts), info
        _assert_frames_exact(out, want)


# ---- B. RES_MAX_OWNV: the resident planner's limit ---------------------------------------------------------------------
@pytest.mark.parametrize("band", ["deep", "deep_planner"])
def test_resident_planner_limit_by_vertex_count(gpu_ctx_factory, oracle, band):
    """The resident schedule forced with B = 4 blocks per frame: the deep scene (<= 2 560 vertices) fits, at s = 1.1
    (2 561 - 4 096) every frame is past 4 x RES_MAX_OWNV, the planner flags it and the list-major launch does the splat."""
    scene, _, W, H, frames = synthetic.lattice_band(band)
    kw = dict(band_params(oracle, band), dcrf_iterations=2)
    blob = _forest()
    spec = [(scene, i) for i in frames[:3]]
    want = _oracle_frames(oracle, blob, kw, 0, spec, [8])
    counts = [w[3] for w in want]
    B = 4
    expect = _planner_fallbacks(counts, B)
    assert expect == (len(spec) if band == "deep_planner" else 0), counts
    rgb, depth = _frames(spec, W, H)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=len(spec), lattice_capacity_log2=13,
                          schedule=dict(splat=2, resident_blocks=B), **kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, synthetic.make_calib(W, H))
    info = ctx.last_schedule()
    assert info["splat"] == "resident" and info["resident_blocks"] == B and info["csr_path"] == 1, info
    assert info["planner_fallback"] == expect and info["vertices"] == sum(counts), (info, counts)
    _assert_frames_exact(out, want)


# ---- C. CS_MCAP: just below the counting-sort ceiling -------------------------------------------------------------------
def test_counting_sort_ceiling_both_schedules(gpu_ctx_factory, oracle):
    """Frames just below 4 096 vertices with 2^13 slots per frame: the counting-sort CSR at its largest capacity, under
    the list-major walk and under the resident schedule with enough blocks (B = 8: 5 120 >= Mf) to hold every frame."""
    band = "deep_cs_ceiling"
    scene, _, W, H, frames = synthetic.lattice_band(band)
    kw = dict(band_params(oracle, band), dcrf_iterations=2)
    blob = _forest()
    spec = [(scene, i) for i in frames]
    want = _oracle_frames(oracle, blob, kw, 0, spec, [8])
    counts = [w[3] for w in want]
    assert 2048 < max(counts) <= CS_MCAP, counts
    rgb, depth = _frames(spec, W, H)
    for splat, B in ((1, 0), (2, 8)):
        assert B == 0 or _planner_fallbacks(counts, B) == 0
        ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=len(spec), lattice_capacity_log2=13,
                              schedule=dict(splat=splat, resident_blocks=B), **kw)
        ctx.forest_load(blob)
        out = ctx.segment_frames(rgb, depth, synthetic.make_calib(W, H))
        info = ctx.last_schedule()
        assert info["csr_path"] == 1 and info["capacity_log2"] == 13 and info["vertices"] == sum(counts), info
        assert info["splat"] == ("resident" if splat == 2 else "list-major") and info["planner_fallback"] == 0, info
        _assert_frames_exact(out, want)


# ---- D. past CS_MCAP: the radix-sort CSR in the frame pipeline ----------------------------------------------------------
def test_radix_csr_in_the_frame_pipeline(gpu_ctx_factory, oracle):
    """Deep frames with more than 4 096 vertices, flat frames and a frame without any valid depth in one chunk, default
    capacity: the build overflows 2^12, then 2^13, and the chunk runs with 2^16 slots per frame on the radix-sort CSR."""
    band = "deep_radix"
    scene, _, W, H, frames = synthetic.lattice_band(band)
    kw = dict(band_params(oracle, band), dcrf_iterations=2)
    blob = _forest()
    spec = [(scene, frames[0]), ("flat", 0), (scene, frames[1]), ("none", 3)]
    want = _oracle_frames(oracle, blob, kw, 0, spec, [8])
    counts = [w[3] for w in want]
    assert min(counts[0], counts[2]) > CS_MCAP, counts
    cap = _capacity_after_overflows(max(counts), W * H)
    assert cap == 16
    rgb, depth = _frames(spec, W, H)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=len(spec), **kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, synthetic.make_calib(W, H))
    info = ctx.last_schedule()
    assert info["capacity_log2"] == cap and info["csr_path"] == 2 and info["splat"] == "list-major", info
    assert info["vertices"] == sum(counts) and info["planner_fallback"] == 0, info
    _assert_frames_exact(out, want)


# ---- E. the worst-case capacity -----------------------------------------------------------------------------------------
def test_worst_case_lattice(gpu_ctx_factory, oracle):
    """Random colour and depth with both kernels x16: (nearly) every entry is a vertex of its own, no vertex list is
    longer than 3 entries and most blur neighbours are missing.  The capacity climbs 2^12 -> 2^13 -> 2^16 -> 2^19, the worst case
    2 N (d+1) of a 160 x 120 frame, without an error."""
    band = "worst_case"
    scene, _, W, H, frames = synthetic.lattice_band(band)
    kw = dict(band_params(oracle, band), dcrf_iterations=2)
    blob = _forest()
    spec = [(scene, i) for i in frames]
    want = _oracle_frames(oracle, blob, kw, 0, spec, [8])
    counts = [w[3] for w in want]
    cap = _capacity_after_overflows(max(counts), W * H)
    assert cap == _ceil_log2(2 * W * H * (FRAME_D + 1)) == 19
    rgb, depth = _frames(spec, W, H)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=len(spec), **kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, synthetic.make_calib(W, H))
    info = ctx.last_schedule()
    assert info["capacity_log2"] == cap and info["csr_path"] == 2 and info["vertices"] == sum(counts), info
    longest = 0
    p = oracle.default_params(**kw)
    for k in range(len(spec)):
        lat = oracle.Lattice(oracle.frame_crf_features(p, rgb[k], oracle.cloud(p, depth[k], synthetic.make_calib(W, H))))
        longest = max(longest, int(np.bincount(lat.offset.ravel()).max()))
    assert longest <= 3 and info["longest_list"] == longest, (info, longest)
    _assert_frames_exact(out, want)


# ---- F. an overflow in the middle of a host call ------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["middle", "last"])
@pytest.mark.parametrize("pinned", [False, True])
def test_overflow_in_one_chunk_of_a_host_call(gpu_ctx_factory, oracle, where, pinned):
    """segment_frames with max_batch = 2 and 5 frames (chunks of 2, 2, 1) on a fresh context: only one chunk holds deep
    frames, which overflow the default 2^12 slots.  Its overflow is seen while the next chunk is being enqueued (the host
    loop then redoes both) or, for the last chunk, by the call's final status check.  Clean chunks before and after it
    must keep their outputs; with pageable outputs (staging ring) and with page-locked ones (out=)."""
    spec = {"middle": [("flat", 0), ("flat", 1), ("deep", 0), ("deep", 1), ("flat", 2)],
            "last": [("flat", 0), ("flat", 1), ("flat", 2), ("flat", 1), ("deep", 0)]}[where]
    W, H = 640, 480
    kw = dict(width=W, height=H, dcrf_iterations=2)
    blob = _forest()
    want = _oracle_frames(oracle, blob, kw, 0, spec, [8])
    counts = [w[3] for w in want]
    chunks = [counts[0:2], counts[2:4], counts[4:5]]
    over = [max(c) > (1 << 12) // 2 for c in chunks]
    assert over == ([False, True, False] if where == "middle" else [False, False, True]), counts
    rgb, depth = _frames(spec, W, H)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=2, **kw)
    ctx.forest_load(blob)
    calib = synthetic.make_calib(W, H)
    if pinned:
        bufs = ctx.host_buffers(len(spec))
        try:
            for k in ("posteriors", "marginals", "labels"):
                bufs[k].fill(0)
            out = ctx.segment_frames(rgb, depth, calib, out=bufs)
            out = {k: out[k].copy() for k in ("posteriors", "marginals", "labels")}
        finally:
            ctx.release_host_buffers(bufs)
    else:
        out = ctx.segment_frames(rgb, depth, calib)
    info = ctx.last_schedule()
    assert info["capacity_log2"] == _capacity_after_overflows(max(counts), W * H) == 13, info
    assert info["n_frames"] == 1 and info["vertices"] == counts[4], info     # the last chunk's build
    _assert_frames_exact(out, want)


# ---- G. the headline chunk on the deep scene ----------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1.0, 1.1])
def test_headline_chunk_on_the_deep_scene(gpu_ctx_factory, oracle, s):
    """64 deep frames of 640 x 480 as ONE chunk (segment_frames_device, max_batch = 64, default schedule), three calls
    on one fresh context.  The first overflows the default 2^12 slots: poll_status reports RVSEG_ERR_CAPACITY and the
    call is repeated.  resident_pays decides from the vertices per frame of the context's previous CLEAN build (none
    before the second call: the flat scene's 360 are assumed), so the schedule may change from the second call to the
    third; at s = 1.1 the second runs resident with the planner giving up on every frame past B x 640 vertices and the
    third goes list-major.  Every clean call bit-exact against the oracle, all 64 frames."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    n, W, H, C = 64, 640, 480, 9
    N = W * H
    p0 = oracle.default_params()
    kw = dict(dcrf_iterations=5, dcrf_xyz_kernel=p0.dcrf_xyz_kernel * s, dcrf_rgb_kernel=p0.dcrf_rgb_kernel * s)
    blob = synthetic.make_forest_bytes(seed=7, n_trees=4, leaves_per_tree=1 << 12, max_depth=20, single_classes=C, layer_classes=(8, 9))
    spec = [("deep", i) for i in range(n)]
    want = _oracle_frames(oracle, blob, kw, 0, spec, [8])
    counts = [w[3] for w in want]
    assert max(counts) > 2048 and max(counts) <= CS_MCAP, (min(counts), max(counts))
    rgb, depth = _frames(spec, W, H)
    calib = synthetic.make_calib(W, H)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=rv.capi.LABEL_CRF, unknown_label=[8], max_batch=n, **kw)
    ctx.forest_load(blob)
    dev = torch.device("cuda", 0)
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    d_marg = torch.zeros((n, C * N), dtype=torch.float32, device=dev)
    d_lab = torch.full((n, N), -99, dtype=torch.int8, device=dev)
    stream = torch.cuda.current_stream(dev)

    def call():
        d_lab.fill_(-99)
        ctx.segment_frames_device(n, d_rgb.data_ptr(), d_depth.data_ptr(), calib, 0, d_marg.data_ptr(), d_lab.data_ptr(), stream.cuda_stream)

    call()
    with pytest.raises(rv.capi.RvsegError) as e:
        ctx.poll_status(wait=True)
    assert e.value.status == rv.capi.ERR_CAPACITY
    seen = 0
    for attempt in range(2):
        call()
        assert ctx.poll_status(wait=True) == rv.capi.OK
        info = ctx.last_schedule()
        resident = _resident_pays(n, N, seen)
        assert info["splat"] == ("resident" if resident else "list-major"), (attempt, seen, info)
        expect = _planner_fallbacks(counts, info["resident_blocks"]) if resident else 0
        assert info["planner_fallback"] == expect, (attempt, info)
        assert info["capacity_log2"] == 13 and info["csr_path"] == 1 and info["vertices"] == sum(counts), info
        torch.cuda.synchronize(dev)
        marg = d_marg.cpu().numpy()
        lab = d_lab.cpu().numpy()
        for i in range(n):
            _, wm, wl, _ = want[i]
            assert np.array_equal(lab[i], wl), (attempt, i)
            assert np.array_equal(marg[i], wm), (attempt, i)
        seen = sum(counts) // n    # crf_frames_status: vertices per frame of the clean build, integer division
    if s == 1.1:   # the case the docstring names: resident with fall-backs, then list-major
        assert _resident_pays(n, N, 0) and not _resident_pays(n, N, seen)


# ---- H. LP_SET: the block-local key set of lattice_points_kernel (and the random clouds of 2^19 .. 2^21 points in
# test_gpu_crf.py: test_lattice_structure_matches_oracle) -----------------------------------------------------------------
def test_lattice_points_key_set_smooth_then_saturated(gpu_ctx_factory, oracle):
    """A cloud of 2^20 points (4 chunks of 256 per block) whose first half is a smooth path through feature space (a few
    vertices per block: the LDS set serves them) and whose second half is random (thousands of distinct vertices per
    block: the set saturates and the keys go to the global table, with the set carried over between chunks).  Structure
    and a filter against the oracle."""
    N, d = 1 << 20, 6
    rng = np.random.default_rng(20)
    t = np.linspace(0.0, 1.0, N // 2, dtype=np.float64)[:, None]
    smooth = (np.array([-1.0, 0.5, 2.0, 0.0, -0.5, 1.5]) + t * np.array([3.0, -2.0, 1.0, 2.5, 2.0, -1.0])).astype(np.float32)
    F = np.concatenate([smooth, (rng.random((N // 2, d)) * 4.0 - 4.0 / 3).astype(np.float32)])
    lat = oracle.Lattice(F)
    n_chunks = lattice_points_chunks(N)
    assert n_chunks == 4
    per_block = distinct_vertices_per_block(lat.offset, n_chunks)
    half = len(per_block) // 2
    assert per_block[:half].max() <= LP_SET and per_block[half:].min() > LP_SET, (per_block[:half].max(), per_block[half:].min())
    ctx = gpu_ctx_factory()
    off, bary, keys, M = ctx.lattice_build(F)
    assert M == lat.M
    assert np.array_equal(bary, lat.barycentric)
    assert np.array_equal(keys[off], lat.keys[lat.offset])
    V = rng.random((N, 3)).astype(np.float32)
    assert np.array_equal(ctx.lattice_filter(V), lat.compute(V))


# ---- I. the generic counting-sort kernel at its largest capacity --------------------------------------------------------
@pytest.mark.parametrize("d,spread", [(3, 12.0), (4, 6.0), (7, 1.9)])
def test_generic_counting_sort_at_its_largest_capacity(gpu_ctx_factory, oracle, d, spread):
    """Clouds with 2 049 - 4 096 vertices and 2^13 slots: the counting-sort CSR at mcap = 4 096 for dimensions whose
    scatter goes entry by entry (csr_scatter_entries_kernel).  Structure, filter and a 3-iteration CRF against the oracle."""
    N = 30000
    rng = np.random.default_rng(d * 31 + N)
    F = (rng.random((N, d)) * spread - spread / 3).astype(np.float32)
    lat = oracle.Lattice(F)
    assert 2048 < lat.M <= CS_MCAP, lat.M
    ctx = gpu_ctx_factory(lattice_capacity_log2=13)
    off, bary, keys, M = ctx.lattice_build(F)
    info = ctx.last_schedule()
    assert info["csr_path"] == 1 and info["capacity_log2"] == 13 and info["vertices"] == lat.M, info
    assert M == lat.M and np.array_equal(bary, lat.barycentric)
    assert np.array_equal(keys[off], lat.keys[lat.offset])
    V = np.random.default_rng(d).random((N, 4)).astype(np.float32)
    assert np.array_equal(ctx.lattice_filter(V), lat.compute(V))
    U = (np.random.default_rng(d + 1).random((N, 5)) * 4).astype(np.float32)
    Q, mp = ctx.crf_infer(U, F, 3.0, 3)
    info = ctx.last_schedule()
    assert info["csr_path"] == 1 and info["capacity_log2"] == 13, info
    want = oracle.crf_inference(U, F, 3.0, 3)
    assert np.array_equal(Q, want)
    assert np.array_equal(mp, oracle.labels(want, 5, 3))


# ---- J. 1022 frames in one chunk ----------------------------------------------------------------------------------------
def test_1022_frames_in_one_chunk(gpu_ctx_factory, oracle):
    """The largest chunk a DenseCRF context takes: 1 022 frames of 32 x 24 through the device entry in one launch, so
    the lattice keys carry frame ids up to 1 021 -- every frame against the oracle."""
    torch = pytest.importorskip("torch")
    import rovinasemanticsegmentation_amd as rv
    n, W, H = 1022, 32, 24
    N = W * H
    kw = dict(width=W, height=H, patch_size=9, patch_size_reduce=3, dcrf_iterations=2)
    D = oracle.feature_length(oracle.default_params(**kw))
    blob = synthetic.make_forest_bytes(seed=5, n_trees=3, leaves_per_tree=64, max_depth=9, D=D, single_classes=9, layer_classes=(8, 9))
    rgb, depth = synthetic.make_batch(n, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=n, **kw)
    ctx.forest_load(blob)
    dev = torch.device("cuda", 0)
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    d_marg = torch.zeros((n, 9 * N), dtype=torch.float32, device=dev)
    d_lab = torch.full((n, N), -99, dtype=torch.int8, device=dev)
    ctx.segment_frames_device(n, d_rgb.data_ptr(), d_depth.data_ptr(), calib, 0, d_marg.data_ptr(), d_lab.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    assert ctx.poll_status(wait=True) == rv.capi.OK
    info = ctx.last_schedule()
    assert info["n_frames"] == n and info["vertices"] > n, info
    torch.cuda.synchronize(dev)
    marg = d_marg.cpu().numpy()
    lab = d_lab.cpu().numpy()
    forest = oracle.Forest(blob)
    p = oracle.default_params(**kw)

    def one(i):
        return oracle.segment_frame(p, forest, 0, rgb[i], depth[i], calib, label_mode=1, unknown=[8])

    with ThreadPoolExecutor(_POOL) as ex:
        want = list(ex.map(one, range(n)))
    for i in list(range(n - 1, -1, -1)):
        _, wm, wl = want[i]
        assert np.array_equal(lab[i], wl), i
        assert np.array_equal(marg[i], wm), i
