"""GPU parity of the permutohedral lattice and the DenseCRF mean-field through the C ABI against
the CPU oracle.  Bar: lattice structure and barycentric weights bit-exact (up to vertex
renumbering, which no result depends on); filter outputs and marginals bit-exact, which implies
the 1e-4 marginal tolerance of the north star; MAP labels identical."""
import os

import numpy as np
import pytest

from rovinasemanticsegmentation_amd import synthetic

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north-star tolerance on CRF marginals (we assert bit-exactness, which is stronger)


def _features(seed, N, d, spread=4.0):
    rng = np.random.default_rng(seed)
    return (rng.random((N, d)) * spread - spread / 3).astype(np.float32)


LP_SET, LP_CHUNKS = 512, 8   # kernels_lattice.hip: lattice_points_kernel's block-local key set, 256-point chunks per block


def lattice_points_chunks(N):
    """kernels_lattice.hip: launch_lattice_points -- 256-point chunks per block, as many (up to 8) as leave >= 1024 blocks."""
    n_chunks = LP_CHUNKS
    while n_chunks > 1 and (N + 255) // 256 // n_chunks < 1024:
        n_chunks >>= 1
    return n_chunks


def distinct_vertices_per_block(offset, n_chunks):
    """Distinct lattice vertices each block of lattice_points_kernel meets (oracle offsets, full blocks)."""
    per = 256 * n_chunks
    nb = offset.shape[0] // per
    rows = np.sort(offset[:nb * per].reshape(nb, -1), axis=1)
    return 1 + (np.diff(rows, axis=1) != 0).sum(1)


@pytest.mark.parametrize("d,N", [(2, 4000), (5, 4000), (6, 4000), (6, 4003), (3, 10), (1, 64), (7, 512),
                                 (6, 1 << 19), (6, 1 << 20), (6, 1 << 21)])
def test_lattice_structure_matches_oracle(gpu_ctx_factory, oracle, d, N):
    """Clouds of 2^19 .. 2^21 points give lattice_points_kernel 2, 4 and 8 chunks per block, and (random features of
    spread 4) thousands of distinct vertices per block: its LDS key set saturates and is carried over between chunks."""
    F = _features(d * 100 + N, N, d)
    lat = oracle.Lattice(F)
    if N >= 1 << 19:
        n_chunks = lattice_points_chunks(N)
        assert n_chunks == {1 << 19: 2, 1 << 20: 4, 1 << 21: 8}[N]
        assert distinct_vertices_per_block(lat.offset, n_chunks).min() > LP_SET
    ctx = gpu_ctx_factory()
    off, bary, keys, M = ctx.lattice_build(F)
    assert M == lat.M
    assert np.array_equal(bary, lat.barycentric)
    got_keys = keys[off]            # N x (d+1) x d
    want_keys = lat.keys[lat.offset]
    assert np.array_equal(got_keys, want_keys)
    assert sorted(map(tuple, keys.tolist())) == sorted(map(tuple, lat.keys.tolist()))


@pytest.mark.parametrize("C", [1, 2, 3, 9])
def test_lattice_filter_bit_exact(gpu_ctx_factory, oracle, C):
    N, d = 6000, 5
    F = _features(7, N, d, spread=3.0)
    V = np.random.default_rng(C).random((N, C)).astype(np.float32)
    want = oracle.Lattice(F).compute(V)
    ctx = gpu_ctx_factory()
    ctx.lattice_build(F)
    got = ctx.lattice_filter(V)
    assert np.abs(got - want).max() <= TOL
    assert np.array_equal(got, want)


def test_lattice_filter_skewed_vertices(gpu_ctx_factory, oracle):
    # nearly all points fall into one simplex: one very long ordered chain per class
    rng = np.random.default_rng(0)
    N, d, C = 40000, 6, 9
    F = (rng.random((N, d)) * 0.05).astype(np.float32)
    V = rng.random((N, C)).astype(np.float32)
    lat = oracle.Lattice(F)
    assert lat.M < 100
    ctx = gpu_ctx_factory()
    ctx.lattice_build(F)
    assert np.array_equal(ctx.lattice_filter(V), lat.compute(V))


def _chain_features(kind, N, d, rng):
    if kind == "skewed":        # nearly all points in one simplex, random weights: binade crossings and ties at random
        return (rng.random((N, d)) * 0.05).astype(np.float32)
    if kind == "constant":      # one weight vector repeated N times: whether an addition ties is the same all along a binade
        return np.tile((rng.random((1, d)) * 0.7).astype(np.float32), (N, 1))
    if kind == "origin":        # points ON a lattice vertex: weights exactly 1 and 0
        return np.zeros((N, d), np.float32)
    F = (rng.random((N, d)) * 0.05).astype(np.float32)      # "mixed": runs of equal weights between random ones
    F[::3] = F[0]
    F[N // 2:N // 2 + N // 8] = 0.0
    return F


@pytest.mark.parametrize("kind", ["skewed", "constant", "origin", "mixed"])
def test_normaliser_ordered_sums_by_wave_scans_equal_the_serial_chain(gpu_ctx_factory, oracle, kind):
    """The normaliser's splat adds a vertex's barycentric weights in list order in fp32.  The default kernel does that
    with exact wave scans inside a binade and falls back to one addition per entry where a tile crosses a binade, holds
    a round-to-even tie or a negative weight (kernels_splat.hip: ordered_tile_sum); rvseg_schedule.serial_chains = 1 is
    the plain dependent chain.  Both must give the oracle's marginals bit for bit on lists of 10^5 entries -- a single
    wrong rounding of a normaliser shows in every marginal of its simplex."""
    rng = np.random.default_rng(len(kind))
    N, d, C = 150000, 6, 3
    F = _chain_features(kind, N, d, rng)
    U = (rng.random((N, C)) * 3).astype(np.float32)
    lat = oracle.Lattice(F)
    assert lat.M < 200
    want = oracle.crf_inference(U, F, 10.0, 2)
    for serial in (0, 1):
        ctx = gpu_ctx_factory(schedule=dict(serial_chains=serial))
        Q, _ = ctx.crf_infer(U, F, 10.0, 2)
        assert np.array_equal(Q, want), (kind, serial, float(np.abs(Q - want).max()))


@pytest.mark.parametrize("C", [9, 8])
@pytest.mark.parametrize("kind", ["skewed", "mixed"])
def test_long_lists_summed_by_scan_blocks_equal_the_serial_adder(gpu_ctx_factory, oracle, C, kind):
    """Launches of a few frames (here: one cloud) give every list of 16 384 entries and more a scan block: one wave per
    class adds the tile's products with ordered_tile_sum instead of the serial adder's 128 dependent additions
    (kernels_splat.hip: splat_scan_item).  Lists of 10^5 entries, 8 and 9 classes (the two block shapes), against the
    oracle bit for bit, with rvseg_schedule.serial_chains = 1 (the serial adder everywhere) as the second witness."""
    rng = np.random.default_rng(C * 7 + len(kind))
    N, d = 120000, 6
    F = _chain_features(kind, N, d, rng)
    U = (rng.random((N, C)) * 4).astype(np.float32)
    want = oracle.crf_inference(U, F, 10.0, 3)
    for serial in (0, 1):
        ctx = gpu_ctx_factory(schedule=dict(serial_chains=serial))
        Q, mp = ctx.crf_infer(U, F, 10.0, 3)
        assert np.array_equal(Q, want), (C, kind, serial, float(np.abs(Q - want).max()))
        assert np.array_equal(mp, want.argmax(1).astype(np.int8))


def test_hash_overflow_falls_back_to_safe_capacity(gpu_ctx_factory, oracle):
    # 2^4 slots cannot hold the lattice: the host entry points rebuild with the safe capacity
    F = _features(3, 2000, 3, spread=40.0)
    lat = oracle.Lattice(F)
    ctx = gpu_ctx_factory(lattice_capacity_log2=4)
    off, bary, keys, M = ctx.lattice_build(F)
    assert M == lat.M and np.array_equal(keys[off], lat.keys[lat.offset])


@pytest.mark.parametrize("C,d", [(9, 6), (2, 3), (21, 5)])
def test_crf_infer_bit_exact(gpu_ctx_factory, oracle, C, d):
    rng = np.random.default_rng(C)
    N = 8000
    F = _features(11, N, d, spread=2.5)
    U = (rng.random((N, C)) * 5).astype(np.float32)
    want = oracle.crf_inference(U, F, 10.0, 5)
    ctx = gpu_ctx_factory()
    Q, mp = ctx.crf_infer(U, F, 10.0, 5)
    assert np.abs(Q - want).max() <= TOL
    assert np.array_equal(Q, want)
    assert np.array_equal(mp, oracle.labels(want, C, 3))
    # zero iterations and zero weight reduce to the softmax of -U
    Q0, _ = ctx.crf_infer(U, F, 10.0, 0)
    assert np.array_equal(Q0, oracle.exp_and_normalize(-U))


def test_crf_label_rule_with_unknown(gpu_ctx_factory, oracle):
    rng = np.random.default_rng(5)
    N, C = 4000, 9
    F = _features(2, N, 6)
    U = (rng.random((N, C)) * 0.7).astype(np.float32)  # flat marginals: many below 2/C
    ctx = gpu_ctx_factory()
    Q, mp = ctx.crf_infer(U, F, 1.0, 2, label_mode=1, unknown_label=8)
    want = oracle.labels(oracle.crf_inference(U, F, 1.0, 2), C, 1, unknown=8)
    assert np.array_equal(mp, want)
    assert (mp == 8).any()


def test_dense_inference_example_on_reference_ppm(gpu_ctx_factory, oracle, golden_dir):
    import rovinasemanticsegmentation_amd as rv
    from test_oracle_crf import dense_inference_inputs
    im, lbl, U, W, H = dense_inference_inputs(golden_dir)
    ctx = gpu_ctx_factory()
    crf = rv.DenseCRF(ctx, W * H, 21)
    crf.setUnaryEnergy(U)
    crf.addPairwiseGaussian(W, H, 3, 3, 3.0)                       # dense_inference.cpp:94
    crf.addPairwiseBilateral(W, H, 80, 80, 13, 13, 13, im, 10.0)   # dense_inference.cpp:101
    Q, mp = crf.inference(5)
    want = oracle.crf_inference_multi(U, [k[0] for k in crf.kernels], [3.0, 10.0], 5)
    assert np.abs(Q - want).max() <= TOL
    assert np.array_equal(Q, want)
    z = np.load(os.path.join(golden_dir, "crf_im2_regression.npz"))
    assert np.array_equal(mp, z["map"])


def test_frames_with_crf_bit_exact(gpu_ctx_factory, oracle):
    blob = synthetic.make_forest_bytes(seed=21, n_trees=4, leaves_per_tree=1024, max_depth=20)
    forest = oracle.Forest(blob)
    rgb, depth = synthetic.make_batch(3, holes=True)
    calib = synthetic.make_calib()
    kw = dict(use_dense_crf=1, dcrf_iterations=5, label_mode=1, max_batch=2)
    ctx = gpu_ctx_factory(**kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    p = oracle.default_params(dcrf_iterations=5)
    for i in range(3):
        post, marg, lab = oracle.segment_frame(p, forest, 1, rgb[i], depth[i], calib, label_mode=1, unknown=[7, 8])
        assert np.array_equal(out["posteriors"][i], post)
        assert np.abs(out["marginals"][i] - marg).max() <= TOL
        assert np.array_equal(out["marginals"][i], marg), i
        assert np.array_equal(out["labels"][i].ravel(), lab)
    # marginals are distributions
    m = out["marginals"][0][: 640 * 480 * 8].reshape(-1, 8)
    assert np.allclose(m.sum(1), 1, atol=1e-5)


def test_config5_shape_dual_layer_10_iterations(gpu_ctx_factory, oracle):
    """BASELINE configs[4] at one frame: 1280x960, dual-layer forest, 10 CRF iterations."""
    W, H = 1280, 960
    blob = synthetic.make_forest_bytes(seed=23, n_trees=4, leaves_per_tree=512, max_depth=14)
    forest = oracle.Forest(blob)
    rgb, depth = synthetic.make_batch(1, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    ctx = gpu_ctx_factory(width=W, height=H, use_dense_crf=1, dcrf_iterations=10, label_mode=1, max_batch=1)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    p = oracle.default_params(width=W, height=H, dcrf_iterations=10)
    post, marg, lab = oracle.segment_frame(p, forest, 1, rgb[0], depth[0], calib, label_mode=1, unknown=[7, 8])
    assert np.array_equal(out["posteriors"][0], post)
    assert np.abs(out["marginals"][0] - marg).max() <= TOL
    assert np.array_equal(out["marginals"][0], marg)
    assert np.array_equal(out["labels"][0].ravel(), lab)


@pytest.mark.parametrize("C,d", [(11, 6), (17, 4), (1, 2)])
def test_crf_infer_class_counts_without_a_fused_update(gpu_ctx_factory, oracle, C, d):
    """C = 11: no fused slice+softmax instantiation (per-entry normaliser, separate kernels);
    C = 17: two splat passes (16 + 1 classes, the second with a partial row); C = 1: degenerate."""
    rng = np.random.default_rng(100 + C)
    N = 6000
    F = _features(7, N, d, spread=3.0)
    U = (rng.random((N, C)) * 4).astype(np.float32)
    want = oracle.crf_inference(U, F, 3.0, 3)
    ctx = gpu_ctx_factory()
    Q, mp = ctx.crf_infer(U, F, 3.0, 3)
    assert np.abs(Q - want).max() <= TOL
    assert np.array_equal(Q, want)
    assert np.array_equal(mp, oracle.labels(want, C, 3))


def test_two_layers_without_fused_update_share_the_normaliser_table(gpu_ctx_factory, oracle):
    """label layers with class counts that have no fused update (11 and 13) run side by side on two streams
    and both read the lattice's per-entry normaliser table; it is filled on the parent stream before the fork."""
    W, H = 160, 120
    blob = synthetic.make_forest_bytes(seed=33, n_trees=3, leaves_per_tree=128, max_depth=10, single_classes=11, layer_classes=(11, 13))
    forest = oracle.Forest(blob)
    rgb, depth = synthetic.make_batch(3, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    kw = dict(width=W, height=H, use_dense_crf=1, dcrf_iterations=2, label_mode=1, max_batch=4, unknown_label=[10, 12])
    ctx = gpu_ctx_factory(**kw)
    ctx.forest_load(blob)
    for _ in range(2):   # the second call rebuilds the lattice: the table must be refilled, not reused
        out = ctx.segment_frames(rgb, depth, calib)
        p = oracle.default_params(width=W, height=H, dcrf_iterations=2)
        for i in range(3):
            post, marg, lab = oracle.segment_frame(p, forest, 1, rgb[i], depth[i], calib, label_mode=1, unknown=[10, 12])
            assert np.array_equal(out["marginals"][i], marg), i
            assert np.array_equal(out["labels"][i].ravel(), lab), i


def test_ten_small_frames_uneven_xcd_groups(gpu_ctx_factory, oracle):
    """10 frames in one chunk: 8 launch groups with 2, 2, 1, ... frames each, 6 trees (not a multiple of
    the 4 tree lanes per point), dual layer, fused labels."""
    W, H = 160, 120
    blob = synthetic.make_forest_bytes(seed=31, n_trees=6, leaves_per_tree=256, max_depth=14)
    forest = oracle.Forest(blob)
    rgb, depth = synthetic.make_batch(10, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    kw = dict(width=W, height=H, use_dense_crf=1, dcrf_iterations=2, label_mode=1, max_batch=16, unknown_label=[7, 8])
    ctx = gpu_ctx_factory(**kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    p = oracle.default_params(width=W, height=H, dcrf_iterations=2)
    for i in range(10):
        post, marg, lab = oracle.segment_frame(p, forest, 1, rgb[i], depth[i], calib, label_mode=1, unknown=[7, 8])
        assert np.array_equal(out["posteriors"][i], post), i
        assert np.array_equal(out["marginals"][i], marg), i
        assert np.array_equal(out["labels"][i].ravel(), lab), i


@pytest.mark.parametrize("B,band,chunk,window", [(2, 1, 64, 1), (8, 8, 128, 1), (16, 4, 64, 0), (5, 32, 128, -1), (3, 2, 128, 2), (4, 16, 64, -1)])
def test_resident_band_splat_is_bit_exact(gpu_ctx_factory, oracle, B, band, chunk, window):
    """The resident band schedule of the mean-field splat (default for chunks of more than 16
    frames, forced here for 8 + 1): a frame's vertices dealt to B blocks, each walking its vertices band by band
    through a precomputed tile list (64-entry chunks packed seven to a tile by the wrap-around rule), the running sums
    parked in LDS and swapped when a slot changes its vertex.  Every chain is still summed in ascending point order
    inside one block, so nothing may change -- for any number of blocks, band size, tile height (64 / 128 entries per
    slot) and pacing window (-1 = no pacing)."""
    blob = synthetic.make_forest_bytes(seed=24, n_trees=3, leaves_per_tree=256, max_depth=12, single_classes=9, layer_classes=(8, 9))
    forest = oracle.Forest(blob)
    W, H = 320, 240
    rgb, depth = synthetic.make_batch(9, W, H, holes=True, start=2)
    calib = synthetic.make_calib(W, H)
    sched = dict(splat=2, resident_blocks=B, resident_band=band, resident_chunk=chunk, resident_window=window)
    ctx = gpu_ctx_factory(width=W, height=H, multi_layer=0, use_dense_crf=1, dcrf_iterations=3, label_mode=1, unknown_label=[8], max_batch=16,
                          schedule=sched)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    info = ctx.last_schedule()
    assert info["splat"] == "resident" and info["planner_fallback"] == 0 and info["resident_blocks"] == B, info
    p = oracle.default_params(width=W, height=H, dcrf_iterations=3)
    for i in range(9):
        post, marg, lab = oracle.segment_frame(p, forest, 0, rgb[i], depth[i], calib, label_mode=1, unknown=[8])
        assert np.array_equal(out["marginals"][i], marg), i
        assert np.array_equal(out["labels"][i].ravel(), lab), i


def test_resident_band_splat_falls_back_when_the_planner_gives_up(gpu_ctx_factory, oracle):
    """A tile table too small for the frame: the planner flags the schedule invalid on the device, the resident
    kernel returns at once and the list-major launch queued behind it does the splat."""
    blob = synthetic.make_forest_bytes(seed=24, n_trees=3, leaves_per_tree=256, max_depth=12, single_classes=9, layer_classes=(8, 9))
    forest = oracle.Forest(blob)
    W, H = 320, 240
    rgb, depth = synthetic.make_batch(2, W, H, holes=True, start=5)
    calib = synthetic.make_calib(W, H)
    ctx = gpu_ctx_factory(width=W, height=H, multi_layer=0, use_dense_crf=1, dcrf_iterations=2, label_mode=1, unknown_label=[8], max_batch=16,
                          schedule=dict(splat=2, resident_band=1, resident_cap_tiles=64))
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    info = ctx.last_schedule()   # the fall-back is reported, not silent
    assert info["splat"] == "resident" and info["planner_fallback"] >= 1, info
    p = oracle.default_params(width=W, height=H, dcrf_iterations=2)
    for i in range(2):
        post, marg, lab = oracle.segment_frame(p, forest, 0, rgb[i], depth[i], calib, label_mode=1, unknown=[8])
        assert np.array_equal(out["marginals"][i], marg), i


@pytest.mark.parametrize("csr_block,splat", [(256, 2), (512, 1), (1024, 2), (2048, 2), (4096, 1), (4096, 2)])
def test_counting_sort_block_sizes(gpu_ctx_factory, oracle, csr_block, splat):
    """rvseg_schedule.csr_block: the counting sort's wave-blocks of 256 .. 4096 points (the library takes 256 for
    launches of <= 8 frames, 1024 otherwise).  The lists -- and the bands the resident schedule cuts them into -- are
    the same for every size, so the marginals are the oracle's to the bit; 6 frames of 320 x 200 = 64 000 points, which
    no block size divides."""
    blob = synthetic.make_forest_bytes(seed=33, n_trees=3, leaves_per_tree=256, max_depth=12, single_classes=9, layer_classes=(8, 9))
    forest = oracle.Forest(blob)
    W, H, n = 320, 200, 6
    rgb, depth = synthetic.make_batch(n, W, H, holes=True, start=2)
    calib = synthetic.make_calib(W, H)
    kw = dict(width=W, height=H, dcrf_iterations=3)
    p = oracle.default_params(**kw)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=n,
                          schedule=dict(splat=splat, csr_block=csr_block), **kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    assert ctx.last_schedule()["splat"] == ("resident" if splat == 2 else "list-major")
    assert ctx.last_schedule()["planner_fallback"] == 0
    for i in range(n):
        post, marg, lab = oracle.segment_frame(p, forest, 0, rgb[i], depth[i], calib, label_mode=1, unknown=[8])
        assert np.array_equal(out["marginals"][i], marg), i
        assert np.array_equal(out["labels"][i].ravel(), lab), i
    with pytest.raises(Exception):
        ctx.set_schedule(csr_block=300)


@pytest.mark.parametrize("scale,B", [(1.0, 4), (3.0, 4), (2.5, 2)])
def test_resident_band_splat_two_layers_and_fine_lattices(gpu_ctx_factory, oracle, scale, B):
    """The resident schedule for the 8-class layer too (two label layers: an 8- and a 9-class mean field over one
    lattice, on two streams), and on lattices with many more vertices per frame than the default kernel widths give
    (both pairwise kernels scaled by 2.5 or 3: a finer lattice; B = 2 makes a block own hundreds of vertices).  At 3.0 a
    frame has up to 1 529 vertices, more than two blocks hold (2 x RES_MAX_OWNV = 1 280), so the B = 2 case runs at 2.5:
    945 - 1 015 vertices, pinned by the band "resident_b2" (test_oracle_crf.py).  planner_fallback = 0 asserts that the
    resident schedule did the splat, not just that it was chosen."""
    blob = synthetic.make_forest_bytes(seed=31, n_trees=3, leaves_per_tree=256, max_depth=12, single_classes=9, layer_classes=(8, 9))
    forest = oracle.Forest(blob)
    W, H = 320, 240
    rgb, depth = synthetic.make_batch(8, W, H, holes=True, start=11)
    calib = synthetic.make_calib(W, H)
    kw = dict(width=W, height=H, dcrf_iterations=2)
    p = oracle.default_params(**kw)
    kw["dcrf_xyz_kernel"] = p.dcrf_xyz_kernel * scale
    kw["dcrf_rgb_kernel"] = p.dcrf_rgb_kernel * scale
    p = oracle.default_params(**kw)
    ctx = gpu_ctx_factory(multi_layer=1, use_dense_crf=1, label_mode=1, unknown_label=[7, 8], max_batch=8, lattice_capacity_log2=13,
                          schedule=dict(splat=2, resident_blocks=B), **kw)
    ctx.forest_load(blob)
    out = ctx.segment_frames(rgb, depth, calib)
    info = ctx.last_schedule()
    assert info["splat"] == "resident" and info["resident_blocks"] == B and info["planner_fallback"] == 0, info
    for i in range(8):
        post, marg, lab = oracle.segment_frame(p, forest, 1, rgb[i], depth[i], calib, label_mode=1, unknown=[7, 8])
        assert np.array_equal(out["marginals"][i], marg), i
        assert np.array_equal(out["labels"][i].ravel(), lab), i


@pytest.mark.parametrize("n_frames", [17, 20, 43])
def test_resident_band_splat_default_path_with_uneven_frame_counts(gpu_ctx_factory, oracle, n_frames):
    """The resident schedule with its own choice of B = CUs / frames blocks per frame (12, 12, 5 here) and frame counts
    that leave the XCD groups uneven.  (Forced: by itself the library takes this schedule from 12 M points per chunk,
    where it is faster than the list-major walk -- 64 frames of 640x480 in test_gpu_batch64.py.)"""
    blob = synthetic.make_forest_bytes(seed=24, n_trees=3, leaves_per_tree=256, max_depth=12, single_classes=9, layer_classes=(8, 9))
    forest = oracle.Forest(blob)
    W, H = 160, 120
    rgb, depth = synthetic.make_batch(n_frames, W, H, holes=True, start=3)
    calib = synthetic.make_calib(W, H)
    kw = dict(width=W, height=H, dcrf_iterations=2)
    ctx = gpu_ctx_factory(multi_layer=0, use_dense_crf=1, label_mode=1, unknown_label=[8], max_batch=64, schedule=dict(splat=2), **kw)
    ctx.forest_load(blob)
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    N = W * H
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    d_marg = torch.zeros((n_frames, 9 * N), dtype=torch.float32, device=dev)
    d_lab = torch.full((n_frames, N), -99, dtype=torch.int8, device=dev)
    ctx.segment_frames_device(n_frames, d_rgb.data_ptr(), d_depth.data_ptr(), calib, 0, d_marg.data_ptr(), d_lab.data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    assert ctx.poll_status(wait=True) == 0
    info = ctx.last_schedule()
    assert info["splat"] == "resident" and info["planner_fallback"] == 0 and info["n_frames"] == n_frames, info
    torch.cuda.synchronize(dev)
    marg = d_marg.cpu().numpy(); lab = d_lab.cpu().numpy()
    p = oracle.default_params(**kw)
    for i in range(n_frames):
        _, wm, wl = oracle.segment_frame(p, forest, 0, rgb[i], depth[i], calib, label_mode=1, unknown=[8])
        assert np.array_equal(marg[i], wm), i
        assert np.array_equal(lab[i], wl), i


def test_config5_chunk_resident_schedule_equals_list_major_walk(gpu_ctx_factory, oracle):
    """BASELINE configs[4] as bench.py runs it on one GPU: a chunk of 16 frames of 1280x960 with two label layers and 10
    CRF iterations (19.7 M points: the library takes the resident band schedule by itself, one launch per layer on two
    streams).  The same chunk with schedule.splat = 1 walks the lists the list-major way; both orders of work sum
    every chain in ascending point order, so marginals and labels have to be identical to the bit -- and frame 5 is
    checked against the CPU oracle as well."""
    torch = pytest.importorskip("torch")
    W, H, n = 1280, 960, 16
    N = W * H
    blob = synthetic.make_forest_bytes(seed=23, n_trees=4, leaves_per_tree=512, max_depth=14)
    rgb, depth = synthetic.make_batch(n, W, H, holes=True)
    calib = synthetic.make_calib(W, H)
    dev = torch.device("cuda", 0)
    d_rgb = torch.from_numpy(rgb).to(dev)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    kw = dict(width=W, height=H, multi_layer=1, use_dense_crf=1, dcrf_iterations=10, label_mode=1, unknown_label=[7, 8], max_batch=n)
    results = []
    for splat, name in ((0, "resident"), (1, "list-major")):   # 0: the library's own choice for this shape
        ctx = gpu_ctx_factory(schedule=dict(splat=splat), **kw)
        ctx.forest_load(blob)
        d_marg = torch.zeros((n, 17 * N), dtype=torch.float32, device=dev)
        d_lab = torch.full((n, 2 * N), -99, dtype=torch.int8, device=dev)
        ctx.segment_frames_device(n, d_rgb.data_ptr(), d_depth.data_ptr(), calib, 0, d_marg.data_ptr(), d_lab.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream)
        assert ctx.poll_status(wait=True) == 0
        assert ctx.last_schedule()["splat"] == name
        assert ctx.last_schedule()["planner_fallback"] == 0   # the resident run really ran resident
        torch.cuda.synchronize(dev)
        results.append((d_marg, d_lab))
        ctx.close()
    assert torch.equal(results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1])
    assert (results[0][1] != -99).all()
    forest = oracle.Forest(blob)
    p = oracle.default_params(width=W, height=H, dcrf_iterations=10)
    _, marg, lab = oracle.segment_frame(p, forest, 1, rgb[5], depth[5], calib, label_mode=1, unknown=[7, 8])
    assert np.array_equal(results[0][0][5].cpu().numpy(), marg)
    assert np.array_equal(results[0][1][5].cpu().numpy(), lab)


def test_one_large_frame_two_layers_scan_blocks_on_two_streams(gpu_ctx_factory, oracle):
    """One 1280x960 frame with two label layers: the 8- and the 9-class mean field run side by side on two streams, both
    through the list-major launch whose longest lists (here up to ~3 x 10^5 entries) go to scan blocks -- two adder waves
    shapes (classes split 4 + 4 and 3 + 3 + 3), producers alternating over 256-entry tiles.  Marginals and labels of
    both layers against the CPU oracle, bit for bit; and the same call with the serial adder only."""
    W, H = 1280, 960
    blob = synthetic.make_forest_bytes(seed=29, n_trees=4, leaves_per_tree=512, max_depth=14)
    rgb, depth = synthetic.make_batch(1, W, H, holes=True, start=7)
    calib = synthetic.make_calib(W, H)
    kw = dict(width=W, height=H, multi_layer=1, use_dense_crf=1, dcrf_iterations=4, label_mode=1, unknown_label=[7, 8], max_batch=1)
    forest = oracle.Forest(blob)
    p = oracle.default_params(width=W, height=H, dcrf_iterations=4)
    _, marg, lab = oracle.segment_frame(p, forest, 1, rgb[0], depth[0], calib, label_mode=1, unknown=[7, 8])
    for serial in (0, 1):
        ctx = gpu_ctx_factory(schedule=dict(serial_chains=serial), **kw)
        ctx.forest_load(blob)
        out = ctx.segment_frames(rgb, depth, calib, want_posteriors=False)
        assert ctx.last_schedule()["splat"] == "list-major" and ctx.last_schedule()["longest_list"] >= 16384
        assert np.array_equal(out["marginals"][0], marg), serial
        assert np.array_equal(out["labels"][0].ravel(), lab), serial
