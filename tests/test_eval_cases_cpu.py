"""CPU pins of the recipes in eval_cases.py: numpy alone shows that every recipe lies on the edge of
csrc/kernels_eval.hip it claims, so a change of a generator fails here and never silently moves a GPU test
(test_gpu_eval_limits.py) off its edge.  The hash is restated only to place colours (eval_cases.color_hash); expected
labels and counts come from the dict, the 256-entry table and np.bincount."""
import numpy as np
import pytest

import eval_cases as ec


# ---- the references on cases small enough to state by hand ----------------------------------------------------------------
def test_references_by_hand():
    coding = ec.entries([[1, 2, 3], [9, 8, 7], [1, 2, 3], [4, 4, 4]], [5, -1, 6, 5])
    rgb = np.array([[1, 2, 3], [9, 8, 7], [4, 4, 4], [0, 0, 0], [1, 2, 4]], np.uint8)
    assert ec.ref_decode(rgb, coding, -7).tolist() == [6, -1, 5, -7, -7]              # the later entry of a colour wins
    assert ec.ref_encode(np.array([5, 6, -1, 0, 127], np.int8), coding).tolist() == [[4, 4, 4], [1, 2, 3], [9, 8, 7], [0, 0, 0], [0, 0, 0]]
    pred = np.array([0, 1, -1, 127, 2, 1, -1], np.int8)
    gt = np.array([1, 1, 127, -128, 0, 2, -1], np.int8)
    counts, oor, skipped = ec.ref_confusion(pred, gt, 2)
    assert counts.tolist() == [[0, 0], [1, 1]] and oor == 2 and skipped == 3         # (-1, 127), (127, -128): skipped
    assert counts.dtype == np.uint64
    assert ec.keys_of(ec.colors_of([0x123456])).tolist() == [0x123456]
    # the restated hash: top nine bits of the 32-bit product
    assert int(ec.color_hash(1)) == 2654435761 >> 23 and int(ec.color_hash(0)) == 0
    assert int(ec.color_hash(0xffffff)) == ((0xffffff * 2654435761) % (1 << 32)) >> 23


# ---- wrap_cluster -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wrap():
    return ec.wrap_cluster()


def test_wrap_cluster_crosses_the_wrap(wrap):
    keys = wrap["keys"]
    assert len(wrap["coding"]) == 256 and len(set(keys.tolist())) == 256              # the load is exactly 256
    assert set(ec.color_hash(keys).tolist()) == {509, 510, 511}
    slots, probes, slot_of = ec.insert_slots(keys)
    used = np.flatnonzero(slot_of >= 0)
    assert len(used) == 256 and slot_of[511] >= 0 and slot_of[0] >= 0
    assert sorted((used - 509) % 512) == list(range(256))                             # contiguous modulo 512: 509 .. 252
    assert probes.max() >= 200 and probes[-1] == probes.max() and slots[-1] == 252
    assert ((slots < 509) & (probes > 0)).sum() >= 250                                # these chains cross 511 -> 0
    labels = set(wrap["labels"].tolist())
    assert {-128, -1, 0, 127} <= labels and len(labels) < 256                         # extremes, and repeats
    assert len(ec.decode_dict(wrap["coding"])) == 256


def test_wrap_cluster_unknown_colours(wrap):
    cl, table = wrap["classes"], set(wrap["keys"].tolist())
    _, _, slot_of = ec.insert_slots(wrap["keys"])
    for name, keys in cl.items():
        assert len(keys) >= 2, name
        if name != "table":
            assert not (set(keys.tolist()) & table), name
    assert (ec.color_hash(cl["miss_whole_cluster"]) == 509).all() and slot_of[253] < 0   # 256 occupied slots, then the empty one
    h = ec.color_hash(cl["miss_inside_cluster"])
    assert (h <= 252).all() and (slot_of[h.astype(np.int64)] >= 0).all()
    h = ec.color_hash(cl["miss_empty_half"])
    assert ((h >= 254) & (h <= 508)).all() and (slot_of[h.astype(np.int64)] < 0).all()
    assert cl["black_white"].tolist() == [0, 0xffffff]
    d = np.abs(ec.colors_of(cl["neighbours"]).astype(int)[:, None] - ec.colors_of(wrap["keys"]).astype(int)[None]).sum(-1)
    assert (d.min(1) == 1).all()                                                      # one step in one channel


def test_wrap_stream_holds_every_class(wrap):
    cl = wrap["classes"]
    # 16 pixels: one colour of every class, black, white and the colour at the end of the longest chain
    for seed in range(3):
        s = set(ec.wrap_stream(wrap, 16, seed).tolist())
        assert all(s & set(v.tolist()) for v in cl.values()) and {0, 0xffffff, int(wrap["keys"][255])} <= s
    # 67 frames of 16 pixels: every colour of every class
    s = set(ec.wrap_stream(wrap, 67 * 16).tolist())
    assert all(set(v.tolist()) <= s for v in cl.values())
    want = ec.ref_decode(ec.colors_of(ec.wrap_stream(wrap, 67 * 16)), wrap["coding"], -1)
    assert (want == -1).sum() >= 100 and len(set(want.tolist())) > 100


# ---- alternating ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total,stride,run_len", [(16, 4096, 0), (400, 4096, 7), (15617, 4096, 4103), (3 * 15617, 4096, 4103),
                                                   (4 * 640 * 480, 1 << 20, (1 << 20) + 7)])
def test_alternating_runs(total, stride, run_len):
    a = ec.alternating(total, 2, stride)
    keys = a["keys"]
    if not run_len:                              # one chunk: the two colours alternate, and there is no room for a run
        assert a["runs"] == [] and len(keys) == total and set(keys.tolist()) == set(a["pair"]) | {a["unknown"]}
        return
    assert a["run_len"] == run_len and run_len % ec.BLOCK_PIXELS == 7 and len(a["runs"]) >= 1
    x, y = a["pair"]
    assert int(ec.color_hash(x)) == int(ec.color_hash(y)) == int(ec.color_hash(a["unknown"])) == 511
    table = ec.decode_dict(a["coding"])
    assert tuple(ec.colors_of([x])[0]) in table and tuple(ec.colors_of([a["unknown"]])[0]) not in table
    head = keys[:5 * ec.CHUNK + 2]
    assert (head[1:] != head[:-1]).all() and set(head.tolist()) == {x, y, a["unknown"]}   # a new colour every pixel
    for start, length, key in a["runs"]:
        assert (keys[start:start + length] == key).all() and keys[start - 1] != key and keys[start + length] != key
        assert len(set(a["pred"][start:start + length].tolist())) == 1                # one (pred, gt) pair per run
        assert start % ec.CHUNK == 3 and (start + length) % ec.CHUNK == 10            # starts and ends inside a chunk
        if length > stride:
            # the lane of the run's first chunk meets the run again in its next chunk, `stride` pixels on
            assert start // ec.CHUNK + stride // ec.CHUNK == (start + length - 1) // ec.CHUNK


def test_grid_stride_case_reaches_a_second_chunk():
    for cus in (256, 304, 64):
        n = ec.grid_stride_frames(cus)
        blocks = ec.launch_blocks(cus, 8, 16)
        assert blocks == ec.launch_blocks(cus, 8) == cus                              # 8 * CUs / 8 for both launches
        chunks = ec.GRID_W * ec.GRID_H // ec.CHUNK
        assert n * chunks > ec.THREADS * blocks >= (n - 1) * chunks
    assert ec.grid_stride_frames(256) == 4
    assert ec.launch_blocks(256, 1, 64) == 512 and ec.launch_blocks(256, 1, 17) == 1024 and ec.launch_blocks(256, 2, 16) == 1024
    n, layers = ec.grid_stride_case(256)
    assert len(layers) == 8
    pairs = set()
    for a in layers:
        (start, length, key), = a["runs"]
        assert length == (1 << 20) + 7 and start + length < n * ec.GRID_W * ec.GRID_H
        pairs.add(a["pair"])
    assert len(pairs) == 8                                                            # another pair of colours per layer
    assert {int(ec.color_hash(a["pair"][0])) for a in layers} == set(range(504, 512))


# ---- layers8 ----------------------------------------------------------------------------------------------------------------
def test_layers8_shared_colours_decode_differently_per_layer():
    rc = ec.layers8()
    assert sum(ec.LAYERS8) == ec.MAX_CLASSES and len(ec.LAYERS8) == ec.MAX_LAYERS and len(rc["shared"]) >= 20
    rgb = ec.colors_of(rc["shared"])
    vec = [ec.ref_decode(rgb, rc["codings"][l]) for l in range(8)]
    for j in range(len(rc["shared"])):
        assert len({int(v[j]) for v in vec}) == 8                                     # a different label in each layer
    assert all(len(c) <= 256 for c in rc["codings"])
    streams = ec.layers8_streams(rc, 16)
    assert all(np.array_equal(streams[0][:12], s[:12]) for s in streams)              # the same bytes in every layer
    want = [ec.ref_decode(ec.colors_of(s), rc["codings"][l], -1) for l, s in enumerate(ec.layers8_streams(rc, 85))]
    assert all((w == -1).any() for w in want)
    pred, gt = ec.layers8_labels(85)
    for l, C in enumerate(ec.LAYERS8):
        counts, oor, skipped = ec.ref_confusion(pred[l], gt[l], C)
        assert oor > 0 and skipped > 0 and counts.sum() > 0
        lab = ec.table_labels_stream(rc["codings"][l], 85, l)
        assert np.array_equal(ec.ref_decode(ec.ref_encode(lab, rc["codings"][l]), rc["codings"][l]), lab)


# ---- bins, rgb_gt -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", ec.BIN_CLASSES)
def test_bins_hold_every_pair_and_the_extremes(C):
    b = ec.bins(C)
    pred, gt, m = b["pred"].astype(int), b["gt"].astype(int), b["n_norun"]
    counts, oor, skipped = ec.ref_confusion(pred[:m], gt[:m], C)
    assert (counts >= 2).all() and counts.shape == (C, C)                             # all C * C bins, at least twice
    have = set(zip(pred[:m].tolist(), gt[:m].tolist()))
    assert all((p, g) in have for p in ec.extremes(C) for g in ec.extremes(C))         # the 36 extreme pairs
    assert ((pred[1:m] != pred[:m - 1]) | (gt[1:m] != gt[:m - 1])).all()               # a new pair every pixel
    counts, oor, skipped = ec.ref_confusion(pred, gt, C)
    assert oor > 0 and skipped > 0
    assert int(counts.sum()) == len(pred) - oor - skipped                             # the total is the scored pixels
    # the run plane: A x 40, skip, A x 40, out of range, A x 40, B
    for start, A, skip, out, B in b["marks"]:
        seq = list(zip(pred[start:start + 3 * ec.RUN + 3].tolist(), gt[start:start + 3 * ec.RUN + 3].tolist()))
        assert seq == [A] * ec.RUN + [skip] + [A] * ec.RUN + [out] + [A] * ec.RUN + [B]
        assert min(skip) < 0 and min(out) >= 0 and max(out) >= C and 0 <= min(A) and max(A) < C and max(B) < C
    skips = [mk[2] for mk in b["marks"]]
    assert (-1, 127) in skips and (127, -128) in skips and (C, 0) in [mk[3] for mk in b["marks"]]


def test_bins_cases_cover_the_sizes():
    cases = ec.bins_cases()
    for C in ec.BIN_CLASSES:
        mine = [(W, H, n) for c, W, H, n in cases if c == C]
        assert (161, 97, 1) in mine and (161, 97, 67) in mine
        assert all(n * W * H >= len(ec.bins(C)["pred"]) for W, H, n in mine)
    for C in (1, 2):
        assert {(W, H) for c, W, H, n in cases if c == C and n == 67} == set(ec.SIZES)   # 67 chunks of P = 16 in one block


@pytest.mark.parametrize("C", ec.BIN_CLASSES)
def test_rgb_gt_leaves_colours_out(C):
    r = ec.rgb_gt(C)
    assert r["left_out"] and 127 in r["left_out"] and r["missing"] == (-1, 0, C)
    black = ~r["gt_rgb"].any(-1)
    assert np.array_equal(black, np.isin(r["gt"], r["left_out"])) and black.any() and not black.all()
    base = ec.ref_confusion(r["pred"], r["gt"], C)
    seen = []
    for missing in r["missing"]:
        dec = ec.ref_decode(r["gt_rgb"], r["coding"], missing)
        assert np.array_equal(dec[~black], r["gt"][~black]) and (dec[black] == missing).all()
        counts, oor, skipped = ec.ref_confusion(r["pred"], dec, C)
        assert int(counts.sum()) == len(dec) - oor - skipped
        seen.append((counts.tobytes(), oor, skipped))
    assert seen[0][2] > seen[1][2] and seen[2][1] > seen[1][1]                        # -1: more skipped; C: more out of range
    assert len({s[0] for s in seen}) >= 2 and base[1] > 0
