"""Data recipes for the limits of the forest walk (csrc/kernels_rf.hip, forest_eval_kernel of
csrc/kernels_forest_tools.hip, rvseg_api.cpp: upload_forest) and of the feature kernels
(csrc/kernels_features.hip) -- a plain helper module like train_cases.py and fusion_cases.py: the CPU pins
(test_frame_cases_cpu.py: numpy and the oracle alone show that a recipe lies on the side of the edge it claims) and the
GPU comparisons (test_gpu_forest_limits.py, test_gpu_feature_limits.py: GPU == oracle, float32 bit patterns) draw the
same bytes from here.

The switches the recipes are built around:
  upload_forest         8-byte nodes while the model has fewer than 2^20 nodes (20-bit child index), else 16-byte nodes
  forest_eval_kernel    4 lanes per point up to 4 trees, 16 from 5 trees; leaf_rows[64 / lanes]; 64 trees at most
  rf_frames_lazy_kernel 16 points per wave, 4 lanes per point, leaf_rows[16], adds in groups of four with a clamped tail;
                        resize records in LDS up to 160 rows (40 KB), through L1 from 161; `wave_inside`:
                        x0 >= 0 && y0 >= 0 && x0 + size < W && y0 + size <= H for every valid point of the wave
  window_map_kernel     80 x 44 tiles with a 10-pixel apron;  normal feature: 16 x 8 sample tiles in LDS for stride <= 2,
                        the gather kernel from stride 3;  to_fix32: the magic-number branch below 2^19, clamp at 9e18
"""
import struct

import numpy as np

from rovinasemanticsegmentation_amd import synthetic

NODES8_LIMIT = 1 << 20      # upload_forest: 8-byte nodes below this many nodes
RT_LDS_ROWS = 160           # launch_rf_frames: resize records in LDS up to 40 KB = 160 rows of 256 B
DM_TW, DM_TH = 80, 44       # window_map_kernel tile
FIX_SMALL = float(1 << 19)  # to_fix32: |v| below this takes the magic-number branch
FIX_CLAMP = 9.0e18 / 4294967296.0   # |v| above this is clamped


def bits(a):
    """float32 bit patterns: NaN and -0.0 count in a comparison"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- forest.dat -----------------------------------------------------------------------------------------------------
def split_features(blob):
    """Features the inner nodes of a forest.dat split on (stream layout: int32 T, then per tree vec<int32> features,
    vec<float> thresholds, vec<int32> left children, the histograms and the multi-histograms)."""
    pos, used = 4, set()
    for _ in range(struct.unpack_from("<i", blob, 0)[0]):
        n = struct.unpack_from("<i", blob, pos)[0]
        feat = np.frombuffer(blob, np.int32, n, pos + 4)
        left = np.frombuffer(blob, np.int32, n, pos + 4 + 4 * n + 4 + 4 * n + 4)
        used |= set(np.unique(feat[left != 0]).tolist())
        pos += 3 * (4 + 4 * n)
        for _vec in range(2):   # histograms, multi_histograms: skip by walking the length prefixes
            cnt = struct.unpack_from("<i", blob, pos)[0]
            pos += 4
            if _vec == 0 and not np.frombuffer(blob, np.int32, cnt, pos).any():
                pos += 4 * cnt      # no single-label histograms at all
                continue
            for _i in range(cnt):
                m = struct.unpack_from("<i", blob, pos)[0]
                pos += 4
                if _vec == 0:
                    pos += 4 * m
                else:
                    for _l in range(m):
                        c = struct.unpack_from("<i", blob, pos)[0]
                        pos += 4 + 4 * c
    assert pos == len(blob)
    return used


def complete_left(depth, extra=()):
    """Left-child array of a complete binary tree with `depth` levels of splits, breadth first (node i -> 2i + 1, 2i + 2),
    then one more split per entry of `extra`: a node that is a leaf at that moment, whose two children are appended."""
    n_inner = (1 << depth) - 1
    n = 2 * n_inner + 1
    left = np.zeros(n + 2 * len(extra), np.int32)
    left[:n_inner] = 2 * np.arange(n_inner, dtype=np.int32) + 1
    for v in extra:
        assert v < n and left[v] == 0
        left[v] = n
        n += 2
    return left


def node_levels(left):
    lev = np.zeros(len(left), np.int32)
    frontier, l = np.zeros(1, np.int64), 0
    while frontier.size:
        kids = left[frontier]
        kids = kids[kids != 0].astype(np.int64)
        frontier = np.concatenate([kids, kids + 1])
        l += 1
        lev[frontier] = l
    return lev


def make_tree(left, feat, thr, rng, S):
    """A tree of the writer: leaves get feature 0 / threshold 0 and random log-histogram rows (in node order)."""
    left = np.asarray(left, np.int32)
    leaf = left == 0
    p = 1e-3 + (1 - 1e-3) * rng.random((int(leaf.sum()), S))
    rows = np.log(p / p.sum(1, keepdims=True)).astype(np.float32)
    return dict(left=left, feat=np.where(leaf, 0, feat).astype(np.int32), thr=np.where(leaf, 0, thr).astype(np.float32), rows=rows)


def write_forest(trees, layers):
    """libforest stream (classifier.cpp:144-152, 210-220) of `trees` (make_tree) with the label layers `layers` (class
    counts, their sum = the width of a leaf row) and no single-label histograms.  Vectorised: 2^20 nodes take a moment."""
    S, L = sum(layers), len(layers)
    out = [struct.pack("<i", len(trees))]
    reclen = 1 + L + S                      # a leaf's multi-histogram record: L, then per layer C_l and C_l floats
    for t in trees:
        left = np.ascontiguousarray(t["left"], np.int32)
        n, leaf = len(left), left == 0
        rows = np.ascontiguousarray(t["rows"], np.float32)
        assert rows.shape == (int(leaf.sum()), S)
        rec = np.empty((rows.shape[0], reclen), np.int32)
        rec[:, 0] = L
        pos = o = 1
        o = 0
        for c in layers:
            rec[:, pos] = c
            rec[:, pos + 1:pos + 1 + c] = rows[:, o:o + c].view(np.int32)
            pos += 1 + c
            o += c
        off = np.concatenate([[0], np.cumsum(np.where(leaf, reclen, 1))])   # inner nodes: one word, 0 layers
        flat = np.zeros(int(off[-1]), np.int32)
        flat[(off[:-1][leaf][:, None] + np.arange(reclen)).ravel()] = rec.ravel()
        head = struct.pack("<i", n)
        out += [head, np.ascontiguousarray(t["feat"], np.int32).tobytes(), head, np.ascontiguousarray(t["thr"], np.float32).tobytes(),
                head, left.tobytes(), head, bytes(4 * n), head, flat.tobytes()]
    return b"".join(out)


def walk(trees, X, nodes=False):
    """The plain walker: float32 compare, left on x < t, right (left + 1) otherwise; tree 0's leaf row is copied, trees
    1 .. T-1 are added in order with float32 adds (classifier.cpp:97-117, 187-208).  nodes=True: the leaf node ids (T, P)."""
    X = np.ascontiguousarray(X, np.float32)
    idx, out, reached = np.arange(len(X)), None, []
    for t in trees:
        left, feat, thr = t["left"], t["feat"], t["thr"].astype(np.float32)
        node = np.zeros(len(X), np.int64)
        while (left[node] != 0).any():
            with np.errstate(invalid="ignore"):
                go_left = X[idx, feat[node]] < thr[node]
            node = np.where(left[node] != 0, left[node] + 1 - go_left, node)
        rows = t["rows"][(np.cumsum(left == 0) - 1)[node]]
        out = rows.copy() if out is None else out + rows
        reached.append(node)
    return np.stack(reached) if nodes else out


# ---- feature layout -------------------------------------------------------------------------------------------------
def layout(r, patch=True):
    """(n_patch, pos_depth, pos_height, pos_normal, D) with every scalar feature on"""
    n = 3 * r * r if patch else 0
    return n, n, n + 1, n + 2, n + 3


def _thresholds(feat, n_patch, rng):
    """Random thresholds in the value range of each feature: bytes (a third of them integers: ties), depth in metres,
    height, normal (a fifth of them exactly -2, the value of a point without a normal)."""
    u = rng.random(len(feat))
    thr = np.floor(u * 256) + np.where(rng.random(len(feat)) < 0.34, 0.0, 0.5)
    thr = np.where(feat == n_patch, 0.5 + 14.5 * u, thr)
    thr = np.where(feat == n_patch + 1, -1.0 + 3.0 * u, thr)
    thr = np.where(feat == n_patch + 2, np.where(u < 0.2, -2.0, (u - 0.2) / 0.8 * (np.pi / 2)), thr)
    return thr.astype(np.float32)


# ---- recipes 1 and 2: tree counts, class sums, point counts -------------------------------------------------------------
EVAL_TREES = (1, 2, 3, 4, 5, 15, 16, 17, 32, 63, 64)
FRAME_TREES = (1, 3, 4, 5, 7, 8, 9, 63, 64)
CLASS_SUMS = (1, 3, 4, 5, 15, 16, 17, 63, 64)
POINT_COUNTS = (1, 15, 16, 17, 63, 64, 65, 257)
EVAL_D = 6      # patch_size_reduce 1: three patch bytes and the three scalars


def small_forest(seed, T, S, D, depth=3, n_patch=None):
    """T complete trees of `depth` levels (8 leaves for depth 3), one layer of S classes; features go round all D so
    that T * (2^depth - 1) >= D inner nodes split on every feature.  Returns (trees, blob)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(D)
    n_inner, trees = (1 << depth) - 1, []
    for t in range(T):
        left = complete_left(depth)
        feat = np.zeros(len(left), np.int64)
        feat[:n_inner] = perm[(t * n_inner + np.arange(n_inner)) % D]
        trees.append(make_tree(left, feat, _thresholds(feat, D - 3 if n_patch is None else n_patch, rng), rng, S))
    return trees, write_forest(trees, [S])


def eval_points(seed, P, D=EVAL_D):
    """Byte-valued points (every column), so that the integer thresholds of _thresholds tie"""
    return np.random.default_rng(seed).integers(0, 256, (P, D)).astype(np.float32)


# ---- recipe 3: degenerate trees ---------------------------------------------------------------------------------------
CHAIN_DEPTH = 1000


def chain_left(right, depth=CHAIN_DEPTH):
    """A chain: the root splits, then always the left (right=False) or always the right child splits again"""
    return complete_left(0, [0] + [2 * k - (0 if right else 1) for k in range(1, depth)])


def degenerate_forests(seed, S=3, D=EVAL_D):
    """name -> (trees, blob, max_depth)"""
    rng = np.random.default_rng(seed)
    def tree(left):
        feat = rng.integers(0, D, len(left))
        return make_tree(left, feat, _thresholds(feat, D - 3, rng), rng, S)
    def chain(right):
        # the chain is followed to its end by the points that keep passing: thresholds that let most of them pass
        left = chain_left(right)
        feat = rng.integers(0, 3, len(left))
        thr = np.where(rng.random(len(left)) < 0.002, 128.0, -1.0 if right else 256.0)
        return make_tree(left, feat, thr, rng, S)
    out = {}
    out["all_roots_leaves"] = ([tree(complete_left(0)) for _ in range(5)], 0)
    out["one_root_leaf"] = ([tree(complete_left(3)), tree(complete_left(0)), tree(complete_left(2))], 3)
    out["left_chain"] = ([chain(False)], CHAIN_DEPTH)
    out["right_chain"] = ([tree(complete_left(1)), chain(True)], CHAIN_DEPTH)
    return {k: (t, write_forest(t, [S]), d) for k, (t, d) in out.items()}


DENORM = np.float32(1e-45)


# ---- recipe 4: special values --------------------------------------------------------------------------------------------
def stump_forests(specials, seed, S=3, filler=None):
    """One stump (root + two leaves) per (feature, threshold) of `specials`, at most 64 trees per forest (63 with a
    `filler` tree appended, which carries the model over a node-format limit).  Returns [(trees, blob)]."""
    rng = np.random.default_rng(seed)
    per = 63 if filler is not None else 64
    out = []
    for i in range(0, len(specials), per):
        trees = [make_tree(complete_left(1), np.array([f, 0, 0]), np.array([t, 0, 0], np.float32), rng, S) for f, t in specials[i:i + per]]
        if filler is not None:
            trees.append(filler)
        out.append((trees, write_forest(trees, [S])))
    return out


SPECIAL_X = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-40, 7.0, 6.5, 7.5, -1.0, 255.0], np.float32)


def special_eval_case():
    """Points whose columns run through SPECIAL_X (each column rotated differently) and one stump per column and special
    threshold: +-inf, NaN, -0.0 (against a feature of +0.0), a denormal, 7 against 7 and 7 +- 0.5."""
    n = len(SPECIAL_X)
    X = np.stack([np.roll(SPECIAL_X, c) for c in range(EVAL_D)], 1)
    X = np.concatenate([X, np.stack([np.roll(SPECIAL_X, 2 * c + 1) for c in range(EVAL_D)], 1)])
    thr = [-np.inf, np.inf, np.nan, -0.0, 0.0, DENORM, -DENORM, 7.0, 6.5, 7.5]
    specials = [(f, np.float32(t)) for f in range(EVAL_D) for t in thr]
    assert len(X) == 2 * n
    return X, specials


def special_frame_thresholds(X, r, depth_mm):
    """Special thresholds for a frame whose oracle features are X (P, D): per patch channel a byte value k that occurs,
    and k +- 0.5; -0.0 on a patch feature that is +0.0 somewhere; +-inf and NaN; for the depth feature exactly
    float32(d) / float32(1000) and both float32 neighbours, for depths d of the frame; -2.0 on the normal."""
    n_patch, pd, ph, pn, _ = layout(r)
    sp = []
    for f in (0, 1, 2, n_patch - 1):
        k = np.float32(np.sort(X[:, f])[len(X) // 2])
        sp += [(f, k), (f, k - np.float32(0.5)), (f, k + np.float32(0.5))]
    zero = [f for f in range(n_patch) if (X[:, f] == 0).any() and (X[:, f] > 0).any()]
    sp += [(zero[0], np.float32(-0.0)), (zero[0], DENORM)]
    sp += [(1, np.float32(-np.inf)), (1, np.float32(np.inf)), (1, np.float32(np.nan)), (pd, np.float32(np.nan)), (pn, np.float32(np.nan))]
    for d in depth_mm:
        t = np.float32(d) / np.float32(1000)
        sp += [(pd, t), (pd, np.nextafter(t, np.float32(-np.inf))), (pd, np.nextafter(t, np.float32(np.inf)))]
    sp += [(pn, np.float32(-2.0)), (pn, np.nextafter(np.float32(-2.0), np.float32(0)))]
    med = np.float32(np.median(X[:, ph]))
    sp += [(ph, med), (ph, np.nextafter(med, np.float32(np.inf)))]
    return sp


# ---- frames -----------------------------------------------------------------------------------------------------------
def small_frame(seed, W=64, H=48, lo=600, hi=15000, black=True):
    """Random colour (a black block: Lab bytes of exactly 0) over a smooth depth ramp with a few holes, so that the
    normal feature takes values as well as -2."""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if black:
        rgb[H // 3:H // 3 + 6, W // 4:W // 4 + 12] = 0
    ys, xs = np.mgrid[0:H, 0:W]
    depth = (lo + (hi - lo) * (xs + 0.5 * ys) / (W + 0.5 * H)).astype(np.uint16)
    depth[rng.random((H, W)) < 0.01] = 0
    return rgb, depth


def special_depths(depth):
    """Three depths (mm) of a frame: near, middle and far"""
    u = np.unique(depth[depth > 0])
    return u[[3, len(u) // 2, -3]]


FRAME_KW = dict(width=64, height=48, stride=1, patch_size=9, patch_size_reduce=3)


# ---- recipe 5: node formats ---------------------------------------------------------------------------------------------
BIG_DEPTH = 19


def big_tree(seed, depth, r, extra=(), S=2):
    """A complete tree of `depth` levels on the features of patch_size_reduce r.  Five nodes of eight split on patch
    cells (going round all of them), one each on depth, height and normal, mixed so that every level from the third on
    has all four kinds.  The nodes on the right spine below the root send every point right (byte < 0, depth < 0,
    height < -inf, normal < -2 never hold; -2.0 is a tie), so the points the root sends right arrive below the last
    inner node -- the largest child indices of the model; `extra` splits go on from there."""
    rng = np.random.default_rng(seed)
    n_patch, pd, ph, pn, D = layout(r)
    left = complete_left(depth, extra)
    n = len(left)
    ids = np.arange(n, dtype=np.int64)
    lev = node_levels(left)
    kind = (ids + lev) % 8
    feat = np.where(kind < 5, (ids * 7 + lev) % n_patch, n_patch + kind - 5)
    thr = _thresholds(feat, n_patch, rng)
    spine = (1 << np.arange(2, depth + 1)) - 2          # nodes 2, 6, 14, ...: the right spine below the root
    never = np.where(feat[spine] == ph, -np.inf, np.where(feat[spine] == pn, -2.0, 0.0))
    thr[spine] = never.astype(np.float32)
    feat[0], thr[0] = pd, np.float32(6.0)              # the root: depth below / above 6 m
    return make_tree(left, feat, thr, rng, S)


def big_models(r, seed=5):
    """name -> (trees, blob, node total): the three models around the 2^20-node switch of upload_forest"""
    last = (1 << (BIG_DEPTH + 1)) - 2                   # the last leaf of the complete tree
    half_last = (1 << BIG_DEPTH) - 2
    out = {
        "compact_full": [big_tree(seed, BIG_DEPTH, r)],                             # 2^20 - 1: 20-bit child index full
        "wide_plus_one_split": [big_tree(seed, BIG_DEPTH, r, extra=(last,))],       # 2^20 + 1: 16-byte nodes
        "wide_two_trees": [big_tree(seed + 1, BIG_DEPTH - 1, r), big_tree(seed + 2, BIG_DEPTH - 1, r, extra=(half_last,))],   # 2^20
    }
    return {k: (t, write_forest(t, [2]), sum(len(x["left"]) for x in t)) for k, t in out.items()}


# ---- recipe 6: wave_inside -------------------------------------------------------------------------------------------
HALF_DEPTH_MM = {0: 5000, 1: 3000, 4: 1000, 9: 500}     # patch_size 9: half = int(9 / (2 d))


def oracle_half(patch_size, depth_mm):
    """feature_extractor.h:139-140 as the oracle restates it: float32 metres, double division, truncation"""
    return int(patch_size / (2.0 * float(np.float32(depth_mm) / np.float32(1000))))


def roi_inside(x, y, half, W, H):
    """kernels_rf.hip: the predicate of the fast path.  Asymmetric on purpose: the 8-byte tap load at the ROI's last
    column must not be the image's last column, while the row pair of the last row exists (prep_kernel duplicates it)."""
    x0, y0, size = x - half, y - half, 2 * half + 1
    return x0 >= 0 and y0 >= 0 and x0 + size < W and y0 + size <= H


def wave_inside_frames(seed, W=64, H=48):
    """Frames of depth 0 with single valid sample points (stride 1: a wave is 16 consecutive pixels of a row), one point
    per wave, on both sides of each of the four comparisons of roi_inside and in the four corners, for every half of
    HALF_DEPTH_MM; plus one wave with an inside and an outside point.  Returns (rgb, depth, points) with points =
    [(frame, x, y, half, inside)]."""
    pts = []
    for half in HALF_DEPTH_MM:
        xs = [half - 1, half, W - 2 - half, W - 1 - half]        # x - half in {-1, 0};  x + half + 1 in {W - 1, W}
        ys = [half - 1, half, H - 1 - half, H - half]            # y - half in {-1, 0};  y + half + 1 in {H, H + 1}
        cand = [(x, H // 2) for x in xs] + [(W // 2, y) for y in ys] + [(x, y) for x in xs for y in ys]
        pts += [(x, y, half) for x, y in cand if 0 <= x < W and 0 <= y < H]
    frames, used = [], []
    placed = []
    for x, y, half in pts:
        wave = (y, x // 16)
        for f in range(len(used) + 1):
            if f == len(used):
                used.append(set())
            if wave not in used[f]:
                used[f].add(wave)
                placed.append((f, x, y, half))
                break
    # the mixed wave: an inside and an outside point of half 4 in one run of 16 pixels
    f = len(used)
    placed += [(f, 3, 20, 4), (f, 9, 20, 4)]
    rng = np.random.default_rng(seed)
    n = f + 1
    rgb = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    depth = np.zeros((n, H, W), np.uint16)
    out = []
    for f, x, y, half in placed:
        depth[f, y, x] = HALF_DEPTH_MM[half]
        out.append((f, x, y, half, roi_inside(x, y, half, W, H)))
    return rgb, depth, out


def patch_forest(seed, r, T=32, depth=5, S=2):
    """A forest that splits on every patch feature of r (and the three scalars): T * (2^depth - 1) inner nodes going
    round the features; a single point walks T * depth of them."""
    D = layout(r)[4]
    assert T * ((1 << depth) - 1) >= D
    return small_forest(seed, T, S, D, depth, n_patch=D - 3)


# ---- recipe 7: resize table in LDS / through L1 -----------------------------------------------------------------------
def near_plane_frame(seed, W=192, H=164):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ys, xs = np.mgrid[0:H, 0:W]
    depth = (600 + 14400 * ((xs * 5 + ys * 3) % 101) / 100.0).astype(np.uint16)
    depth[:, :W // 2] = 500
    return rgb, depth


# ---- recipe 8: patch_size_reduce 1 and 16 ----------------------------------------------------------------------------------
def halves_frame(seed, W=64, H=48):
    """patch_size 9: quarters of half 0 (5 m), 3 (1.4 m), 8 (0.55 m) and 9 = patch_size (0.5 m)"""
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    depth = np.empty((H, W), np.uint16)
    depth[:H // 2, :W // 2], depth[:H // 2, W // 2:] = 5000, 1400
    depth[H // 2:, :W // 2], depth[H // 2:, W // 2:] = 550, 500
    return rgb, depth


# ---- recipe 9: validity at the limits ---------------------------------------------------------------------------------
DEPTH_LIMITS = ((0.5, 15.0), (0.7, 1.3), (0.3, 65.535), (0.7005, 1.2995), (1.0, 1.0))


def limits_frame(dmin, dmax, W=64, H=48):
    """Every depth within +-3 mm of both limits, plus 0 and 65535, repeated over the image"""
    vals = {0, 65535}
    for lim in (dmin, dmax):
        vals |= set(range(int(np.floor(lim * 1000)) - 3, int(np.ceil(lim * 1000)) + 4))
    vals = np.array(sorted(v for v in vals if 0 <= v <= 65535), np.uint16)
    ys, xs = np.mgrid[0:H, 0:W]
    depth = vals[(xs + 5 * ys) % len(vals)]
    rgb = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return rgb, depth, vals


# ---- recipes 10 and 11: image sizes, strides --------------------------------------------------------------------------
IMAGE_SIZES = ((21, 21), (30, 24), (80, 44), (81, 45), (79, 43), (160, 88), (161, 89), (64, 4), (128, 8))
STRIDE_CASES = ((1, 33, 25), (1, 47, 31), (2, 66, 50), (2, 94, 62),      # lw % 16 in {1, 15}, lh % 8 in {1, 7}: partial tiles
                (3, 120, 90), (5, 120, 90), (8, 120, 88))                # the gather kernel


def size_calib():
    """The stock 640 x 480 calibration for every image size: scaled down with a tiny image, its focal length would make
    neighbouring rows differ by more than PCL's depth-change threshold, and no pixel would have a normal."""
    return synthetic.make_calib()


def smooth_depth(W, H):
    ys, xs = np.mgrid[0:H, 0:W]
    return (2000 + 3 * xs + 2 * ys + 40 * np.sin(xs / 37.0) * np.cos(ys / 23.0)).astype(np.uint16)


def size_frames(W, H, seed=0):
    """Depth images of one size: smooth; with random isolated holes; and, where the image has a window-map seam, one
    image per k in 8..11 with isolated holes k pixels from the first pixel on either side of each seam, horizontally,
    vertically and diagonally."""
    rng = np.random.default_rng(seed + W * 1000 + H)
    frames = [smooth_depth(W, H)]
    d = smooth_depth(W, H)
    d[rng.random((H, W)) < 0.004] = 0
    frames.append(d)
    sx, sy = list(range(DM_TW, W, DM_TW)), list(range(DM_TH, H, DM_TH))
    if sx or sy:
        for k in (8, 9, 10, 11):
            d = smooth_depth(W, H)
            def hole(y, x):
                if 0 <= y < H and 0 <= x < W:
                    d[y, x] = 0
            for s in sx:
                hole(H // 4, s - k)            # k pixels left of column s, the first of the right tile
                hole(3 * H // 4, s - 1 + k)    # k pixels right of column s - 1, the last of the left tile
            for s in sy:
                hole(s - k, W // 5)
                hole(s - 1 + k, 4 * W // 5)
            for s in sx:
                for t in sy:
                    hole(t - k, s - k)
                    hole(t - 1 + k, s - 1 + k)
            frames.append(d)
    return frames


def holes_depth(W, H, seed):
    rng = np.random.default_rng(seed)
    d = smooth_depth(W, H)
    d[rng.random((H, W)) < 0.006] = 0
    return d


# ---- recipe 12: large coordinates ----------------------------------------------------------------------------------------
def scaled_calib(log2_scale):
    """The stock 640 x 480 calibration with R scaled.  Its principal point lies far outside the 96 x 64 frames it is used
    on, which they need: PCL's depth-change test is relative once |z| >> 1, and around the principal row neighbouring
    rows differ by more than 4 % of z, so that no pixel there has a normal."""
    c = synthetic.make_calib().copy()
    c[9:18] *= np.float32(2.0 ** log2_scale)     # R; a power of two changes no rounding step before the overflow
    return c


def large_frame(W=96, H=64):
    d = smooth_depth(W, H)
    d[20, 30] = d[40, 70] = d[33, 50] = 0
    return d


def window_fix_sums(cloud, dist, y, x):
    """True window sums (Python integers) of the 2^-32 fixed-point x gradients at pixel (y, x), per coordinate"""
    rect = int(min(dist[y, x], 10.0))
    sums = [0, 0, 0]
    for yy in range(y - rect // 2, y - rect // 2 + rect):
        for xx in range(x - rect // 2, x - rect // 2 + rect):
            g = cloud[yy, xx + 1] - cloud[yy, xx - 1]
            if np.isfinite(g).all():
                for k in range(3):
                    s = min(max(float(g[k]) * 4294967296.0, -9.0e18), 9.0e18)
                    sums[k] += int(np.rint(s))
    return sums


# ---- recipe 13: normals at the ends of acos ---------------------------------------------------------------------------
def identity_calib():
    return np.concatenate([np.eye(3).ravel(), np.eye(3).ravel(), np.zeros(3)]).astype(np.float32)


def camera_calib(W, H):
    """R = I, t = 0 and the stock K^-1: base z is the optical axis, so |n_z| is the cosine of a plane's tilt"""
    c = synthetic.make_calib(W, H).copy()
    c[9:18] = np.eye(3, dtype=np.float32).ravel()
    c[18:21] = 0
    return c


TILT_SLOPES = (0.0, 2.0, 12.0, 30.0, 60.0, 100.0)   # mm of depth per pixel; 100 stays under PCL's depth-change threshold


def tilted_depth(W, H, axis, slope, lo=1500.0):
    """A surface tilted about one image axis: the depth rises by `slope` mm per pixel along the other"""
    ys, xs = np.mgrid[0:H, 0:W]
    return (lo + slope * (xs if axis == "y" else ys)).astype(np.uint16)
