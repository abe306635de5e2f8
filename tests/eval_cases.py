"""Data recipes for the limits of the scoring kernels (csrc/kernels_eval.hip) -- a plain helper module
like frame_cases.py: numpy only.  The CPU pins (test_eval_cases_cpu.py) show from numpy alone that each recipe lies on
the edge it claims; the GPU comparisons (test_gpu_eval_limits.py) draw the same bytes from here and compare with exact
equality.

The references are plain restatements of the operation, not of the kernels:
  ref_decode     a Python dict (r, g, b) -> label filled in entry order (the later entry wins), default `missing`
  ref_encode     a 256-entry table "last colour of this (uint8)label, else black"
  ref_confusion  np.bincount on int64: a pair with a negative side is skipped, then a pair with a side >= C is out of range

The switches of the code the recipes are built around:
  decode_color          512-slot open-addressed hash, linear probing that wraps from slot 511 to slot 0, <= 256 entries
  the three kernels     16-pixel chunks, 256 lanes per block; a lane's next chunk lies 256 * gridDim.x chunks on; a chunk
                        takes the 16-byte path when both pointers are 16-byte aligned, the chunk is whole and its pixel
                        offset is a multiple of 16; per-lane caches (last_key / last_label, run_key / run_n) live across
                        a lane's chunks
  eval_launch           gridDim.x = min(blocks_per_cu * CUs / layers, ceil(n_chunks / 256)); blocks_per_cu 8 for the
                        conversions, 8 / 4 / 2 for the confusion at C^2 <= 256 / <= 1024 / above
  counters              [8 layers][64 * 64] uint64, then 8 out-of-range counters

`color_hash` is restated here only to choose inputs (colours of a wanted hash) and for the pins; no expected value is
computed from it."""
import numpy as np

HASH_SLOTS = 512
CHUNK = 16
THREADS = 256
BLOCK_PIXELS = CHUNK * THREADS          # 4096: pixels of one pass of one block
MAX_LAYERS = 8
MAX_CLASSES = 64

SIZES = ((4, 4), (5, 4), (5, 5), (17, 5), (161, 97))     # P = 16 (one chunk), 20 and 25 (chunk + tail), 85, 15617 (odd)
FRAME_COUNTS = (1, 3, 67)
MISSING_LABELS = (0, -1, -128, 127)
LAYERS8 = (1, 2, 3, 5, 8, 13, 16, 16)   # sum 64: the loader's limit
GRID_W, GRID_H = 640, 480


# ---- references -------------------------------------------------------------------------------------------------------
def entries(colors, labels):
    """A coding in the form of config.json: a list of {name, color, label}"""
    return [{"name": "e%d" % i, "color": [int(v) for v in c], "label": int(l)} for i, (c, l) in enumerate(zip(colors, labels))]


def keys_of(rgb):
    rgb = np.asarray(rgb)
    return rgb[..., 0].astype(np.int64) << 16 | rgb[..., 1].astype(np.int64) << 8 | rgb[..., 2].astype(np.int64)


def colors_of(keys):
    keys = np.asarray(keys, np.int64)
    return np.stack([keys >> 16 & 255, keys >> 8 & 255, keys & 255], -1).astype(np.uint8)


def decode_dict(coding):
    table = {}
    for e in coding:
        table[tuple(int(v) for v in e["color"])] = int(np.int64(e["label"]).astype(np.int8))
    return table


def ref_decode(rgb, coding, missing=0):
    """rgb (..., 3) uint8 -> int8: the dict looked up once per distinct colour of the image"""
    table = decode_dict(coding)
    uniq, inv = np.unique(keys_of(rgb).ravel(), return_inverse=True)
    lab = np.array([table.get((int(k) >> 16, int(k) >> 8 & 255, int(k) & 255), missing) for k in uniq], np.int64)
    return lab.astype(np.int8)[inv].reshape(np.shape(rgb)[:-1])


def encode_table(coding):
    lut = np.zeros((256, 3), np.uint8)
    for e in coding:
        lut[int(np.int64(e["label"]).astype(np.int8)) & 255] = [int(v) for v in e["color"]]
    return lut


def ref_encode(labels, coding):
    return encode_table(coding)[np.asarray(labels, np.int8).view(np.uint8)]


def ref_confusion(pred, gt, C):
    """(counts [gt][pred] uint64, out of range, skipped)"""
    p = np.asarray(pred).astype(np.int64).ravel()
    g = np.asarray(gt).astype(np.int64).ravel()
    skip = (p < 0) | (g < 0)                       # first: (-1, 127) is skipped, not out of range
    oor = ~skip & ((p >= C) | (g >= C))
    ok = ~skip & ~oor
    counts = np.bincount(g[ok] * C + p[ok], minlength=C * C).reshape(C, C).astype(np.uint64)
    return counts, int(oor.sum()), int(skip.sum())


# ---- choosing inputs: colours by hash ----------------------------------------------------------------------------------
def color_hash(key):
    return (np.asarray(key, np.uint64) * np.uint64(2654435761) & np.uint64(0xffffffff)) >> np.uint64(23)


_scan = {}


def scanned_keys():
    """2^21 distinct 24-bit keys spread over the colour cube, and their hashes (about 4096 keys per hash value)"""
    if not _scan:
        k = (np.arange(1 << 21, dtype=np.uint64) * np.uint64(0x9E3779) + np.uint64(12345)) % np.uint64(1 << 24)
        _scan["k"], _scan["h"] = k.astype(np.int64), color_hash(k).astype(np.int64)
    return _scan["k"], _scan["h"]


def keys_with_hash(h, count, skip=0):
    k, hs = scanned_keys()
    out = k[hs == h][skip:skip + count]
    assert len(out) == count
    return out


def insert_slots(keys):
    """Where linear probing puts `keys` (distinct, in order): (slot of each key, probes from its home).  For the pins."""
    slot_of = np.full(HASH_SLOTS, -1, np.int64)
    slots, probes = [], []
    for k in keys:
        h = int(color_hash(k))
        n = 0
        while slot_of[h] >= 0:
            h = (h + 1) % HASH_SLOTS
            n += 1
        slot_of[h] = k
        slots.append(h)
        probes.append(n)
    return np.array(slots), np.array(probes), slot_of


# ---- frames from per-layer streams ------------------------------------------------------------------------------------
def fit(stream, total):
    """`stream` (len, ...) repeated or cut to `total` pixels"""
    stream = np.asarray(stream)
    reps = -(-total // len(stream))
    return np.concatenate([stream] * reps)[:total] if reps > 1 else stream[:total]


def frames(streams, n, W, H):
    """Per-layer streams (each n * W * H pixels, in the order a layer's chunks run: frame after frame) -> (n, L, H, W[, 3])"""
    per = [np.asarray(s).reshape((n, H, W) + np.shape(s)[1:]) for s in streams]
    return np.ascontiguousarray(np.stack(per, 1))


ALL_LABELS = np.arange(-128, 128).astype(np.int8)


def label_stream(total, seed=0):
    """Every int8 value, in runs of 1, 2 and 19, for the encoder"""
    rng = np.random.default_rng(seed)
    base = np.concatenate([ALL_LABELS, np.repeat(rng.permutation(ALL_LABELS), 2), np.repeat(ALL_LABELS[::7], 19)])
    return fit(np.roll(base, -seed * 5), total)


# ---- recipe: wrap_cluster ---------------------------------------------------------------------------------------------
def wrap_cluster():
    """256 colours of hash 509, 510 and 511: the cluster runs from slot 509 over the wrap to slot 252.  `classes` names
    the colours an image is made of."""
    k509, k510, k511 = keys_with_hash(509, 90), keys_with_hash(510, 90), keys_with_hash(511, 90)
    keys = np.empty(256, np.int64)
    keys[0::3], keys[1::3], keys[2::3] = k511[:86], k509[:85], k510[:85]
    keys[255] = k509[85]                                # the last inserted: home 509, lands about 256 probes on
    labels = ((np.arange(256) * 37) % 200 - 100).astype(np.int64)
    labels[:8] = [-128, -1, 0, 127, -128, 0, 127, -1]
    table = set(keys.tolist())
    allk, allh = scanned_keys()
    free = ~np.isin(allk, keys)

    def unknown(lo, hi, count, step):
        return allk[free & (allh >= lo) & (allh <= hi)][::step][:count]
    near = []
    for k in keys[[0, 1, 2, 100, 255]]:
        for sh in (0, 8, 16):
            ch = (int(k) >> sh & 255)
            for d in (1, -1):
                if 0 <= ch + d <= 255:
                    near.append(int(k) + (d << sh))
    near = np.array([k for k in near if k not in table], np.int64)
    classes = {
        "table": keys,
        "miss_whole_cluster": allk[free & (allh == 509)][:12],        # walks 509 .. 252 before the empty slot 253
        "miss_inside_cluster": unknown(0, 252, 40, 997),
        "miss_empty_half": unknown(254, 508, 40, 1013),
        "black_white": np.array([0x000000, 0xffffff], np.int64),
        "neighbours": near,
    }
    assert not (set(classes["black_white"].tolist()) & table)
    return dict(coding=entries(colors_of(keys), labels), keys=keys, labels=labels, classes=classes)


def wrap_stream(rc, total, seed=0):
    """Colour keys of an image: one colour of each class first (so that 16 pixels hold every class), then every colour of
    every class in runs of 1 .. 3"""
    cl = rc["classes"]
    head = np.array([cl[name][(seed + i) % len(cl[name])] for i, name in enumerate(cl)] + [0x000000, 0xffffff, int(cl["table"][255])], np.int64)
    body = np.concatenate([np.roll(v, -seed) for v in cl.values()])
    rng = np.random.default_rng(seed)
    body = np.repeat(body, rng.integers(1, 4, len(body)))
    return fit(np.concatenate([head, body]), total)


# ---- recipe: alternating ----------------------------------------------------------------------------------------------
def alternating(total, C, stride=BLOCK_PIXELS, seed=0):
    """Two colours of one hash alternate pixel by pixel (every pixel misses `last_key` and probes), between runs of one
    colour of stride + 7 pixels (stride a multiple of 4096 pixels, a lane's distance between its chunks when
    gridDim.x = stride / 4096), each starting 3 pixels into a chunk.  A stream too short for a run of stride + 7 falls
    back to 4096 + 7 and then to 7.  Returns the coding, the colour stream, a prediction stream that is constant over
    each run, and the runs [(start, length, key)]."""
    h = (HASH_SLOTS - 1 - seed) % HASH_SLOTS
    a, b = keys_with_hash(h, 2, skip=seed)
    c, d = keys_with_hash((h + 1) % HASH_SLOTS, 1, skip=seed)[0], keys_with_hash(77 + seed, 1)[0]
    u = keys_with_hash(h, 1, skip=seed + 2)[0]                         # not in the table: probes past a and b
    labels = [C - 1, 0, -1, C]
    coding = entries(colors_of([a, b, c, d]), labels)
    run_len = next((s + 7 for s in (stride, BLOCK_PIXELS) if total >= s + 7 + 200), 7)   # below 131 pixels: no run at all
    keys = np.empty(total, np.int64)
    alt = np.array([a, b], np.int64)
    keys[:] = alt[np.arange(total) & 1]
    keys[5::23] = u
    pred = ((np.arange(total) // 5) % (C + 2) - 1).astype(np.int8)     # -1 .. C
    runs, pos = [], 5 * CHUNK + 3
    for i, key in enumerate((a, c, b, d, a)):
        if pos + run_len + 41 > total:
            break
        keys[pos:pos + run_len] = key
        keys[pos - 1] = keys[pos + run_len] = b if key != b else c      # the run is exactly run_len long
        pred[pos:pos + run_len] = (C - 1, 0)[i & 1]
        runs.append((pos, run_len, int(key)))
        pos = (pos + run_len + 41 + CHUNK - 1) // CHUNK * CHUNK + 3
    return dict(coding=coding, keys=keys, pred=pred, runs=runs, run_len=run_len, pair=(int(a), int(b)), unknown=int(u))


# ---- recipe: layers8 --------------------------------------------------------------------------------------------------
N_SHARED = 24


def layers8():
    """One coding per layer of LAYERS8.  N_SHARED colours are in all eight, with a label that differs from layer to layer
    ((j + 5 l) mod 41 - 1: 5 l < 41 for l < 8); each layer adds 10 + l colours of its own."""
    shared = keys_with_hash(300, 8).tolist() + keys_with_hash(301, 8).tolist() + keys_with_hash(5, 8).tolist()
    shared = np.array(shared, np.int64)
    codings, own = [], []
    for l, C in enumerate(LAYERS8):
        mine = keys_with_hash(40 + l, 10 + l, skip=3)
        lab_shared = (np.arange(N_SHARED) + 5 * l) % 41 - 1
        lab_mine = (np.arange(len(mine)) * 3 + l) % (C + 3) - 2          # -2 .. C
        codings.append(entries(colors_of(np.concatenate([shared, mine])), np.concatenate([lab_shared, lab_mine])))
        own.append(mine)
    return dict(codings=codings, shared=shared, own=own, unknown=keys_with_hash(300, 3, skip=20))


def layers8_streams(rc, total, seed=0):
    """Colour keys per layer: the same bytes of shared colours at the same pixels of every layer, then the layer's own"""
    rng = np.random.default_rng(seed)
    common = np.repeat(np.concatenate([rc["shared"], rc["unknown"]]), rng.integers(1, 3, N_SHARED + 3))
    return [fit(np.concatenate([common, np.roll(rc["own"][l], -seed), rc["unknown"][:1]]), total) for l in range(MAX_LAYERS)]


def layers8_labels(total, seed=0):
    """(pred, gt) label streams per layer with values -2 .. C + 1, no runs to speak of"""
    rng = np.random.default_rng(100 + seed)
    pred = [rng.integers(-2, C + 2, total).astype(np.int8) for C in LAYERS8]
    gt = [rng.integers(-2, C + 2, total).astype(np.int8) for C in LAYERS8]
    return pred, gt


def table_labels_stream(coding, total, seed=0):
    """Labels that are in the coding, and whose colour decodes back to them (the label's last colour is not overwritten
    by a later entry of the same colour)"""
    dec, enc = decode_dict(coding), encode_table(coding)
    ok = [l for l in sorted(set(dec.values())) if dec.get(tuple(int(v) for v in enc[l & 255])) == l]
    rng = np.random.default_rng(seed)
    return np.array(ok, np.int8)[rng.integers(0, len(ok), total)]


# ---- recipe: bins -----------------------------------------------------------------------------------------------------
BIN_CLASSES = (1, 2, 63, 64)
RUN = 40


def extremes(C):
    return [-128, -1, 0, C - 1, C, 127]


def _no_repeats(pairs):
    """The pairs reordered so that no two neighbours are equal (greedy: a pair equal to its predecessor waits)"""
    out, waiting = [], []
    for p in pairs:
        cand = [p] + waiting
        waiting = []
        for q in cand:
            if out and out[-1] == q:
                waiting.append(q)
            else:
                out.append(q)
    other = [p for p in pairs if p not in waiting][:1] or [(-1, -1)]
    for q in waiting:                      # C = 1: the pair (0, 0) is most of the pool; part them with another pair
        out += [other[0], q] if out[-1] == q else [q]
    return out


def bins(C):
    """(pred, gt) int8 streams of one layer of C classes: a plane with a new pair every pixel that holds every one of the
    C * C pairs twice and the 36 pairs of `extremes`, then a run plane A x 40, skip, A x 40, out of range, A x 40, B ...
    Returns the streams and where the planes lie."""
    full = [(p, g) for g in range(C) for p in range(C)]
    n = len(full)
    step1 = next(s for s in range(n // 2 + 1, 2 * n + 2) if np.gcd(s, n) == 1)
    step2 = next(s for s in range(n // 3 + 1, 2 * n + 2) if np.gcd(s, n) == 1 and s != step1)
    ext = [(p, g) for p in extremes(C) for g in extremes(C)]
    pool = [full[(i * step1) % n] for i in range(n)] + ext[:18] + [full[(7 + i * step2) % n] for i in range(n)] + ext[18:]
    norun = _no_repeats(pool)
    skips = [(-1, 0), (0, -1), (-128, -128), (-1, 127), (127, -128), (-1, C)]
    oors = [(C, 0), (0, C), (127, 127), (C, C - 1), (C - 1, 127), (127, 0)]
    runs, marks = [], []
    for i in range(6):
        A = full[(i * 5) % n]
        B = full[(i * 5 + n // 2 + 1) % n]
        start = len(norun) + len(runs)
        runs += [A] * RUN + [skips[i]] + [A] * RUN + [oors[i]] + [A] * RUN + [B]
        marks.append((start, A, skips[i], oors[i], B))
    both = np.array(norun + runs, np.int64)
    assert both.min() >= -128 and both.max() <= 127
    return dict(pred=both[:, 0].astype(np.int8), gt=both[:, 1].astype(np.int8), n_norun=len(norun), marks=marks)


def bins_cases():
    """(C, W, H, n): every size and frame count that holds the whole stream of C"""
    out = []
    for C in BIN_CLASSES:
        need = len(bins(C)["pred"])
        for W, H in SIZES:
            for n in FRAME_COUNTS:
                if n * W * H >= need:
                    out.append((C, W, H, n))
    return out


# ---- recipe: rgb_gt ---------------------------------------------------------------------------------------------------
def rgb_gt(C):
    """The ground truth of bins(C) as colours.  Labels v with v mod 5 = 3, and 127, are left out of the table: they
    encode to black, which is not in the table either, and so score as `missing_label` (-1: unscored, 0: class 0,
    C: out of range)."""
    b = bins(C)
    values = sorted(set(b["gt"].tolist()))
    left_out = [v for v in values if v % 5 == 3 or v == 127]
    kept = [v for v in values if v not in left_out]
    coding = entries([[v & 255, (v * 7 + 3) & 255, 77] for v in kept], kept)
    return dict(pred=b["pred"], gt=b["gt"], gt_rgb=ref_encode(b["gt"], coding), coding=coding, left_out=left_out,
                missing=(-1, 0, C))


# ---- grid stride ------------------------------------------------------------------------------------------------------
def launch_blocks(cus, layers, c_max=None):
    """gridDim.x of eval_launch before the cap by the chunk count: the conversions (c_max None) and the confusion"""
    per_cu = 8 if c_max is None or c_max * c_max <= 256 else (4 if c_max * c_max <= 1024 else 2)
    return max(1, per_cu * cus // layers)


def grid_stride_frames(cus):
    """The fewest 640 x 480 frames of the 8-layer model with which a lane gets a second chunk"""
    chunks = GRID_W * GRID_H // CHUNK
    return THREADS * launch_blocks(cus, MAX_LAYERS, max(LAYERS8)) // chunks + 1


def grid_stride_case(cus):
    """Per layer of LAYERS8 an `alternating` stream over n VGA frames whose runs are as long as a lane's step from one
    of its chunks to the next, plus 7"""
    n = grid_stride_frames(cus)
    total = n * GRID_W * GRID_H
    stride = launch_blocks(cus, MAX_LAYERS, max(LAYERS8)) * BLOCK_PIXELS
    return n, [alternating(total, C, stride, seed=l) for l, C in enumerate(LAYERS8)]
