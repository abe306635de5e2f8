// Scoring on the device: colour-coded label images (RgbLabelConversion, include/rgb_label_conversion.h) and the
// confusion matrix of src/test.cpp:186-195 / src/test_multi.cpp:222-233, plus the C-ABI entry points that drive them
// and the host-only score formulas of test.cpp:203-228.  See include/rvseg.h and DESIGN.md "Scoring".
//
// Three streaming kernels, each over (layer) x (16-pixel chunks of every frame's plane of that layer):
//   labels_from_rgb       48 B in, 16 B out per chunk: the layer's colour table as an open-addressed hash in LDS
//   labels_to_rgb         16 B in, 48 B out per chunk: 256-entry LDS table indexed by (uint8)label
//   confusion_accumulate  16 B of predictions + 16 B (int8) or 48 B (RGB8) of ground truth per chunk, into a
//                         uint32 LDS histogram [C][C] per block; per-lane run-length cache in registers, so a frame of
//                         one class does not put 64 lanes on one LDS address; one 64-bit device atomic per non-zero
//                         bin and block at the end.  Integer counts: exact and independent of order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "rvseg_internal.h"

namespace rvseg {

namespace {

constexpr int kHashSlots = 512;                 // >= 2 x the 256 entries a layer may hold: load factor <= 1/2
constexpr int kMaxCodingEntries = 256;
constexpr int kMaxEvalClasses = 64;             // C <= 64: [C][C] uint32 = 16 KB of LDS
constexpr uint32_t kEmptySlot = 0xffffffffu;    // colours are 24-bit keys, so this never matches one
constexpr int kThreads = 256;
constexpr int kChunk = 16;                      // pixels per lane-step

// One layer's colour coding as the kernels read it (copied into LDS at block start).
struct EvalTable {
    uint32_t key[kHashSlots];    // r << 16 | g << 8 | b, or kEmptySlot
    int32_t missing;             // label of a colour that is not in the table (0 = the reference's std::map default)
    int8_t label[kHashSlots];
    uint32_t enc[256];           // (uint8)label -> r | g << 8 | b << 16; (0, 0, 0) for labels not in the table
};
static_assert(sizeof(EvalTable) % 4 == 0, "EvalTable is copied in 32-bit words");
constexpr int kTableWords = (int)(sizeof(EvalTable) / 4);

__host__ __device__ inline uint32_t color_hash(uint32_t key) { return (key * 2654435761u) >> 23; }   // top 9 bits

__device__ inline int8_t decode_color(const EvalTable& t, uint32_t key) {
    uint32_t h = color_hash(key);
    for (int i = 0; i < kHashSlots; i++) {       // the host keeps at least half the slots empty: a miss ends early
        const uint32_t s = t.key[h];
        if (s == key) return t.label[h];
        if (s == kEmptySlot) break;
        h = (h + 1) & (kHashSlots - 1);
    }
    return (int8_t)t.missing;
}

__device__ inline void load_table(EvalTable& dst, const EvalTable* src) {
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d = reinterpret_cast<uint32_t*>(&dst);
    for (int i = threadIdx.x; i < kTableWords; i += blockDim.x) d[i] = s[i];
}

// Where chunk c of this block's layer lives.  Planes are frame-major: plane = frame * planes_per_frame + plane_of_layer.
struct ChunkPos {
    size_t pix;   // first pixel (index into the whole n x planes_per_frame x P buffer)
    int cnt;      // pixels in the chunk (16, or the plane's tail)
};

__device__ inline ChunkPos chunk_pos(uint64_t c, uint32_t chunks_per_plane, uint32_t P, int planes_per_frame, int plane_of_layer) {
    const uint64_t f = c / chunks_per_plane;
    const uint32_t k = (uint32_t)(c - f * chunks_per_plane);
    const size_t plane = (size_t)f * planes_per_frame + plane_of_layer;
    ChunkPos r;
    r.pix = plane * P + (size_t)k * kChunk;
    r.cnt = (int)min((uint32_t)kChunk, P - k * kChunk);
    return r;
}

__device__ inline uint32_t byte_of(const uint32_t* w, int b) { return (w[b >> 2] >> ((b & 3) * 8)) & 255u; }

// ---- labels_from_rgb ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void labels_from_rgb_kernel(const uint8_t* __restrict__ rgb, int8_t* __restrict__ out,
                                                                  const EvalTable* __restrict__ tables, int layer_fixed,
                                                                  int planes_per_frame, uint32_t P, uint32_t chunks_per_plane,
                                                                  uint64_t n_chunks, int vec_ok) {
    __shared__ EvalTable tab;
    const int layer = layer_fixed >= 0 ? layer_fixed : (int)blockIdx.y;
    const int plane_of_layer = layer_fixed >= 0 ? 0 : (int)blockIdx.y;
    load_table(tab, tables + layer);
    __syncthreads();
    uint32_t last_key = kEmptySlot;
    int8_t last_label = 0;
    auto decode = [&](uint32_t key) -> int8_t {   // neighbouring pixels mostly share a colour: skip the LDS probe
        if (key != last_key) { last_key = key; last_label = decode_color(tab, key); }
        return last_label;
    };
    for (uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * kThreads) {
        const ChunkPos q = chunk_pos(c, chunks_per_plane, P, planes_per_frame, plane_of_layer);
        if (vec_ok && q.cnt == kChunk && (q.pix & 15) == 0) {
            const uint4* src = reinterpret_cast<const uint4*>(rgb + q.pix * 3);
            uint32_t w[12];
            const uint4 a = src[0], b = src[1], d = src[2];
            w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
            w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            w[8] = d.x; w[9] = d.y; w[10] = d.z; w[11] = d.w;
            uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < kChunk; j++) {
                const uint32_t key = byte_of(w, 3 * j) << 16 | byte_of(w, 3 * j + 1) << 8 | byte_of(w, 3 * j + 2);
                o[j >> 2] |= ((uint32_t)(uint8_t)decode(key)) << ((j & 3) * 8);
            }
            *reinterpret_cast<uint4*>(out + q.pix) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            for (int j = 0; j < q.cnt; j++) {
                const uint8_t* px = rgb + (q.pix + j) * 3;
                out[q.pix + j] = decode((uint32_t)px[0] << 16 | (uint32_t)px[1] << 8 | px[2]);
            }
        }
    }
}

// ---- labels_to_rgb ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void labels_to_rgb_kernel(const int8_t* __restrict__ labels, uint8_t* __restrict__ rgb,
                                                                const EvalTable* __restrict__ tables, int layer_fixed,
                                                                int planes_per_frame, uint32_t P, uint32_t chunks_per_plane,
                                                                uint64_t n_chunks, int vec_ok) {
    __shared__ uint32_t enc[256];
    const int layer = layer_fixed >= 0 ? layer_fixed : (int)blockIdx.y;
    const int plane_of_layer = layer_fixed >= 0 ? 0 : (int)blockIdx.y;
    for (int i = threadIdx.x; i < 256; i += blockDim.x) enc[i] = tables[layer].enc[i];
    __syncthreads();
    for (uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * kThreads) {
        const ChunkPos q = chunk_pos(c, chunks_per_plane, P, planes_per_frame, plane_of_layer);
        if (vec_ok && q.cnt == kChunk && (q.pix & 15) == 0) {
            const uint4 v = *reinterpret_cast<const uint4*>(labels + q.pix);
            const uint32_t in[4] = {v.x, v.y, v.z, v.w};
            uint32_t w[12] = {};
#pragma unroll
            for (int j = 0; j < kChunk; j++) {
                const uint32_t col = enc[(in[j >> 2] >> ((j & 3) * 8)) & 255u];
#pragma unroll
                for (int ch = 0; ch < 3; ch++) {
                    const int b = 3 * j + ch;
                    w[b >> 2] |= ((col >> (8 * ch)) & 255u) << ((b & 3) * 8);
                }
            }
            uint4* dst = reinterpret_cast<uint4*>(rgb + q.pix * 3);
            dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
            dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
            dst[2] = make_uint4(w[8], w[9], w[10], w[11]);
        } else {
            for (int j = 0; j < q.cnt; j++) {
                const uint32_t col = enc[(uint8_t)labels[q.pix + j]];
                uint8_t* px = rgb + (q.pix + j) * 3;
                px[0] = (uint8_t)col; px[1] = (uint8_t)(col >> 8); px[2] = (uint8_t)(col >> 16);
            }
        }
    }
}

struct LayerClasses { int c[RVSEG_MAX_LAYERS]; };   // C of every layer, passed by value

// ---- confusion_accumulate -----------------------------------------------------------------------------------------
// counts: [RVSEG_MAX_LAYERS][64 * 64] uint64 (row = ground truth, column = prediction), then [RVSEG_MAX_LAYERS] uint64
// out-of-range counters.  One block works on one layer (blockIdx.y) and a grid-stride share of its chunks.
template <bool kRgb>
__global__ __launch_bounds__(kThreads) void confusion_accumulate_kernel(const int8_t* __restrict__ pred, const void* __restrict__ gt,
                                                                       const EvalTable* __restrict__ tables, int L, LayerClasses cc, uint32_t P,
                                                                       uint32_t chunks_per_plane, uint64_t n_chunks,
                                                                       unsigned long long* __restrict__ counts, int vec_ok) {
    __shared__ uint32_t hist[kMaxEvalClasses * kMaxEvalClasses];
    __shared__ EvalTable tab;
    __shared__ uint32_t s_oor;
    const int layer = (int)blockIdx.y;
    const int C = cc.c[layer];
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) hist[i] = 0u;
    if (threadIdx.x == 0) s_oor = 0u;
    if (kRgb) load_table(tab, tables + layer);
    __syncthreads();

    uint32_t run_key = kEmptySlot, run_n = 0, oor = 0;
    uint32_t last_key = kEmptySlot;
    int8_t last_label = 0;
    auto count = [&](int p, int g) {
        if (p < 0 || g < 0) return;                             // test.cpp:187
        if (p >= C || g >= C) { oor++; return; }                // the reference indexes past its arrays here
        const uint32_t key = (uint32_t)(g * C + p);
        if (key == run_key) { run_n++; return; }
        if (run_n) atomicAdd(&hist[run_key], run_n);            // ds_add_u32, only when the pair changes
        run_key = key;
        run_n = 1;
    };
    auto gt_rgb = [&](uint32_t key) -> int {
        if (key != last_key) { last_key = key; last_label = decode_color(tab, key); }
        return last_label;
    };
    const uint8_t* g8 = static_cast<const uint8_t*>(gt);
    for (uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x; c < n_chunks; c += (uint64_t)gridDim.x * kThreads) {
        const ChunkPos q = chunk_pos(c, chunks_per_plane, P, L, layer);
        if (vec_ok && q.cnt == kChunk && (q.pix & 15) == 0) {
            const uint4 pv = *reinterpret_cast<const uint4*>(pred + q.pix);
            const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
            if (kRgb) {
                const uint4* src = reinterpret_cast<const uint4*>(g8 + q.pix * 3);
                const uint4 a = src[0], b = src[1], d = src[2];
                const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w};
#pragma unroll
                for (int j = 0; j < kChunk; j++) {
                    const uint32_t key = byte_of(w, 3 * j) << 16 | byte_of(w, 3 * j + 1) << 8 | byte_of(w, 3 * j + 2);
                    count((int)(int8_t)(pw[j >> 2] >> ((j & 3) * 8)), gt_rgb(key));
                }
            } else {
                const uint4 gv = *reinterpret_cast<const uint4*>(g8 + q.pix);
                const uint32_t gw[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
                for (int j = 0; j < kChunk; j++)
                    count((int)(int8_t)(pw[j >> 2] >> ((j & 3) * 8)), (int)(int8_t)(gw[j >> 2] >> ((j & 3) * 8)));
            }
        } else {
            for (int j = 0; j < q.cnt; j++) {
                const size_t i = q.pix + j;
                int g;
                if (kRgb) g = gt_rgb((uint32_t)g8[3 * i] << 16 | (uint32_t)g8[3 * i + 1] << 8 | g8[3 * i + 2]);
                else g = (int)(int8_t)g8[i];
                count((int)pred[i], g);
            }
        }
    }
    if (run_n) atomicAdd(&hist[run_key], run_n);
    if (oor) atomicAdd(&s_oor, oor);
    __syncthreads();
    unsigned long long* lc = counts + (size_t)layer * kMaxEvalClasses * kMaxEvalClasses;
    for (int i = threadIdx.x; i < C * C; i += blockDim.x) {
        const uint32_t v = hist[i];
        if (v) atomicAdd(lc + i, (unsigned long long)v);
    }
    if (threadIdx.x == 0 && s_oor)
        atomicAdd(counts + (size_t)RVSEG_MAX_LAYERS * kMaxEvalClasses * kMaxEvalClasses + layer, (unsigned long long)s_oor);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
// context state (allocated on first use, freed by rvseg_destroy, discarded by rvseg_forest_load)
// ---------------------------------------------------------------------------------------------------------------------
struct EvalState {
    bool has_coding[RVSEG_MAX_LAYERS] = {};
    EvalTable host_tables[RVSEG_MAX_LAYERS];
    DevBuf tables;     // EvalTable[RVSEG_MAX_LAYERS]
    DevBuf counts;     // uint64: [RVSEG_MAX_LAYERS][64 * 64], then [RVSEG_MAX_LAYERS] out of range
    DevBuf stage_a, stage_b;   // host entry points
    std::vector<std::pair<hipStream_t, Event>> pending;   // last event recorded per caller stream
};

constexpr size_t kCountWords = (size_t)RVSEG_MAX_LAYERS * kMaxEvalClasses * kMaxEvalClasses + RVSEG_MAX_LAYERS;

void eval_destroy(rvseg_ctx* ctx) {
    EvalState* e = ctx->eval;
    if (!e) return;
    for (auto& pe : e->pending) (void)hipEventSynchronize(pe.second);   // before the events and the tables go
    delete e;
    ctx->eval = nullptr;
}

namespace {

rvseg_status eval_state(rvseg_ctx* ctx, EvalState** out) {
    if (!ctx->forest_loaded) {
        ctx->err = "no forest loaded: the label layers and class counts of the scoring calls come from the model";
        return RVSEG_ERR_INVALID_ARG;
    }
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    if (!ctx->eval) {
        // tables and zeroed counters first: a failure leaves nothing behind and the next call tries again
        DevBuf tables, counts;
        rvseg_status st;
        if ((st = dev_alloc(ctx, tables, sizeof(EvalTable) * RVSEG_MAX_LAYERS)) != RVSEG_OK) return st;
        if ((st = dev_alloc(ctx, counts, kCountWords * sizeof(uint64_t))) != RVSEG_OK) return st;
        RV_HIP(ctx, hipMemset(counts.p, 0, kCountWords * sizeof(uint64_t)));
        ctx->eval = new EvalState();
        ctx->eval->tables = std::move(tables);
        ctx->eval->counts = std::move(counts);
    }
    *out = ctx->eval;
    return RVSEG_OK;
}

rvseg_status wait_pending(rvseg_ctx* ctx, EvalState* e) {
    for (auto& pe : e->pending) RV_HIP(ctx, hipEventSynchronize(pe.second));
    return RVSEG_OK;
}

rvseg_status record_pending(rvseg_ctx* ctx, EvalState* e, hipStream_t s) {
    for (auto& pe : e->pending)
        if (pe.first == s) { RV_HIP(ctx, hipEventRecord(pe.second, s)); return RVSEG_OK; }
    Event ev;
    RV_HIP(ctx, event_create(ev, hipEventDisableTiming));
    e->pending.emplace_back(s, std::move(ev));
    RV_HIP(ctx, hipEventRecord(e->pending.back().second, s));
    return RVSEG_OK;
}

int cu_count(int device) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || n <= 0) n = 256;
    return n;
}

// Shape of one launch over n frames: every layer (layer < 0, planes n x L, grid.y = L) or one (n planes, grid.y = 1).
struct EvalLaunch {
    int planes_per_frame, layers, layer_fixed;
    uint32_t P, chunks_per_plane;
    uint64_t n_chunks;   // per grid row
    dim3 grid;
};

EvalLaunch eval_launch(const rvseg_ctx* ctx, int layer, int n_frames, int blocks_per_cu) {
    EvalLaunch g;
    const int L = ctx->forest.n_layers;
    g.layers = layer < 0 ? L : 1;
    g.planes_per_frame = layer < 0 ? L : 1;
    g.layer_fixed = layer;
    g.P = (uint32_t)ctx->params.width * (uint32_t)ctx->params.height;
    g.chunks_per_plane = (g.P + kChunk - 1) / kChunk;
    g.n_chunks = (uint64_t)n_frames * g.chunks_per_plane;
    // a few blocks per CU over all grid rows (bounded flushes), at least enough that no block's share of pixels
    // reaches 2^31: the LDS bins and the per-lane run counters are uint32
    uint64_t bx = std::max<uint64_t>(1, (uint64_t)(blocks_per_cu * cu_count(ctx->params.device)) / (uint64_t)g.layers);
    bx = std::min<uint64_t>(bx, (g.n_chunks + kThreads - 1) / kThreads);
    const uint64_t max_chunks_per_block = (1ull << 31) / kChunk;
    bx = std::max<uint64_t>(bx, (g.n_chunks + max_chunks_per_block - 1) / max_chunks_per_block);
    g.grid = dim3((unsigned)std::max<uint64_t>(bx, 1), (unsigned)g.layers);
    return g;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

rvseg_status check_layer_coding(rvseg_ctx* ctx, EvalState* e, int layer) {
    const int L = ctx->forest.n_layers;
    if (layer >= L) { ctx->err = "layer " + std::to_string(layer) + " out of range (the model has " + std::to_string(L) + ")"; return RVSEG_ERR_INVALID_ARG; }
    for (int l = layer < 0 ? 0 : layer; l < (layer < 0 ? L : layer + 1); l++)
        if (!e->has_coding[l]) { ctx->err = "no colour coding set for layer " + std::to_string(l) + " (rvseg_color_coding_set)"; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

rvseg_status convert_device(rvseg_ctx* ctx, bool to_rgb, int32_t layer, int32_t n, const void* d_in, void* d_out, hipStream_t s) {
    EvalState* e;
    rvseg_status st;
    if ((st = eval_state(ctx, &e)) != RVSEG_OK) return st;
    if (n < 0 || (n > 0 && (!d_in || !d_out))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if ((st = check_layer_coding(ctx, e, layer)) != RVSEG_OK) return st;
    if (n == 0) return RVSEG_OK;
    const EvalLaunch g = eval_launch(ctx, layer, n, 8);
    const int vec_ok = aligned16(d_in) && aligned16(d_out);
    if (to_rgb)
        labels_to_rgb_kernel<<<g.grid, kThreads, 0, s>>>(static_cast<const int8_t*>(d_in), static_cast<uint8_t*>(d_out), e->tables.as<EvalTable>(),
                                                         g.layer_fixed, g.planes_per_frame, g.P, g.chunks_per_plane, g.n_chunks, vec_ok);
    else
        labels_from_rgb_kernel<<<g.grid, kThreads, 0, s>>>(static_cast<const uint8_t*>(d_in), static_cast<int8_t*>(d_out), e->tables.as<EvalTable>(),
                                                           g.layer_fixed, g.planes_per_frame, g.P, g.chunks_per_plane, g.n_chunks, vec_ok);
    RV_LAUNCHED(to_rgb ? "labels_to_rgb" : "labels_from_rgb");
    RV_LAUNCH_OK(ctx);
    return record_pending(ctx, e, s);
}

rvseg_status accumulate_device(rvseg_ctx* ctx, int32_t n, const int8_t* d_pred, const void* d_gt, int32_t gt_format, hipStream_t s) {
    EvalState* e;
    rvseg_status st;
    if ((st = eval_state(ctx, &e)) != RVSEG_OK) return st;
    if (n < 0 || (n > 0 && (!d_pred || !d_gt))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (gt_format != RVSEG_GT_LABELS && gt_format != RVSEG_GT_RGB) { ctx->err = "gt_format must be RVSEG_GT_LABELS or RVSEG_GT_RGB"; return RVSEG_ERR_INVALID_ARG; }
    const int L = ctx->forest.n_layers;
    LayerClasses cc{};
    for (int l = 0; l < L; l++) {
        cc.c[l] = ctx->forest.class_counts[l];
        if (cc.c[l] > kMaxEvalClasses) { ctx->err = "more than 64 classes in a layer"; return RVSEG_ERR_CAPACITY; }
    }
    if (gt_format == RVSEG_GT_RGB && (st = check_layer_coding(ctx, e, -1)) != RVSEG_OK) return st;
    if (n == 0) return RVSEG_OK;
    // blocks per CU: 8 keep every SIMD busy (two waves each); each block ends with one device atomic per non-zero bin,
    // so large class counts get fewer blocks
    int c_max = 1;
    for (int l = 0; l < L; l++) c_max = std::max(c_max, cc.c[l]);
    const EvalLaunch g = eval_launch(ctx, -1, n, c_max * c_max <= 256 ? 8 : (c_max * c_max <= 1024 ? 4 : 2));
    // no block's share of a layer may reach 2^32 pixels (uint32 LDS bins and run counters); eval_launch keeps it below 2^31
    const uint64_t per_block = (g.n_chunks + (uint64_t)g.grid.x * kThreads - 1) / ((uint64_t)g.grid.x * kThreads) * kThreads * kChunk;
    if (per_block >= (1ull << 32)) { ctx->err = "internal: confusion block share exceeds 2^32 pixels"; return RVSEG_ERR_CAPACITY; }
    const int vec_ok = aligned16(d_pred) && aligned16(d_gt);
    unsigned long long* counts = e->counts.as<unsigned long long>();
    if (gt_format == RVSEG_GT_RGB)
        confusion_accumulate_kernel<true><<<g.grid, kThreads, 0, s>>>(d_pred, d_gt, e->tables.as<EvalTable>(), L, cc, g.P, g.chunks_per_plane, g.n_chunks, counts, vec_ok);
    else
        confusion_accumulate_kernel<false><<<g.grid, kThreads, 0, s>>>(d_pred, d_gt, e->tables.as<EvalTable>(), L, cc, g.P, g.chunks_per_plane, g.n_chunks, counts, vec_ok);
    RV_LAUNCHED("confusion_accumulate");
    RV_LAUNCH_OK(ctx);
    return record_pending(ctx, e, s);
}

}  // namespace
}  // namespace rvseg

using namespace rvseg;

// NULL = the context's own stream, as for every other _device entry point

extern "C" {

rvseg_status rvseg_color_coding_set(rvseg_ctx* ctx, int32_t layer, int32_t n, const uint8_t* rgb, const int8_t* labels,
                                    int8_t missing_label) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    EvalState* e;
    rvseg_status st;
    if ((st = eval_state(ctx, &e)) != RVSEG_OK) return st;
    if (layer < 0 || layer >= ctx->forest.n_layers) { ctx->err = "layer out of range of the loaded model"; return RVSEG_ERR_INVALID_ARG; }
    if (n < 0 || (n > 0 && (!rgb || !labels))) { ctx->err = "bad colour coding"; return RVSEG_ERR_INVALID_ARG; }
    if (n > kMaxCodingEntries) { ctx->err = "more than 256 colour coding entries in one layer"; return RVSEG_ERR_CAPACITY; }
    // the reference's std::map assignments in entry order (rgb_label_conversion.h:29-38): the later entry wins, for a
    // repeated colour (decode) as for a repeated label (encode)
    EvalTable t;
    for (int i = 0; i < kHashSlots; i++) { t.key[i] = kEmptySlot; t.label[i] = 0; }
    for (int i = 0; i < 256; i++) t.enc[i] = 0u;
    t.missing = missing_label;
    for (int i = 0; i < n; i++) {
        const uint32_t key = (uint32_t)rgb[3 * i] << 16 | (uint32_t)rgb[3 * i + 1] << 8 | rgb[3 * i + 2];
        uint32_t h = color_hash(key);
        while (t.key[h] != kEmptySlot && t.key[h] != key) h = (h + 1) & (kHashSlots - 1);
        t.key[h] = key;
        t.label[h] = labels[i];
        t.enc[(uint8_t)labels[i]] = (uint32_t)rgb[3 * i] | (uint32_t)rgb[3 * i + 1] << 8 | (uint32_t)rgb[3 * i + 2] << 16;
    }
    if ((st = wait_pending(ctx, e)) != RVSEG_OK) return st;   // earlier work may still read the old table
    RV_HIP(ctx, hipMemcpy(e->tables.as<EvalTable>() + layer, &t, sizeof(t), hipMemcpyHostToDevice));
    e->host_tables[layer] = t;
    e->has_coding[layer] = true;
    return RVSEG_OK;
}

rvseg_status rvseg_labels_from_rgb_device(rvseg_ctx* ctx, int32_t layer, int32_t n_images, const uint8_t* d_rgb, int8_t* d_labels,
                                          void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    return convert_device(ctx, false, layer, n_images, d_rgb, d_labels, stream_of(ctx, hip_stream));
}

rvseg_status rvseg_labels_to_rgb_device(rvseg_ctx* ctx, int32_t layer, int32_t n_images, const int8_t* d_labels, uint8_t* d_rgb,
                                        void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    return convert_device(ctx, true, layer, n_images, d_labels, d_rgb, stream_of(ctx, hip_stream));
}

// host variants: staged through the context's stream, max_batch images per round trip
static rvseg_status convert_host(rvseg_ctx* ctx, bool to_rgb, int32_t layer, int32_t n, const void* in, void* out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    EvalState* e;
    rvseg_status st;
    if ((st = eval_state(ctx, &e)) != RVSEG_OK) return st;
    if (n < 0 || (n > 0 && (!in || !out))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if ((st = check_layer_coding(ctx, e, layer)) != RVSEG_OK) return st;
    const size_t planes = layer < 0 ? (size_t)ctx->forest.n_layers : 1;
    const size_t px = (size_t)ctx->params.width * ctx->params.height * planes;   // pixels per image
    const int chunk = std::max(1, ctx->params.max_batch);
    if ((st = dev_reserve(ctx, e->stage_a, px * 3 * chunk)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, e->stage_b, px * 3 * chunk)) != RVSEG_OK) return st;
    const size_t in_b = to_rgb ? 1 : 3, out_b = to_rgb ? 3 : 1;
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int m = std::min(chunk, n - i0);
        RV_HIP(ctx, hipMemcpyAsync(e->stage_a.p, static_cast<const uint8_t*>(in) + i0 * px * in_b, m * px * in_b, hipMemcpyHostToDevice, ctx->stream));
        if ((st = convert_device(ctx, to_rgb, layer, m, e->stage_a.p, e->stage_b.p, ctx->stream)) != RVSEG_OK) return st;
        RV_HIP(ctx, hipMemcpyAsync(static_cast<uint8_t*>(out) + i0 * px * out_b, e->stage_b.p, m * px * out_b, hipMemcpyDeviceToHost, ctx->stream));
        RV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RVSEG_OK;
}

rvseg_status rvseg_labels_from_rgb(rvseg_ctx* ctx, int32_t layer, int32_t n_images, const uint8_t* rgb, int8_t* labels) {
    return convert_host(ctx, false, layer, n_images, rgb, labels);
}

rvseg_status rvseg_labels_to_rgb(rvseg_ctx* ctx, int32_t layer, int32_t n_images, const int8_t* labels, uint8_t* rgb) {
    return convert_host(ctx, true, layer, n_images, labels, rgb);
}

rvseg_status rvseg_eval_reset(rvseg_ctx* ctx) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    EvalState* e;
    rvseg_status st;
    if ((st = eval_state(ctx, &e)) != RVSEG_OK) return st;
    if ((st = wait_pending(ctx, e)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemsetAsync(e->counts.p, 0, kCountWords * sizeof(uint64_t), ctx->stream));
    RV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RVSEG_OK;
}

rvseg_status rvseg_eval_accumulate_device(rvseg_ctx* ctx, int32_t n_frames, const int8_t* d_pred, const void* d_gt, int32_t gt_format,
                                          void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    return accumulate_device(ctx, n_frames, d_pred, d_gt, gt_format, stream_of(ctx, hip_stream));
}

rvseg_status rvseg_eval_accumulate(rvseg_ctx* ctx, int32_t n_frames, const int8_t* pred, const void* gt, int32_t gt_format) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    EvalState* e;
    rvseg_status st;
    if ((st = eval_state(ctx, &e)) != RVSEG_OK) return st;
    if (n_frames < 0 || (n_frames > 0 && (!pred || !gt))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (gt_format != RVSEG_GT_LABELS && gt_format != RVSEG_GT_RGB) { ctx->err = "gt_format must be RVSEG_GT_LABELS or RVSEG_GT_RGB"; return RVSEG_ERR_INVALID_ARG; }
    const size_t px = (size_t)ctx->params.width * ctx->params.height * ctx->forest.n_layers;   // label pixels per frame
    const size_t gt_b = gt_format == RVSEG_GT_RGB ? 3 : 1;
    const int chunk = std::max(1, ctx->params.max_batch);
    if ((st = dev_reserve(ctx, e->stage_a, px * chunk)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, e->stage_b, px * 3 * chunk)) != RVSEG_OK) return st;
    for (int i0 = 0; i0 < n_frames; i0 += chunk) {
        const int m = std::min(chunk, n_frames - i0);
        RV_HIP(ctx, hipMemcpyAsync(e->stage_a.p, pred + i0 * px, m * px, hipMemcpyHostToDevice, ctx->stream));
        RV_HIP(ctx, hipMemcpyAsync(e->stage_b.p, static_cast<const uint8_t*>(gt) + i0 * px * gt_b, m * px * gt_b, hipMemcpyHostToDevice, ctx->stream));
        if ((st = accumulate_device(ctx, m, e->stage_a.as<int8_t>(), e->stage_b.p, gt_format, ctx->stream)) != RVSEG_OK) return st;
        RV_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the staging buffers are reused by the next round
    }
    return RVSEG_OK;
}

rvseg_status rvseg_eval_confusion(rvseg_ctx* ctx, int32_t layer, uint64_t* counts_out, uint64_t* out_of_range) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    EvalState* e;
    rvseg_status st;
    if ((st = eval_state(ctx, &e)) != RVSEG_OK) return st;
    if (layer < 0 || layer >= ctx->forest.n_layers) { ctx->err = "layer out of range of the loaded model"; return RVSEG_ERR_INVALID_ARG; }
    if ((st = wait_pending(ctx, e)) != RVSEG_OK) return st;   // every _device accumulate enqueued so far
    const int C = ctx->forest.class_counts[layer];
    std::vector<uint64_t> all(kCountWords);
    RV_HIP(ctx, hipMemcpyAsync(all.data(), e->counts.p, kCountWords * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    RV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t* lc = all.data() + (size_t)layer * kMaxEvalClasses * kMaxEvalClasses;
    if (counts_out) std::memcpy(counts_out, lc, sizeof(uint64_t) * C * C);
    if (out_of_range) *out_of_range = all[(size_t)RVSEG_MAX_LAYERS * kMaxEvalClasses * kMaxEvalClasses + layer];
    return RVSEG_OK;
}

// test.cpp:203-228, with the reference's types and order of operations: float accumulators fed double expressions,
// `static_cast<float>` of each count, int divisors (here exact uint64) converted to double.
rvseg_status rvseg_eval_scores_from_counts(const uint64_t* counts, int32_t C, double* global_acc, float* class_avg_acc, float* iou,
                                           double* row_pct_out) {
    if (!counts || C < 1) return RVSEG_ERR_INVALID_ARG;
    std::vector<uint64_t> class_count(C, 0), vote_count(C, 0);
    uint64_t total = 0;
    for (int i = 0; i < C; i++)
        for (int j = 0; j < C; j++) {
            const uint64_t v = counts[(size_t)i * C + j];
            class_count[i] += v;
            vote_count[j] += v;
            total += v;
        }
    uint64_t total_acc = 0;
    float avg_acc = 0, iou_acc = 0;
    for (int i = 0; i < C; i++) {
        const double cls = (double)(class_count[i] ? class_count[i] : 1);
        for (int j = 0; j < C; j++) {
            const uint64_t v = counts[(size_t)i * C + j];
            if (i == j) {
                total_acc += v;
                avg_acc += 100.0 * static_cast<float>(v) / cls;
                const uint64_t x = class_count[i] + vote_count[i] - v;
                iou_acc += 100.0 * static_cast<float>(v) / (double)(x ? x : 1);
            }
            if (row_pct_out) row_pct_out[(size_t)i * C + j] = 100.0 * static_cast<float>(v) / cls;
        }
    }
    if (global_acc) *global_acc = 100.0 * static_cast<float>(total_acc) / (double)total;   // NaN for total == 0, as in the reference
    if (class_avg_acc) *class_avg_acc = avg_acc / C;
    if (iou) *iou = iou_acc / C;
    return RVSEG_OK;
}

}  // extern "C"
