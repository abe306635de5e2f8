// The projector of the local-map half (src/segmenter.cpp:234-240, 576-578 of the reference):
//     _projector.project(zbuffer, index_image, m_multi->transform().inverse(), *cloud)
// fps_mapper::MultiProjector is not in the reference tree, so the projection is this build's own definition, written
// down in include/rvseg.h (and DESIGN.md section 13).  Per pixel the winner is the kept point with the smallest w and,
// among equal w, the smallest index: what the sequential "if (z < zbuffer) { zbuffer = z; index = i; }" loop over
// ascending i leaves behind.  On the device that rule is ONE unsigned 64-bit minimum: w is positive (w >= depth_min > 0),
// so its bit pattern orders like its value, and the key (bits(w) << 32) | i orders by w first and by index second.
// Every kept (point, image) issues one atomic min on the pixel's key; the order of arrival cannot change a minimum.
#include <cmath>
#include <cstring>

#include "rvseg_internal.h"
#include "rvseg_pipeline.h"

namespace rvseg {

constexpr int PROJECT_GROUP = 32;                    // images per launch group: bounds the key image
constexpr unsigned long long PROJECT_NO_KEY = ~0ull; // the cleared key: above every real one (bits(w) <= 0x7f800000)

// the matrices of one launch group: a kernel argument, so every read is a uniform (scalar) load
struct ProjectGroup {
    float P[PROJECT_GROUP][12];
    int n;
};

// one thread per point; walks the images of the group
__global__ void __launch_bounds__(256)
project_points_kernel(ProjectGroup g, const float* __restrict__ xyz, int N, int W, int H, float depth_min, float depth_max,
                      unsigned pixels, unsigned long long* __restrict__ keys) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (unsigned)N) return;
    const float x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
    const float fW = (float)W, fH = (float)H;
    for (int m = 0; m < g.n; m++) {
        const float* P = g.P[m];
        const float w = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
        if (!(w >= depth_min && w <= depth_max)) continue;   // NaN fails both
        const float px = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
        const float py = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
        const float cu = rintf(px / w), cv = rintf(py / w);
        if (!(cu >= 0.0f && cu < fW && cv >= 0.0f && cv < fH)) continue;   // on the floats: huge or NaN never converts
        const unsigned pix = (unsigned)(int)cv * (unsigned)W + (unsigned)(int)cu;
        const unsigned long long key = ((unsigned long long)__float_as_uint(w) << 32) | i;
        (void)__hip_atomic_fetch_min(keys + (size_t)m * pixels + pix, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// key -> index (low word, or -1 for the cleared key) and the optional z-buffer (high word, or +inf)
__global__ void __launch_bounds__(256)
project_resolve_kernel(const unsigned long long* __restrict__ keys, unsigned n, int32_t* __restrict__ index, float* __restrict__ zbuffer) {
    const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    const unsigned long long key = keys[e];
    const bool none = key == PROJECT_NO_KEY;
    index[e] = none ? -1 : (int32_t)(unsigned)key;
    if (zbuffer) zbuffer[e] = none ? __uint_as_float(0x7f800000u) : __uint_as_float((unsigned)(key >> 32));
}

static void launch_project_group(const ProjectGroup& g, const float* d_xyz, int N, const rvseg_params& p, unsigned pixels,
                                 unsigned long long* keys, int32_t* d_index, float* d_zbuffer, hipStream_t s) {
    if (N > 0)
        project_points_kernel<<<dim3((unsigned)(((long long)N + 255) / 256)), dim3(256), 0, s>>>(g, d_xyz, N, p.width, p.height, p.depth_min,
                                                                                                 p.depth_max, pixels, keys);
    RV_LAUNCHED("project_points_kernel");
    const unsigned n = (unsigned)g.n * pixels;
    project_resolve_kernel<<<dim3((n + 255) / 256), dim3(256), 0, s>>>(keys, n, d_index, d_zbuffer);
    RV_LAUNCHED("project_resolve_kernel");
}

rvseg_status project_check(rvseg_ctx* ctx, int32_t n_images, const float* proj, int32_t N, const void* xyz, const void* index_out) {
    if (n_images < 0 || N < 0 || (n_images > 0 && (!proj || !index_out)) || (n_images > 0 && N > 0 && !xyz)) {
        ctx->err = "bad arguments";
        return RVSEG_ERR_INVALID_ARG;
    }
    if (!(ctx->params.depth_min > 0.0f)) { ctx->err = "the projector needs depth_min > 0"; return RVSEG_ERR_INVALID_ARG; }
    const unsigned long long hits = (unsigned long long)n_images * ((unsigned long long)ctx->params.width * ctx->params.height);
    if (hits >= 0xFFFFFFFFull) { ctx->err = "too many index-image pixels for one call"; return RVSEG_ERR_INVALID_ARG; }
    return RVSEG_OK;
}

rvseg_status project_enqueue(rvseg_ctx* ctx, FusionState* fs, int32_t n_images, const float* proj, int32_t N, const float* d_xyz,
                             int32_t* d_index, float* d_zbuffer, hipStream_t s) {
    const size_t pixels = (size_t)ctx->params.width * ctx->params.height;
    if (n_images == 0 || pixels == 0) return RVSEG_OK;
    const int widest = n_images < PROJECT_GROUP ? n_images : PROJECT_GROUP;
    rvseg_status st = dev_reserve(ctx, fs->proj_keys, (size_t)widest * pixels * sizeof(unsigned long long));
    if (st != RVSEG_OK) return st;
    for (int m0 = 0; m0 < n_images; m0 += PROJECT_GROUP) {
        ProjectGroup g{};
        g.n = n_images - m0 < PROJECT_GROUP ? n_images - m0 : PROJECT_GROUP;
        std::memcpy(g.P, proj + (size_t)m0 * 12, (size_t)g.n * 12 * sizeof(float));
        RV_HIP(ctx, hipMemsetAsync(fs->proj_keys.p, 0xFF, (size_t)g.n * pixels * sizeof(unsigned long long), s));
        launch_project_group(g, d_xyz, N, ctx->params, (unsigned)pixels, fs->proj_keys.as<unsigned long long>(), d_index + (size_t)m0 * pixels,
                             d_zbuffer ? d_zbuffer + (size_t)m0 * pixels : nullptr, s);
        RV_LAUNCH_OK(ctx);
    }
    return RVSEG_OK;
}

}  // namespace rvseg

using namespace rvseg;

extern "C" rvseg_status rvseg_project_cloud_device(rvseg_ctx* ctx, int32_t n_images, const float* proj, int32_t N, const float* d_cloud_xyz,
                                                   int32_t* d_index_out, float* d_zbuffer_out, void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_status st = project_check(ctx, n_images, proj, N, d_cloud_xyz, d_index_out);
    if (st != RVSEG_OK) return st;
    if (n_images == 0) return RVSEG_OK;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    FusionState* fs;
    if ((st = fusion_state(ctx, &fs)) != RVSEG_OK) return st;
    hipStream_t s = stream_of(ctx, hip_stream);
    timer_reset(ctx);
    timer_mark(ctx, "project", s);
    st = project_enqueue(ctx, fs, n_images, proj, N, d_cloud_xyz, d_index_out, d_zbuffer_out, s);
    timer_mark(ctx, "end", s);
    return st;
}

extern "C" rvseg_status rvseg_project_cloud(rvseg_ctx* ctx, int32_t n_images, const float* proj, int32_t N, const float* cloud_xyz,
                                            int32_t* index_out, float* zbuffer_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    rvseg_status st = project_check(ctx, n_images, proj, N, cloud_xyz, index_out);
    if (st != RVSEG_OK) return st;
    if (n_images == 0) return RVSEG_OK;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    FusionState* fs;
    if ((st = fusion_state(ctx, &fs)) != RVSEG_OK) return st;
    hipStream_t s = ctx->stream;
    const size_t n = (size_t)n_images * ctx->params.width * ctx->params.height;
    if ((st = dev_reserve(ctx, fs->proj_xyz, (size_t)(N > 0 ? N : 1) * 12)) != RVSEG_OK) return st;
    if ((st = dev_reserve(ctx, fs->proj_stage_idx, n * 4)) != RVSEG_OK) return st;
    if (zbuffer_out && (st = dev_reserve(ctx, fs->proj_stage_z, n * 4)) != RVSEG_OK) return st;
    if (N > 0) RV_HIP(ctx, hipMemcpyAsync(fs->proj_xyz.p, cloud_xyz, (size_t)N * 12, hipMemcpyHostToDevice, s));
    if ((st = project_enqueue(ctx, fs, n_images, proj, N, fs->proj_xyz.as<float>(), fs->proj_stage_idx.as<int32_t>(),
                              zbuffer_out ? fs->proj_stage_z.as<float>() : nullptr, s)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(index_out, fs->proj_stage_idx.p, n * 4, hipMemcpyDeviceToHost, s));
    if (zbuffer_out) RV_HIP(ctx, hipMemcpyAsync(zbuffer_out, fs->proj_stage_z.p, n * 4, hipMemcpyDeviceToHost, s));
    RV_HIP(ctx, hipStreamSynchronize(s));
    return RVSEG_OK;
}

// K * [R_c^T | -R_c^T t_c] * T^-1 in double, in the order include/rvseg.h writes down, rounded to fp32 once
extern "C" rvseg_status rvseg_projection_matrix(const float K[9], const float calib_R_t[12], const float node_pose[12], float P_out[12]) {
    if (!K || !calib_R_t || !node_pose || !P_out) return RVSEG_ERR_INVALID_ARG;
    auto dot3 = [](double a0, double b0, double a1, double b1, double a2, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; };
    double Rc[3][3], tc[3], Rn[3][3], tn[3], A[3][3], b[3], c[3];
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) { Rc[r][k] = calib_R_t[r * 3 + k]; Rn[r][k] = node_pose[r * 4 + k]; }
        tc[r] = calib_R_t[9 + r];
        tn[r] = node_pose[r * 4 + 3];
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) A[i][j] = dot3(Rc[0][i], Rn[j][0], Rc[1][i], Rn[j][1], Rc[2][i], Rn[j][2]);   // R_c^T * R_n^T
    for (int i = 0; i < 3; i++) b[i] = dot3(Rn[0][i], tn[0], Rn[1][i], tn[1], Rn[2][i], tn[2]);                   // R_n^T * t_n
    for (int i = 0; i < 3; i++) c[i] = dot3(Rc[0][i], b[0] + tc[0], Rc[1][i], b[1] + tc[1], Rc[2][i], b[2] + tc[2]);
    for (int r = 0; r < 3; r++) {
        for (int j = 0; j < 3; j++) P_out[r * 4 + j] = (float)dot3(K[r * 3], A[0][j], K[r * 3 + 1], A[1][j], K[r * 3 + 2], A[2][j]);
        P_out[r * 4 + 3] = (float)-dot3(K[r * 3], c[0], K[r * 3 + 1], c[1], K[r * 3 + 2], c[2]);
    }
    return RVSEG_OK;
}
