// The external provider of single-frame semantics (replaces Segmenter::processFramesFromQueueExternal,
// src/segmenter.cpp:445-514): the rectified xyz image of the request (:466-488), the layer layout the provider's
// distributions come in (single_frame_segmentation_server.py:68-71), and the frame CRF on those distributions.  The
// frame machinery itself (chunks, staging ring, overflow contract) is rvseg_pipeline.hip's segment_host / segment_device.
#include <cstdint>

#include "rvseg_internal.h"
#include "rvseg_kernels.h"
#include "rvseg_pipeline.h"

namespace rvseg {

// ---------------------------------------------------------------------------------------------
// rectify_depth: depth (mm) -> (R*Kinv)*(d*x, d*y, d) + t as three packed floats per pixel, NaN outside
// [depth_min, depth_max].  The expressions are prep_kernel's (kernels_features.hip) and the oracle's orc_cloud: products
// and sums rounded one by one, left to right (the file is compiled with -ffp-contract=off).
// Pure streaming, 2 B in and 12 B out per pixel: a lane takes four consecutive pixels of the n x H x W array -- one
// 8-byte load, three 16-byte stores, 48 contiguous bytes.  Four pixels may cross a row end (or, when W*H is no multiple
// of four, a frame end), so x, y and the frame are carried per pixel; the last (n*W*H) % 4 pixels, and every pixel when
// a pointer is not aligned for the wide accesses, go one at a time.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void rectify_pixel(const float* __restrict__ A, uint16_t mm, int x, int y, float dmin, float dmax,
                                              float& ox, float& oy, float& oz) {
    const float d = (float)mm / 1000.0f;
    float m0, m1, m2;
    if (d < dmin || d > dmax) {
        m0 = m1 = m2 = __int_as_float(0x7fc00000);
    } else {
        m0 = d * (float)x; m1 = d * (float)y; m2 = d;
    }
    ox = ((A[0] * m0 + A[1] * m1) + A[2] * m2) + A[9];
    oy = ((A[3] * m0 + A[4] * m1) + A[5] * m2) + A[10];
    oz = ((A[6] * m0 + A[7] * m1) + A[8] * m2) + A[11];
}

__global__ void __launch_bounds__(256)
rectify_depth_kernel(int W, int npix, size_t total, float dmin, float dmax, const uint16_t* __restrict__ depth,
                     const float* __restrict__ calibA,   // n x 12: A = R*Kinv (row-major 9), t (3)
                     float* __restrict__ xyz, int wide) {
    const size_t first = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (first >= total) return;
    int frame = (int)(first / (size_t)npix);
    int pix = (int)(first - (size_t)frame * npix);
    int y = pix / W, x = pix - y * W;
    const bool full = wide && first + 4 <= total;
    const int count = first + 4 <= total ? 4 : (int)(total - first);
    uint16_t mm[4] = {0, 0, 0, 0};
    if (full) {
        const uint2 v = *reinterpret_cast<const uint2*>(depth + first);
        mm[0] = (uint16_t)(v.x & 0xffffu); mm[1] = (uint16_t)(v.x >> 16);
        mm[2] = (uint16_t)(v.y & 0xffffu); mm[3] = (uint16_t)(v.y >> 16);
    } else {
        for (int k = 0; k < count; k++) mm[k] = depth[first + k];
    }
    float o[12];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        if (k < count) rectify_pixel(calibA + (size_t)frame * 12, mm[k], x, y, dmin, dmax, o[3 * k], o[3 * k + 1], o[3 * k + 2]);
        else o[3 * k] = o[3 * k + 1] = o[3 * k + 2] = 0.f;
        // the next pixel: row end, then frame end
        if (++x == W) { x = 0; y++; }
        if (++pix == npix) { pix = 0; y = 0; frame++; }
    }
    float* out = xyz + first * 3;
    if (full) {
        float4* out4 = reinterpret_cast<float4*>(out);
        out4[0] = make_float4(o[0], o[1], o[2], o[3]);
        out4[1] = make_float4(o[4], o[5], o[6], o[7]);
        out4[2] = make_float4(o[8], o[9], o[10], o[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; k++)
            if (k < 3 * count) out[k] = o[k];
    }
}

static void launch_rectify_depth(int W, int H, int n, float dmin, float dmax, const uint16_t* d_depth, const float* d_calibA,
                                 float* d_xyz, hipStream_t s) {
    const size_t total = (size_t)W * H * n;
    const size_t lanes = (total + 3) / 4;
    const int wide = ((uintptr_t)d_depth % 8 == 0 && (uintptr_t)d_xyz % 16 == 0) ? 1 : 0;
    rectify_depth_kernel<<<dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s>>>(W, W * H, total, dmin, dmax, d_depth, d_calibA,
                                                                                     d_xyz, wide);
    RV_LAUNCHED("rectify_depth_kernel");
}

// what the two segment entries share: the argument rules of include/rvseg.h
static rvseg_status external_args(rvseg_ctx* ctx, int32_t n_frames, const void* rgb, const void* depth, const float* calib,
                                  const void* dist, int32_t dist_stride) {
    if (ctx->external.n_layers == 0) {
        ctx->err = "no external layer layout set (rvseg_external_layers_set)";
        return RVSEG_ERR_INVALID_ARG;
    }
    if (n_frames < 0 || (n_frames > 0 && (!rgb || !depth || !calib || !dist))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (dist_stride != 1 && dist_stride != ctx->params.stride) {
        ctx->err = "dist_stride must be 1 (full resolution) or params.stride";
        return RVSEG_ERR_INVALID_ARG;
    }
    return RVSEG_OK;
}

}  // namespace rvseg

using namespace rvseg;

extern "C" {

rvseg_status rvseg_rectify_depth_device(rvseg_ctx* ctx, int32_t n_frames, const uint16_t* d_depth_mm, const float* calib,
                                        float depth_min, float depth_max, float* d_xyz_out, void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (n_frames < 0 || (n_frames > 0 && (!d_depth_mm || !calib || !d_xyz_out))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (n_frames == 0) return RVSEG_OK;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    Pipeline* im = pipeline_of(ctx);   // the calibration ring only: no frame tables, so no stride rule applies here
    hipStream_t s = stream_of(ctx, hip_stream);
    rvseg_status st = upload_calib(ctx, im, calib, n_frames, s);
    if (st != RVSEG_OK) return st;
    launch_rectify_depth(ctx->params.width, ctx->params.height, n_frames, depth_min, depth_max, d_depth_mm, im->calibA.as<float>(),
                         d_xyz_out, s);
    RV_LAUNCH_OK(ctx);
    return RVSEG_OK;
}

rvseg_status rvseg_rectify_depth(rvseg_ctx* ctx, int32_t n_frames, const uint16_t* depth_mm, const float* calib, float depth_min,
                                 float depth_max, float* xyz_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    if (n_frames < 0 || (n_frames > 0 && (!depth_mm || !calib || !xyz_out))) { ctx->err = "bad arguments"; return RVSEG_ERR_INVALID_ARG; }
    if (n_frames == 0) return RVSEG_OK;
    RV_HIP(ctx, hipSetDevice(ctx->params.device));
    const size_t npix = (size_t)ctx->params.width * ctx->params.height;
    DevBuf d_depth, d_xyz;   // freed on every return (hipFree waits for the device)
    rvseg_status st;
    if ((st = dev_alloc(ctx, d_depth, npix * 2 * n_frames)) != RVSEG_OK) return st;
    if ((st = dev_alloc(ctx, d_xyz, npix * 12 * n_frames)) != RVSEG_OK) return st;
    RV_HIP(ctx, hipMemcpyAsync(d_depth.p, depth_mm, npix * 2 * n_frames, hipMemcpyHostToDevice, ctx->stream));
    if ((st = rvseg_rectify_depth_device(ctx, n_frames, d_depth.as<uint16_t>(), calib, depth_min, depth_max, d_xyz.as<float>(),
                                         nullptr)) != RVSEG_OK) { (void)hipStreamSynchronize(ctx->stream); return st; }
    RV_HIP(ctx, hipMemcpyAsync(xyz_out, d_xyz.p, npix * 12 * n_frames, hipMemcpyDeviceToHost, ctx->stream));
    RV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RVSEG_OK;
}

rvseg_status rvseg_external_layers_set(rvseg_ctx* ctx, int32_t n_layers, const int32_t* class_counts) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    // the limits of the forest loader (upload_forest)
    if (n_layers < 1 || n_layers > RVSEG_MAX_LAYERS) { ctx->err = "external layers: 1 to 8 label layers"; return RVSEG_ERR_INVALID_ARG; }
    if (!class_counts) { ctx->err = "external layers: null class counts"; return RVSEG_ERR_INVALID_ARG; }
    int sum = 0;
    for (int l = 0; l < n_layers; l++) {
        if (class_counts[l] < 1 || class_counts[l] > kMaxClasses) { ctx->err = "external layers: every layer needs 1 to 64 classes"; return RVSEG_ERR_INVALID_ARG; }
        sum += class_counts[l];
    }
    if (sum > kMaxClasses) { ctx->err = "external layers: more than 64 classes over all layers is not supported"; return RVSEG_ERR_INVALID_ARG; }
    // every limit is checked before the layout is touched: a refused call leaves the previous one in place
    LayerLayout lay;
    lay.n_layers = n_layers;
    for (int l = 0; l < n_layers; l++) lay.class_counts[l] = class_counts[l];
    lay.sum_classes = sum;
    ctx->external = lay;
    return RVSEG_OK;
}

rvseg_status rvseg_segment_external_device(rvseg_ctx* ctx, int32_t n_frames, const uint8_t* d_rgb, const uint16_t* d_depth_mm,
                                           const float* calib, const float* d_distributions, int32_t dist_stride,
                                           float* d_marginals_out, int8_t* d_labels_out, void* hip_stream) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    const rvseg_status st = external_args(ctx, n_frames, d_rgb, d_depth_mm, calib, d_distributions, dist_stride);
    if (st != RVSEG_OK) return st;
    if (n_frames == 0) return RVSEG_OK;
    const ExternalInput ext{d_distributions, dist_stride};
    return segment_device(ctx, &ext, n_frames, d_rgb, d_depth_mm, calib, nullptr, d_marginals_out, d_labels_out, hip_stream);
}

rvseg_status rvseg_segment_external(rvseg_ctx* ctx, int32_t n_frames, const uint8_t* rgb, const uint16_t* depth_mm, const float* calib,
                                    const float* distributions, int32_t dist_stride, float* marginals_out, int8_t* labels_out) {
    if (!ctx) return RVSEG_ERR_INVALID_ARG;
    const rvseg_status st = external_args(ctx, n_frames, rgb, depth_mm, calib, distributions, dist_stride);
    if (st != RVSEG_OK) return st;
    if (n_frames == 0) return RVSEG_OK;
    const ExternalInput ext{distributions, dist_stride};
    return segment_host(ctx, &ext, n_frames, rgb, depth_mm, calib, nullptr, marginals_out, labels_out);
}

}  // extern "C"
