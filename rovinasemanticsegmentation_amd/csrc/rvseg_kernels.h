// Kernel-launch interface between the pipeline translation unit and the kernel files.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rvseg_internal.h"

namespace rvseg {

// Geometry + feature layout of one camera configuration, passed to kernels by value.
struct FrameGeom {
    int W, H, stride;
    int lw, lh;                 // stride grid = low-resolution posterior image (W/stride x H/stride)
    float depth_min, depth_max; // metres (cloud NaN rule, feature_extractor.h:210)
    float dmin_mm, dmax_mm;     // float(d*1000.0) (mask rule, feature_extractor.h:43-44,60)
    int patch_size, r;          // patch_size, patch_size_reduce
    int n_patch;                // r*r*3 or 0 when the colour patch is disabled
    int pos_depth, pos_height, pos_normal; // index of each scalar feature in the vector or -1
    int D;                      // feature length
    float fill;                 // low-res image fill value
    int rt_rows;                // rows of the ResizeRow table (largest ROI half size + 1), 0 without colour patch
};

struct LabCoeffs { int c[9]; };

// cv::resize coefficient tables of the 8-bit patch path, one row per ROI half size
// (size = 2*half+1), host-computed with the formula the oracle states (OpenCV 2.4 imgwarp.cpp).
constexpr int RT_MAXR = 16;
struct ResizeRec { int16_t ofs, w0, w1, ofs1; };   // first tap, 11-bit weights of the two taps, second tap (both inside the ROI)
struct ResizeRow {
    ResizeRec x[RT_MAXR];   // x axis: weights clamped at the ROI border (OpenCV's xofs / alpha)
    ResizeRec y[RT_MAXR];   // y axis: weights kept, the two rows clipped to the ROI (OpenCV's yofs / beta + row clipping)
};

// float up-sampling tables (cv::resize INTER_LINEAR on CV_32FC(n), segmenter.cpp:380-382)
struct UpsampleTables {
    DevBuf xofs, ax0, ax1;  // W entries
    DevBuf yofs, ay0, ay1;  // H entries
};

// ---- kernels_features.hip --------------------------------------------------------------------
// d_lab2 (optional): the Lab image again with every pixel next to the one below it, {lab(y, x), lab(y + 1, x)} per
// pixel: a bilinear tap quad of the patch resize is then ONE 16-byte load (kernels_rf.hip, rf_frames_lazy_kernel)
void launch_prep(const FrameGeom& g, const LabTables& lab, const uint8_t* d_rgb, const uint16_t* d_depth,
                 const float* d_calibA, uint32_t* d_lab, float4* d_cloud, uint8_t* d_change, int n, hipStream_t s,
                 uint2* d_lab2 = nullptr);
void launch_window_map(const FrameGeom& g, const float4* d_cloud, uint8_t* d_change, uint8_t* d_rect, int n, hipStream_t s);
void launch_normal_feature(const FrameGeom& g, const float4* d_cloud, const uint8_t* d_rect, float* d_nfeat,
                           int n, hipStream_t s);

// ---- kernels_forest_tools.hip ----------------------------------------------------------------
// The loaded forest on one chunk of n points with materialised D-dimensional features (rvseg_forest_tools.hip).
// Per-tree tables are [T][stride], stride a multiple of 4 and >= n; every output of launch_tools_votes is optional.
//   d_out        : [n][S] the forest's posterior sums
//   d_vote_table : per leaf row, the label rule on the leaf's own histogram of the layer
//   d_pred       : [n] the forest's label of the layer's classes [layer_off, layer_off + C) of a leaf row
struct RefitLayers { int n_layers, sum_classes, class_counts[RVSEG_MAX_LAYERS], offset[RVSEG_MAX_LAYERS]; };
void launch_forest_eval(const DeviceForest& f, const float* d_X, int n, int D, float* d_out, hipStream_t s);
void launch_tools_votes(const DeviceForest& f, const uint8_t* d_vote_table, int layer_off, int C, const float* d_X, int n, int D,
                        size_t stride, int32_t* d_rows, uint8_t* d_votes, int32_t* d_pred, hipStream_t s);
// d_agree [T][T] += the points of the chunk on which two trees vote alike; d_confusion [C][C] += [label][pred];
// d_counts [leaf row][sum_classes] += the chunk's examples per (layer, class).  d_flag: a label was out of range.
void launch_tools_agree(const uint8_t* d_votes, int n_trees, int n, int stride, int max_blocks, unsigned long long* d_agree, hipStream_t s);
void launch_tools_confusion(const int32_t* d_labels, const int32_t* d_pred, int n, int C, int max_blocks, unsigned long long* d_confusion,
                            int* d_flag, hipStream_t s);
void launch_tools_refit_count(const int32_t* d_rows, const int32_t* d_labels, int n_trees, int n, int stride, const RefitLayers& lay,
                              int max_blocks, uint32_t* d_counts, int* d_flag, hipStream_t s);

// ---- kernels_prune.hip -----------------------------------------------------------------------
// The simulated-annealing chain of rvseg_forest_prune, one launch per proposal (rules: prune_host.h).  d_votes is
// [T][stride] bytes and d_labels [stride], stride a multiple of 4 and the tails beyond P zero.  What the chain carries
// from launch to launch lives in one PruneControl on the device; errors and ticket are zero between launches.
struct PruneStep;   // prune_host.h
struct PruneControl {
    unsigned errors, ticket;                          // this launch's error count; blocks that have added theirs
    int32_t n_state[2], n_best;
    float cur_energy, best_energy;
    int32_t pad;
    int32_t state[2][RVSEG_PRUNE_MAX_STATE];          // step s reads state[s & 1] and writes state[(s + 1) & 1]
    int32_t best[RVSEG_PRUNE_MAX_STATE];
};
int prune_grid(int P, int max_blocks);
// state[0] / n_state[0] -> its energy as cur_energy and best_energy, itself as the best state
void launch_prune_init(const uint8_t* d_votes, const int32_t* d_labels, int P, size_t stride, int grid, PruneControl* d_ctl, hipStream_t s);
// steps first_step .. first_step + n_steps - 1, back to back; d_step_kind [all steps], d_trace [all iterations]
void launch_prune_steps(const uint8_t* d_votes, const int32_t* d_labels, int P, size_t stride, int grid, const PruneStep* d_steps,
                        int first_step, int n_steps, PruneControl* d_ctl, uint8_t* d_step_kind, rvseg_prune_trace_row* d_trace, hipStream_t s);

// ---- kernels_rf.hip --------------------------------------------------------------------------
// The frame path: per-point features computed on demand + forest traversal over the stride grid of n frames.
//   d_low   : n x (lh*lw*S) low-resolution log-posteriors, layers concatenated per frame, each
//             [ly][lx][class]; invalid-depth cells receive g.fill
//   d_lab2  : the row-pair Lab image of launch_prep, when rf_frames_wants_lab2(f)
void launch_rf_frames(const FrameGeom& g, const DeviceForest& f, const ResizeRow* d_rt, const uint32_t* d_lab,
                      const uint16_t* d_depth, const float4* d_cloud, const float* d_nfeat, float* d_low, int n,
                      hipStream_t s, const uint2* d_lab2 = nullptr);
// true when the frame kernel can use the row-pair Lab image (8-byte nodes exist for this model)
bool rf_frames_wants_lab2(const DeviceForest& f);
// The same features materialised (rvseg_extract_features, rvseg_forest_train_frames); needs no model.
//   d_dump  : n x (lh*lw) x D feature vectors, zero patch values at invalid-depth points
//   d_valid : n x (lh*lw) mask bytes
void launch_feature_dump(const FrameGeom& g, const ResizeRow* d_rt, const uint32_t* d_lab, const uint16_t* d_depth,
                         const float4* d_cloud, const float* d_nfeat, float* d_dump, uint8_t* d_valid, int n, hipStream_t s);
// cv::resize to full resolution + pack [layer][y][x][class] (segmenter.cpp:380-431)
void launch_upsample_pack(const FrameGeom& g, const LayerLayout& f, const UpsampleTables& t,
                          const float* d_low, float* d_post, int n, hipStream_t s);
// label rules (rvseg_label_mode) over N points x C classes, class-contiguous
void launch_labels_frames(const float* d_values, int n_frames, int N, const LayerLayout& f, int mode, const int* unknown,
                          int8_t* d_labels, hipStream_t s);
void launch_labels(const float* d_values, size_t n_points, int C, int mode, int unknown, int8_t* d_labels,
                   hipStream_t s);

}  // namespace rvseg
