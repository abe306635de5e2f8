// Launch interface between the forest learner (rvseg_train.hip) and its kernels (kernels_train.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rvseg_kernels.h"
#include "train_host.h"

namespace rvseg {

constexpr int TR_BINS = 256;    // values of a byte feature

// The training set on the device, passed to kernels by value: feature-major, bytes for byte-valued features, floats for
// the others.
struct TrainSetView {
    int P, D, L;
    size_t stride;          // elements per feature row (>= P)
    uint8_t* Xb;            // [D][stride]
    float* Xf;              // [n_nb][stride]
    int* lab;               // [L][stride] class index per layer
    const int* nb_index;    // [D]: row of the feature in Xf, -1 for a byte feature
};

// The slot tables of one batch of a level: a slot is a frontier node that is being searched.
struct LevelSlots {
    int K;                  // sampled features per slot
    const int* node_of;     // [P] node of every example
    const int* slot_of;     // [nodes] slot of a node, -1 outside the batch
    const unsigned* w;      // [P] bootstrap multiplicity
    const int* slot_layer;  // [slots] label layer the node drew
    const int* slot_feat;   // [slots][K] features the node drew, in sampled order
};

// The class weights of one tree's split objective (rvseg_class_prior), passed to the cut kernels by value: 16 floats,
// uniform across the launch, so they sit in scalar registers.  A class the tree's data set does not hold has 0 here;
// the kernels never read it.
struct ClassWeights {
    float w[TR_CMAX];
};

// ---- data set construction ------------------------------------------------------------------------------------
// per feature of the row-major P x D matrix X: not_byte[f] = 1 unless every value is an integer in [0, 255];
// not_finite[0] = 1 when a value is NaN or infinite
void launch_train_feature_stats(const float* X, int P, int D, int* not_byte, int* not_finite, hipStream_t s);
void launch_train_pack(const float* X, const TrainSetView& v, hipStream_t s);
// flags[p] = the stride-grid point has valid depth and every label layer is >= 0 there
void launch_train_frame_flags(const FrameGeom& g, const uint8_t* valid, const int8_t* labels, int L, int* flags, hipStream_t s);
// the flagged points' features and labels to rows base + offs[p] of the set
void launch_train_frame_scatter(const FrameGeom& g, const int* flags, const int* offs, const float* dump, const int8_t* labels, size_t base,
                                const TrainSetView& v, hipStream_t s);
size_t train_scan_temp_bytes(size_t n);
hipError_t launch_train_scan_offsets(void* temp, size_t temp_bytes, const int* flags, int* offs, size_t n, hipStream_t s);

// ---- the learner ----------------------------------------------------------------------------------------------
// mult (null: every example once): how often the tree's data set holds each example -- a boosting round's resample
void launch_train_class_count(const TrainSetView& v, const unsigned* mult, unsigned* cnt, hipStream_t s);   // cnt[layer][TR_CMAX] += mult
// w += P draws with replacement from the P positions of the data set; positions (null: position n is example n): the
// example at each position of a resample
void launch_train_bootstrap(int P, uint64_t kt, const int* positions, unsigned* w, hipStream_t s);
// The two cut searches take the tree's class weights `cw`: null runs the integer objective (oracle definition 2), else
// the class-weighted one (rvseg_class_prior, definition 2).
// byte features of S slots: class totals, (feature, value, class) histograms, the best cut of every (slot, feature)
void launch_train_search_bytes(const TrainSetView& v, const LevelSlots& sl, int S, const ClassWeights* cw, unsigned* totals, unsigned* hist,
                               CutResult* cuts, hipStream_t s);
// float features: one (segment << 32 | ordered value, example) pair per (bootstrap example, sampled float feature)
void launch_train_emit(const TrainSetView& v, const LevelSlots& sl, unsigned long long* keys, unsigned* vals, unsigned* counter,
                       unsigned capacity, hipStream_t s);
size_t train_sort_temp_bytes(size_t n);
hipError_t launch_train_sort(void* temp, size_t temp_bytes, unsigned long long* keys_in, unsigned long long* keys_out, unsigned* vals_in,
                             unsigned* vals_out, size_t n, unsigned end_bit, hipStream_t s);
// the best cut of every float (slot, feature) segment of the sorted pairs (needs the slots' totals)
void launch_train_scan(const TrainSetView& v, const LevelSlots& sl, int S, const ClassWeights* cw, unsigned n_items, const unsigned long long* keys,
                       const unsigned* vals, const unsigned* totals, CutResult* cuts, hipStream_t s);
// every example of a freshly split node moves to a child
void launch_train_route(const TrainSetView& v, int* node_of, const int* split_feat, const float* split_thr, const int* split_left,
                        hipStream_t s);
void launch_train_leaf_count(const TrainSetView& v, const int* node_of, const unsigned* mult, unsigned* cnt, hipStream_t s);   // cnt[node][layer][TR_CMAX] += mult

// ---- a boosting round (BoostedRandomForestLearner::learn, learning.cpp:1162-1217) ------------------------------
// idx[n] = the first index with !(u_n > cumsum[index]), clamped to N - 1, u_n = boost_uniform(kb, n); mult[idx[n]] += 1
// (mult may be null)
void launch_train_boost_resample(const float* cumsum, int N, uint64_t kb, int* idx, unsigned* mult, hipStream_t s);
// miss[n] = (vote_label[node_of[n]] != label[n])
void launch_train_vote_flags(const int* node_of, const int* vote_label, const int* label, int N, uint8_t* miss, hipStream_t s);
// The ordered fp32 sums, each bit for bit the serial chain in example order, each one wave:
//   error[0] = sum of w[n] over the misses
void launch_train_boost_error(const float* w, const uint8_t* miss, int N, float* error, hipStream_t s);
//   w[n] *= scale for the misses (one fp32 multiply), then total[0] = sum of w[n]
void launch_train_boost_update_total(float* w, const uint8_t* miss, int N, float scale, float* total, hipStream_t s);
//   w[n] /= total[0], then cumsum[n] = w[n] + cumsum[n-1]
void launch_train_boost_update_cumsum(float* w, int N, const float* total, float* cumsum, hipStream_t s);

}  // namespace rvseg
