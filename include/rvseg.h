/*
 * rvseg.h -- C ABI of librvseg.so: the MI355X (gfx950) per-pixel inference path
 *
 *     RGB-D frame -> feature_extractor -> libforest random-forest evaluation
 *                 -> DenseCRF mean-field (permutohedral lattice) -> softmax / argmax
 *
 * This is the drop-in boundary for the hot path of VisualComputingInstitute/
 * RovinaSemanticSegmentation.  The reference has no FFI: the path is reached by ordinary C++
 * calls from `class Segmenter` (include/segmenter.h:47-69).  Every entry point below names the
 * reference interface it replaces (paths relative to the reference tree).  Plain pointers and
 * sizes only; no C++ or torch types cross this boundary; nothing throws across it.
 *
 * Memory conventions
 *   - "host" entry points take host pointers and copy through HBM themselves.
 *   - "_device" entry points take device (HBM) pointers plus a hipStream_t passed as void*;
 *     they enqueue work on that stream and return without synchronising.
 *   - A ctx owns its device buffers, forest copy and LUTs; the caller owns every in/out buffer.
 *   - One ctx per (thread, device).  Calls on one ctx must be serialised by the caller, exactly
 *     as the reference serialises its libraries behind _frame_mtx (src/segmenter.cpp:336-435).
 *
 * Layouts (identical to the reference's)
 *   rgb        n x H x W x 3 uint8, channel order as delivered to FeatureExtractor::extract
 *              (RGB; the R/B swap inside CV_BGR2Lab is part of the trained feature definition,
 *              include/feature_extractor.h:129, src/test.cpp:130)
 *   depth_mm   n x H x W uint16, millimetres (include/feature_extractor.h:59-60)
 *   calib      21 floats: K^-1 (3x3 row-major), R (3x3 row-major), t (3): Calibration::
 *              _intrinsic_inverse, _extrinsic.linear(), _extrinsic.translation()
 *              (include/calibration.h:19-21; used at include/feature_extractor.h:223)
 *   posteriors per frame: layers concatenated, each [y][x][class] float32, offset of layer l =
 *              sum_{l'<l} H*W*C_l'  (src/segmenter.cpp:413-431; srv/SingleFrameSegmentation.srv
 *              label_distribution)
 *   labels     per frame: layers concatenated, each H x W int8
 *   CRF        unary / Q: N x C float32, class-contiguous per point (= column-major C x N
 *              Eigen::MatrixXf, third-party/densecrf/include/densecrf.h:56);
 *              features: N x d float32 (= column-major d x N)
 */
#ifndef RVSEG_H
#define RVSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVSEG_MAX_LAYERS 8

typedef struct rvseg_ctx rvseg_ctx;

typedef enum rvseg_status {
    RVSEG_OK = 0,
    RVSEG_ERR_INVALID_ARG = 1, /* bad pointer / size / parameter                                   */
    RVSEG_ERR_IO = 2,          /* libf::Exception("Could not open file.") (libforest io.h:118-121) */
    RVSEG_ERR_FORMAT = 3,      /* malformed or inconsistent forest.dat                             */
    RVSEG_ERR_NO_FOREST = 4,   /* empty forest: the reference asserts (classifier.cpp:168,189),
                                  compiled out in Release -> UB; here a clean error               */
    RVSEG_ERR_HIP = 5,         /* HIP runtime failure (message in rvseg_last_error)                */
    RVSEG_ERR_NO_DEVICE = 6,   /* no gfx950 device: the product never falls back to the CPU        */
    RVSEG_ERR_CAPACITY = 7,    /* lattice hash table / batch / ensemble capacity exceeded          */
    RVSEG_NOT_READY = 8        /* rvseg_poll_status without waiting: the work is still running      */
} rvseg_status;

/* Label rules found in the reference. */
typedef enum rvseg_label_mode {
    RVSEG_LABEL_EVAL = 0,     /* src/test.cpp:160-175: strict '>' from -1000, -1 when nothing wins  */
    RVSEG_LABEL_CRF = 1,      /* src/segmenter.cpp:646-657: strict '>' from 2.0/C else "Unknown"    */
    RVSEG_LABEL_NOCRF = 2,    /* src/segmenter.cpp:664-679: strict '>' from -1000, sum!=0 guard     */
    RVSEG_LABEL_ARGMAX = 3    /* DenseCRF::currentMap, densecrf.cpp:202-211: first maximum          */
} rvseg_label_mode;

/* Parameter block = the hot-path keys of resources/config.json. */
typedef struct rvseg_params {
    int32_t width, height;          /* camera size (Segmenter::_camera_w/_camera_h)                */
    int32_t stride;                 /* rf_prediction_stride, config.json:87                         */
    float depth_min, depth_max;     /* config.json:89-90 (metres)                                   */
    int32_t patch_size;             /* config.json:32                                               */
    int32_t patch_size_reduce;      /* config.json:34                                               */
    int32_t feature_color_patch, feature_depth, feature_height, feature_normal; /* config.json:41-44 */
    float fill_value;               /* low-res image init: 0 (segmenter.cpp:358-362) or -1000
                                       (test.cpp:143-147)                                           */
    int32_t use_dense_crf;          /* config.json:81 (per-frame CRF as composed by the north star) */
    float dcrf_xyz_kernel, dcrf_rgb_kernel, dcrf_kernel_weight; /* config.json:82-84 (multipliers)  */
    int32_t dcrf_iterations;        /* config.json:85                                               */
    int32_t multi_layer;            /* 1: multiClassLogPosterior (shared forest, segmenter.cpp:368),
                                       0: classLogPosterior (test.cpp:151)                          */
    int32_t label_mode;             /* rvseg_label_mode                                             */
    int32_t unknown_label[RVSEG_MAX_LAYERS]; /* Segmenter::_layer_unknown_label, segmenter.cpp:88-96 */
    int32_t max_batch;              /* frames processed per launch group (device buffers are sized
                                       for this many frames); 1 .. 4096, and at most 1022 with
                                       use_dense_crf (the lattice's 10-bit frame field): rvseg_create
                                       refuses more with RVSEG_ERR_INVALID_ARG                      */
    int32_t device;                 /* HIP device ordinal                                           */
    int32_t lattice_capacity_log2;  /* hash-table slots per frame = 2^this; 0 = 2^12 (the Segmenter
                                       kernel gives ~300 vertices / frame on the synthetic scenes, up to
                                       ~2 200 on a real photo with a 1-10 m depth range), -1 = worst case
                                       2*N*(d+1).  Overflow is detected, never silent: the context then
                                       raises its capacity (x8 per step, up to the worst case) for all
                                       later work; host entry points redo the chunk themselves, the
                                       asynchronous _device entry point reports RVSEG_ERR_CAPACITY from
                                       rvseg_poll_status (and from the next call)                     */
} rvseg_params;

/* Fills *p with the defaults of resources/config.json. */
void rvseg_params_default(rvseg_params *p);

/* Replaces: Segmenter::Segmenter's model/feature set-up (src/segmenter.cpp:106-129) minus ROS.
 * Fails with RVSEG_ERR_NO_DEVICE when no GPU is present. */
rvseg_status rvseg_create(const rvseg_params *params, rvseg_ctx **out);
void rvseg_destroy(rvseg_ctx *ctx);
/* Message of the last failing call on ctx (or of the last failing rvseg_create if ctx == NULL). */
const char *rvseg_last_error(const rvseg_ctx *ctx);
const char *rvseg_status_string(rvseg_status s);
/* D of the feature vector, include/feature_extractor.h:46-51 (366 with the default config). */
int32_t rvseg_feature_length(const rvseg_ctx *ctx);

/* ---- forest: replaces libf::RandomForest::read (libforest classifier.cpp:222-235) ------------ */
rvseg_status rvseg_forest_load(rvseg_ctx *ctx, const char *path);
rvseg_status rvseg_forest_load_mem(rvseg_ctx *ctx, const void *buf, size_t size);
/* A stream that does not parse is refused and the loaded model stays.  A forest that parses but is past the
 * context's limits (more than 64 classes over all layers or 8 layers, no histograms for params.multi_layer) is
 * refused and leaves ctx with no model: calls that need one return RVSEG_ERR_NO_FOREST until a load succeeds. */
/* Host-only validation of a forest.dat image with the loader's own parser and limits (no context, no
 * GPU): format, child links, split features < feature_length (<= 0: not checked), at most 64 trees
 * (RVSEG_ERR_CAPACITY: libforest has no limit, the device evaluator does) and 64 classes.  err_out
 * (optional) receives the message.  The reference has no such check: a bad model "will result in
 * segfaults" (README.md:30). */
rvseg_status rvseg_forest_check(const void *buf, size_t size, int32_t feature_length, int32_t *n_trees,
                                int32_t *n_nodes_total, int32_t *max_depth, char *err_out, size_t err_cap);
/* Replaces libf::RandomForest::write (classifier.cpp:210-220; DecisionTree::write :144-152): the loaded
 * model in the reference's stream format, node for node -- a file read with rvseg_forest_load is
 * written back byte for byte.  _mem: *size_out receives the needed size; out may be NULL to query. */
rvseg_status rvseg_forest_write(const rvseg_ctx *ctx, const char *path);
rvseg_status rvseg_forest_write_mem(const rvseg_ctx *ctx, void *out, size_t out_cap, size_t *size_out);
/* The same writer without a context: parse `buf`, serialise it again (host only; used by the CPU tests
 * to pin the writer against the reference-written golden files). */
rvseg_status rvseg_forest_rewrite(const void *buf, size_t size, void *out, size_t out_cap, size_t *size_out);
/* ---- forest training on the GPU: replaces RandomForestLearner::learn + DecisionTreeLearner::learn +
 *      updateMultiHistograms + forest->write (libforest learning.cpp:410-1073, src/train.cpp:225-249) for the
 *      model family this path evaluates.  Parameters = the learner settings of src/train.cpp / config.json. */
typedef struct rvseg_train_params {
    int32_t num_trees;                /* config.json:37 (4)                                                   */
    int32_t max_depth;                /* config.json:38 (30): a node deeper than this is not split (learning.cpp:525) */
    int32_t min_split_examples;       /* config.json:39 (50)                                                  */
    int32_t min_child_split_examples; /* learning.h:116 (1)                                                   */
    int32_t num_features;             /* features tried per node; 0 = ceil(sqrt(D)) (autoconf, learning.cpp:367) */
    int32_t use_bootstrap;            /* 1 (train.cpp:226): N draws with replacement per tree                 */
    float smoothing;                  /* learning.h:117 (1): log((h + s) / (total + C s))                     */
    uint64_t seed;                    /* the reference seeds from std::random_device (learning.cpp:18) and is
                                         not reproducible; here equal seeds give equal bytes                  */
} rvseg_train_params;
void rvseg_train_params_default(rvseg_train_params *tp);
/* X: P x D host floats (one DataPoint per row), labels: P x n_layers class indices (DataStorage's multi labels),
 * class_counts per layer (at most 16 each).  Writes a forest.dat image (multi_histograms = the "shared" forest of
 * train.cpp:231; with one layer also `histograms`), loadable with rvseg_forest_load_mem and by the reference.
 * Search = the reference's: minimum of E(left) + E(right) (EfficientEntropyHistogram, fastlog2) over the thresholds at
 * midpoints of adjacent values at least 1e-6 apart (learning.cpp:578-592) -- exact for every feature: byte-valued
 * features through per-value histograms, the others through a sort per level; leaf histograms exactly as
 * updateMultiHistograms computes them (learning.cpp:960-1012); nodes numbered as the reference's depth-first stack
 * would.  Equal seeds give equal bytes, and the bytes equal the CPU oracle's depth-first learner (tests).
 * The trained model is also kept on the context: when out_cap is too small (RVSEG_ERR_INVALID_ARG, *size_out = needed
 * size) or forest_out is NULL, fetch it with rvseg_forest_train_result instead of training again. */
rvseg_status rvseg_forest_train(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels,
                                int32_t n_layers, const int32_t *class_counts, const rvseg_train_params *tp,
                                void *forest_out, size_t out_cap, size_t *size_out);
rvseg_status rvseg_forest_train_result(rvseg_ctx *ctx, void *forest_out, size_t out_cap, size_t *size_out);
/* Training straight from labelled key frames: replaces the extraction loop of src/train.cpp:115-147 as well.  Features
 * are extracted on the device (FeatureExtractor::extract, WITH_POSITIVE_LABEL branch: stride-grid points with valid
 * depth whose labels are all >= 0, include/feature_extractor.h:93-121) and packed there (Lab patch bytes as bytes,
 * depth / height / normal as floats); no P x D float matrix exists anywhere.
 *   rgb n x H x W x 3, depth_mm n x H x W, calib n x 21 (all host memory, the context's width / height / stride);
 *   labels n x L x H x W int8 (label_type = char, include/defines.h), < 0 = unlabelled
 *   augment != 0: the reference's augmentation -- every frame with colour offsets -20, 0, +20 (`color += a` on the
 *   8UC3 image, i.e. OpenCV's Scalar(a,0,0,0): channel 0 only, saturated) and each of those also flipped horizontally
 *   (colour, depth and labels, same calibration): six extractions per frame, in the reference's order
 *   n_examples_out (optional): training points extracted. */
rvseg_status rvseg_forest_train_frames(rvseg_ctx *ctx, int32_t n_frames, const uint8_t *rgb, const uint16_t *depth_mm,
                                       const float *calib, const int8_t *labels, int32_t n_layers,
                                       const int32_t *class_counts, int32_t augment, const rvseg_train_params *tp,
                                       void *forest_out, size_t out_cap, size_t *size_out, int32_t *n_examples_out);
/* n_layers / class_counts describe the active mode (multi_layer or single). */
rvseg_status rvseg_forest_info(const rvseg_ctx *ctx, int32_t *n_trees, int32_t *n_nodes_total,
                               int32_t *max_depth, int32_t *n_layers,
                               int32_t class_counts[RVSEG_MAX_LAYERS]);
/* Replaces: RandomForest::classLogPosterior / multiClassLogPosterior per DataPoint
 * (libforest classifier.cpp:166-208).  X: P x D host floats; out: P x sumC host floats. */
rvseg_status rvseg_forest_eval(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, float *out);

/* ---- boosted forest: replaces libf::BoostedRandomForest and BoostedRandomForestLearner (libforest
 *      classifier.cpp:238-307, learning.cpp:1117-1234, classifiers.h:349-425): multiclass AdaBoost (SAMME) over decision
 *      trees.  The model is T trees and one float weight per tree; classLogPosterior is a vector of C zeros to which, in
 *      tree order, weight_t is added at the label tree t votes for (Classifier::classify: the first index with the
 *      strictly greatest value of the leaf's single-label histogram).  multiClassLogPosterior is "not supported" there
 *      and here.
 *   Stream: int32 T, then per tree the weight and the tree.  BoostedRandomForest::write emits the weight first (:250-262),
 *   ::read expects the tree first (:264-280): the reference cannot read its own files.  The caller names the order; it is
 *   never guessed from the bytes. */
typedef enum rvseg_boosted_order {
    RVSEG_BOOSTED_WEIGHT_FIRST = 0,   /* what BoostedRandomForest::write produces (the default of the bindings) */
    RVSEG_BOOSTED_TREE_FIRST = 1,     /* what BoostedRandomForest::read accepts                                */
    RVSEG_BOOSTED_AS_LOADED = -1      /* the write calls only: the order the model was read in                 */
} rvseg_boosted_order;
/* Host-only validation, like rvseg_forest_check: its limits (64 trees, 64 classes, split features, child links), and
 * every leaf carries a non-empty single-label histogram of one class count, and the stream ends with the last tree. */
rvseg_status rvseg_boosted_check(const void *buf, size_t size, int32_t order, int32_t feature_length, int32_t *n_trees,
                                 int32_t *n_nodes_total, int32_t *max_depth, char *err_out, size_t err_cap);
/* Host-only: parse `buf` in in_order, serialise it in out_order.  Equal orders return the stream byte for byte. */
rvseg_status rvseg_boosted_rewrite(const void *buf, size_t size, int32_t in_order, int32_t out_order, void *out,
                                   size_t out_cap, size_t *size_out);
/* Replaces BoostedRandomForest::read.  The model becomes the context's forest: rvseg_forest_eval, rvseg_forest_info and
 * the single-layer frame path then return its vote sums (each leaf's device row is weight_t at its vote label and +0.0
 * elsewhere; a weight is stored as w + 0.0f, so -0.0 votes like the reference's 0 + (-0.0)).  A context with
 * params.multi_layer = 1 refuses it (RVSEG_ERR_INVALID_ARG) and keeps its previous model, as a stream that does not
 * parse does. */
rvseg_status rvseg_boosted_load(rvseg_ctx *ctx, const char *path, int32_t order);
rvseg_status rvseg_boosted_load_mem(rvseg_ctx *ctx, const void *buf, size_t size, int32_t order);
/* Replaces BoostedRandomForest::write: the loaded boosted model in `order`; a stream is written back byte for byte in
 * the order it was read in (RVSEG_BOOSTED_AS_LOADED).  RVSEG_ERR_NO_FOREST when the context's forest is not a boosted
 * one.  rvseg_forest_write and rvseg_forest_write_mem refuse a boosted model (RVSEG_ERR_INVALID_ARG). */
rvseg_status rvseg_boosted_write(const rvseg_ctx *ctx, const char *path, int32_t order);
rvseg_status rvseg_boosted_write_mem(const rvseg_ctx *ctx, int32_t order, void *out, size_t out_cap, size_t *size_out);
/* Replaces BoostedRandomForest::getWeights: the loaded model's tree weights as the stream holds them.  weights_out (cap floats) may be
 * NULL to query *n_out; order_out (optional): the order the model was read in. */
rvseg_status rvseg_boosted_weights(const rvseg_ctx *ctx, float *weights_out, int32_t cap, int32_t *n_out,
                                   int32_t *order_out);
/* Replaces BoostedRandomForestLearner::learn (learning.cpp:1120-1234) with a DecisionTreeLearner of tp's settings;
 * tp->num_trees is the number of boosting rounds (1..64).  X: P x D host floats, labels: P class indices of one layer
 * with C classes (2..16).  Per round: P draws from the example weights pick the tree's data set, the tree is learnt on
 * it (rvseg_forest_train's learner; tp->use_bootstrap is applied on top of the resample), error = the fp32 sum in
 * example order of the weights of the examples of the whole set the tree misclassifies, alpha = logf((1 - error) /
 * error) + log(C - 1) narrowed to float, misclassified weights are multiplied by expf(alpha), every weight is divided
 * by their fp32 sum.  All of it runs on the device but alpha.  The reference draws from std::random_device and has no
 * guard for degenerate rounds; here (build-owned definitions):
 *   1. round key kb = mix64(seed ^ mix64(0x626F6F73 + round)); draw n is u_n = (float)(draw64(kb, n) >> 40) * 2^-24;
 *      the round's tree is tree 0 of a one-tree forest trained with seed draw64(kb, 2^40) on the resample;
 *   2. u picks the first index i with !(u > cumsum[i]) (binary search), clamped to P - 1;
 *   3. error, the total and cumsum are fp32 sums in example order, bit for bit the serial chain;
 *   4. error == 0: the tree is added with alpha = +inf and boosting ends; error >= 1, or a total that is not positive
 *      and finite: the tree is not added and boosting ends; otherwise the reference's arithmetic, negative alpha included.
 * Writes the WEIGHT_FIRST stream (what the reference's write would).  The model is also kept on the context, apart
 * from any model it has loaded: when out_cap is too small (RVSEG_ERR_INVALID_ARG, *size_out = needed size) or out is
 * NULL, fetch it with rvseg_boosted_train_result, in either order, instead of training again.  errors_out / alphas_out (optional, tp->num_trees floats): per round that grew a tree;
 * rounds_out (optional): trees kept -- 0 when the first round stops without a tree; the stream is then the empty
 * ensemble's four bytes, which no loader accepts. */
rvseg_status rvseg_boosted_train(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels, int32_t C,
                                 const rvseg_train_params *tp, void *out, size_t out_cap, size_t *size_out,
                                 float *errors_out, float *alphas_out, int32_t *rounds_out);
rvseg_status rvseg_boosted_train_result(const rvseg_ctx *ctx, int32_t order, void *out, size_t out_cap, size_t *size_out);
/* The boosting round's kernels on caller-supplied weights, for parity tests (in the spirit of rvseg_extract_features):
 * error = serial sum of weights[n] over miss[n] != 0 (miss may be NULL: none); weights[n] *= exp_alpha for those;
 * weights /= their serial sum; cumsum; idx[n] = the draw of definitions 1 and 2 under round key `key`.  weights must
 * be >= +0 (neither NaN nor -0.0, whose first running sum the chain would turn into +0.0) with a positive finite sum, else RVSEG_ERR_INVALID_ARG.  Every output is optional. */
rvseg_status rvseg_boosted_resample(rvseg_ctx *ctx, const float *weights, const uint8_t *miss, int32_t N, float exp_alpha,
                                    uint64_t key, float *error_out, float *weights_out, float *cumsum_out,
                                    int32_t *idx_out);

/* ---- class-frequency-weighted split objective: DecisionTreeLearner::setUseClassFrequency (libforest learning.h:111,
 *      default true; learning.cpp:708-717).  src/train.cpp:232 switches it off for the ROVINA forests, which is what
 *      rvseg_forest_train and rvseg_boosted_train learn; every other user of the library, libforest's own example among
 *      them (example/main.cpp:92-104), gets it on.  Single-layer learners only: the reference refuses the weighting in
 *      its multi-layer learner (learning.cpp:498-501) and train.cpp does not use it, so the multi-layer and the frames
 *      entry points are not extended.
 *   Build-owned definitions:
 *   1. Weights of a tree.  cnt_c = the sum of multiplicities of class c in the tree's data set: the set after the
 *      bootstrap when use_bootstrap is on, else the set as given; for a boosting round the round's resample, with the
 *      bootstrap on top if set.  Nb = the sum of cnt_c.  INVERSE_FREQUENCY: w_c = (float)Nb / (float)cnt_c, which is
 *      getInvertedClassFrequency on the bootstrapped storage (data.h:346-357, learning.cpp:712).  A class with
 *      cnt_c == 0 has no weight; it is never read (2).  GIVEN: w_c = weights[c], the same for every tree and round.
 *   2. Objective of one side with integer class counts n_c:
 *        M = 0.0f;        for c ascending with n_c > 0:  M += w_c * (float)n_c
 *        E = -ENTROPY(M); for c ascending with n_c > 0:  E += ENTROPY(w_c * (float)n_c)
 *      with ENTROPY and fastlog2 as in the unweighted objective, all fp32, every product rounded before it is added (no
 *      FMA).  The cut's objective is E(left) + E(right).
 *   3. Everything else is unchanged: the stop rules and min_child_split_examples read the UNWEIGHTED integer masses
 *      (learning.cpp:773, 842-843); candidates, thresholds and their guard, tie rules, the random keys, leaf histograms,
 *      node numbering and the stream are rvseg_forest_train's.  NONE runs the integer expression, not the weighted one
 *      with ones ((float)(sum of n_c) and the sum of (float)n_c differ above 2^24), so it keeps the bytes of
 *      rvseg_forest_train / rvseg_boosted_train for every input.
 *   4. What this is not: the reference's running value.  Its right-hand histogram starts from initEntropies, which
 *      reads the unweighted histogram (:279-293), and turns weighted only class by class as subOne touches them
 *      (:235-256); its weighted counts are running float sums.  The definition above is what its left-hand histogram
 *      tracks (reset, then addOne, :220-234), applied to both sides and without the drift.  The weighted objective is
 *      therefore unpinned against the reference, by nature, like the learner's random stream. */
typedef enum { RVSEG_PRIOR_NONE = 0, RVSEG_PRIOR_INVERSE_FREQUENCY = 1, RVSEG_PRIOR_GIVEN = 2 } rvseg_prior_mode;
typedef struct rvseg_class_prior {
    int32_t mode;        /* rvseg_prior_mode */
    float weights[16];   /* GIVEN: one weight per class, the first C are read */
} rvseg_class_prior;
/* rvseg_forest_train for one layer of C classes (2..16; labels: P class indices) and rvseg_boosted_train, with the
 * split objective of `prior`.  prior == NULL or mode NONE return exactly what those two return.  The trained model is
 * kept on the context in the same way, so rvseg_forest_train_result / rvseg_boosted_train_result serve both.
 * RVSEG_ERR_INVALID_ARG, with the previous model kept and rvseg_last_error naming the field: an unknown mode; GIVEN
 * with a weight among the first C that is not finite or not > 0; C outside 2..16. */
rvseg_status rvseg_forest_train_prior(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels, int32_t C,
                                      const rvseg_train_params *tp, const rvseg_class_prior *prior, void *forest_out,
                                      size_t out_cap, size_t *size_out);
rvseg_status rvseg_boosted_train_prior(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels, int32_t C,
                                       const rvseg_train_params *tp, const rvseg_class_prior *prior, void *out,
                                       size_t out_cap, size_t *size_out, float *errors_out, float *alphas_out,
                                       int32_t *rounds_out);

/* ---- forest tools: replaces libforest's tools.h (AccuracyTool, ConfusionMatrixTool, CorrelationTool; tools.cpp) and
 *      Classifier::classify on a data set, for the loaded model, and re-estimates a loaded forest's leaves.
 *      X: P x D host floats, D == rvseg_feature_length, P >= 1.  `layer` indexes the layers of the context's active
 *      mode (what rvseg_forest_info reports): a multi_layer = 0 context has one, the single-label histograms -- the head
 *      the reference's tools see; on a multi_layer = 1 context the label rule is applied to
 *      multiClassLogPosterior[layer], which is this build's extension.  C = class_counts[layer].
 *      The label rule is Classifier::classify (classifier.cpp:29-51): label 0, then index i wins iff post[i] > prob -- equal
 *      values keep the lower index, a NaN never wins and a NaN at index 0 is never beaten.
 *      Refused with RVSEG_ERR_INVALID_ARG, nothing written: layer out of range, D != the feature length, P <= 0, a label
 *      outside [0, C) (the reference indexes out of bounds there).  RVSEG_ERR_NO_FOREST: no model loaded. */
/* Replaces Classifier::classify(DataStorage) (classifier.cpp:53-62) for the loaded model, forest or boosted: the label rule
 * on the forest posterior (tree 0's leaf row += trees 1..T-1 in order, as rvseg_forest_eval).  labels_out: P. */
rvseg_status rvseg_forest_classify(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, int32_t layer, int32_t *labels_out);
/* Replaces DecisionTree::classify per tree (tools.cpp:214-218): votes_out[t * P + n] = the label rule on tree t's own
 * leaf histogram of the layer (DecisionTree::classLogPosterior).  For a boosted model these are the trees' own labels,
 * whatever their weights. */
rvseg_status rvseg_forest_classify_trees(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, int32_t layer, uint8_t *votes_out);
/* One pass over X: the forest's labels (pred_out, P), the confusion counts [true][predicted] (confusion_out, C x C;
 * tools.cpp:121-128) and per tree pair the points on which the two trees vote alike (agree_out, T x T, symmetric, P on the
 * diagonal; P minus Util::hammingDist, tools.cpp:226).  Every output is optional; labels (P) may be NULL when
 * confusion_out is NULL. */
rvseg_status rvseg_forest_measure(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels, int32_t layer,
                                  int32_t *pred_out, uint64_t *confusion_out, uint64_t *agree_out);
/* Host only, no context: the reference's float arithmetic on the counts.  accuracy = 1.0f - errors / (float)size with
 * errors the off-diagonal total as an int (AccuracyTool::measure, tools.cpp:77).  confusion_norm_out (C x C) =
 * (float)min(count, 2^24) / (int)row_total (ConfusionMatrixTool::measure, tools.cpp:126-135: the reference grows the cell
 * with "+= 1" on a float, which stops at 2^24); a true class without examples gives the reference's 0 / 0 = NaN row.
 * Both outputs are optional. */
rvseg_status rvseg_forest_tools_scores(const uint64_t *confusion, int32_t C, float *accuracy_out, float *confusion_norm_out);
/* Host only: CorrelationTool::measure (tools.cpp:226-228) per cell, 1 - (int)(P - agree) / (float)P; the diagonal is 1. */
rvseg_status rvseg_forest_tools_correlation(const uint64_t *agree, int32_t T, uint64_t P, float *corr_out);
/* Replaces DecisionTreeLearner::updateHistograms / updateMultiHistograms (learning.cpp:918-1012) on a loaded
 * RandomForest: the same trees -- features, thresholds and child links byte for byte as loaded -- with every leaf's
 * histograms re-estimated from (X, labels) as rvseg_forest_train estimates them: per leaf and (layer, class) the
 * examples that land there, each adding the inverted class frequency of its label in this set, stored as
 * log((h + smoothing) / (total + C * smoothing)).  labels: P x n_layers class indices; n_layers / class_counts must be
 * the heads the model carries: its multi layers one to one, or, for a model with only a single-label head, that one
 * layer; anything else is RVSEG_ERR_INVALID_ARG.  A single-label head beside exactly one multi layer of the same class
 * count is written from the same labels (what rvseg_forest_train writes); beside other multi layers no labels are its
 * own and it stays as loaded.  At most 16 classes per layer, as the trainer.
 * Size protocol of rvseg_forest_write_mem: *size_out receives the needed size, forest_out may be NULL to query (with
 * counts_out NULL too, nothing runs).  counts_out (optional): n_nodes_total x sumC uint32, [tree][node in stream
 * order][layers concatenated], zeros at inner nodes.  The loaded model is not replaced.  RVSEG_ERR_NO_FOREST on a
 * boosted model. */
rvseg_status rvseg_forest_refit(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels, int32_t n_layers,
                                const int32_t *class_counts, float smoothing, void *forest_out, size_t out_cap,
                                size_t *size_out, uint32_t *counts_out);

/* ---- forest pruning: replaces RandomForestPrune::prune (libforest todos.txt:310-350) and the simulated-annealing driver
 *      it is written against (mcmc.h:147-240, GeometricCoolingSchedule :272-346) for the loaded RandomForest.  A state is
 *      a list of 1 .. RVSEG_PRUNE_MAX_STATE tree indices, duplicates allowed.  X, P, D and `layer` as for the forest
 *      tools above.  The chain, in fp32 as written there: while (temperature > end) { iteration++; temperature *= alpha;
 *      inner_loops proposals; one trace row }; improvement = new energy - current energy; accepted when improvement <= 0,
 *      else when logf(u) <= -improvement / temperature; the best state is updated after every proposal and is the result.
 *      Build-owned, where the reference draws from std::random_device: step s (counted over the whole run) draws
 *      d_k = draw64(mix64(seed ^ mix64(0x7072756E)), 4 s + k) (train_host.h) for slot k = 0 move choice, 1 tree, 2
 *      position, 3 acceptance; a uniform is (float)(d >> 40) * 2^-24, an index below n is d % n.  Moves are registered in
 *      the order exchange, remove, add, those with probability > 0 only, and chosen by the probSum scan of mcmc.h:178-198
 *      (no match: the last registered).  Exchange (todos.txt:134-166): state[d_2 % |state|] = d_1 % T.  Remove (:51-93):
 *      drops entry d_2 % |state|; a one-tree state is copied.  Add (:103-129): appends d_1 % T; a state already at
 *      RVSEG_PRUNE_MAX_STATE is copied, which is this build's own rule.
 *      RVSEG_PRUNE_ERROR (PruneEnergy, todos.txt:186-226): per point the trees of the state vote in order, the label is
 *      the first whose count exceeds the running maximum (label 0 with 0 votes to start), a point whose label differs --
 *      any label outside [0, C) does -- is an error; energy = (float)min(errors, 2^24) / (float)P.  The layer may have at
 *      most 16 classes.  The votes of every tree stay on the device for the whole call and every proposal is one kernel;
 *      the host is not waited for until the last.  RVSEG_PRUNE_COVER (the second PruneEnergy, todos.txt:245-297):
 *      dist[i][j] = P - agree[i][j] (rvseg_forest_measure), energy = (float)(sum over trees j of the least dist[i][j]
 *      over the state's i) / (float)|state|; the chain then runs on the host over the T x T counts. */
#define RVSEG_PRUNE_MAX_STATE 64
typedef enum { RVSEG_PRUNE_ERROR = 0, RVSEG_PRUNE_COVER = 1 } rvseg_prune_energy;
typedef struct rvseg_prune_params {
    float start_temperature;          /* todos.txt:319 (100)                                                  */
    float end_temperature;            /* todos.txt:320 (1e-5)                                                 */
    float alpha;                      /* todos.txt:318 (0.95), in (0, 1)                                      */
    int32_t inner_loops;              /* todos.txt:314 (250)                                                  */
    float p_exchange, p_remove, p_add; /* todos.txt:324-325 (1, 0, 0): >= 0, not all zero                     */
    int32_t energy;                   /* rvseg_prune_energy; default RVSEG_PRUNE_ERROR (todos.txt:328)        */
    uint64_t seed;
} rvseg_prune_params;
typedef struct rvseg_prune_trace_row {   /* the arguments of PruneCallback::callback, todos.txt:34-44 */
    int32_t iteration;
    float temperature, energy, best_energy;
    int32_t state_size;
} rvseg_prune_trace_row;
void rvseg_prune_params_default(rvseg_prune_params *pp);
/* Host only: the temperature iterations of a schedule, counted by running its fp32 loop, and its proposals
 * (iterations x inner_loops).  RVSEG_ERR_INVALID_ARG for what rvseg_forest_prune refuses in `pp`. */
rvseg_status rvseg_prune_schedule(const rvseg_prune_params *pp, int32_t *iterations_out, int32_t *steps_out);
/* state_inout (capacity RVSEG_PRUNE_MAX_STATE) / n_state_inout: the initial state in, the best state out.  trace_out
 * (optional, trace_cap rows): one row per temperature iteration, the first trace_cap of them; n_trace_out (optional):
 * the iterations run.  step_kind_out (optional, one byte per proposal): 0 rejected, 1 accepted with improvement <= 0,
 * 2 accepted uphill.  Refused with RVSEG_ERR_INVALID_ARG, outputs untouched: a boosted model, an empty or over-long
 * state or a tree index outside [0, T), alpha outside (0, 1), inner_loops < 1, a negative or all-zero move probability,
 * a schedule of more than 2^22 proposals, a layer out of range or, for RVSEG_PRUNE_ERROR, of more than 16 classes.
 * start_temperature <= end_temperature runs no iteration and returns the initial state with its energy. */
rvseg_status rvseg_forest_prune(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels, int32_t layer,
                                const rvseg_prune_params *pp, int32_t *state_inout, int32_t *n_state_inout,
                                float *best_energy_out, rvseg_prune_trace_row *trace_out, int32_t trace_cap,
                                int32_t *n_trace_out, uint8_t *step_kind_out);
/* The energy of one state.  labels may be NULL for RVSEG_PRUNE_COVER. */
rvseg_status rvseg_forest_prune_energy(rvseg_ctx *ctx, const float *X, int32_t P, int32_t D, const int32_t *labels,
                                       int32_t layer, int32_t energy, const int32_t *state, int32_t n_state,
                                       float *energy_out);
/* The context's model becomes the forest of trees state[0 .. n_state) of the loaded one, in that order, duplicates
 * included (newForest->addTree, todos.txt:344-348); rvseg_forest_write then emits it.  At most 64 entries, the loader's
 * limit.  A refused call keeps the model. */
rvseg_status rvseg_forest_prune_apply(rvseg_ctx *ctx, const int32_t *state, int32_t n_state);

/* ---- features: replaces Features::FeatureExtractor::extract, NO_LABEL branch
 *      (include/feature_extractor.h:41-291).  Host buffers, one frame.  feat_out: capacity
 *      (H/stride+1)*(W/stride+1) x D floats; x_v / y_v same capacity.  Exists for parity tests:
 *      the production path never materialises features. */
rvseg_status rvseg_extract_features(rvseg_ctx *ctx, const uint8_t *rgb, const uint16_t *depth_mm,
                                    const float *calib, float *feat_out, int32_t *x_v, int32_t *y_v,
                                    int32_t *n_points);

/* ---- whole per-frame path: replaces the body of Segmenter::processFramesFromQueueInternalRF
 *      (src/segmenter.cpp:351-431) and, with use_dense_crf, the DenseCRF call shape of
 *      Segmenter::processMapFromQueue (src/segmenter.cpp:639-657) applied per frame.
 *      calib: n x 21 floats (HOST memory in both variants).  Any output pointer may be NULL.
 *        posteriors_out  n x sumC*H*W   RF log-posteriors (the node's `posteriors` vector)
 *        marginals_out   n x sumC*H*W   CRF marginals (only with use_dense_crf)
 *        labels_out      n x L*H*W      labels of the CRF marginals (or of the posteriors
 *                                       without CRF) under params.label_mode */
rvseg_status rvseg_segment_frames(rvseg_ctx *ctx, int32_t n_frames, const uint8_t *rgb,
                                  const uint16_t *depth_mm, const float *calib, float *posteriors_out,
                                  float *marginals_out, int8_t *labels_out);
/* Page-locks a caller buffer (hipHostRegister) / releases it.  rvseg_segment_frames recognises page-locked input and
 * output buffers (registered here, or allocated with hipHostMalloc) and lets the copy engines read / write them directly:
 * without it every output crosses the host memory twice (pinned staging, then the caller's pageable buffer), which
 * bounds a call that returns marginals -- 11 MB per frame, src/segmenter.cpp:413-434 -- at the host's memcpy rate.
 * Register once, reuse the buffers across calls (registration costs milliseconds). */
rvseg_status rvseg_host_register(void *p, size_t bytes);
rvseg_status rvseg_host_unregister(void *p);
rvseg_status rvseg_segment_frames_device(rvseg_ctx *ctx, int32_t n_frames, const uint8_t *d_rgb,
                                         const uint16_t *d_depth_mm, const float *calib,
                                         float *d_posteriors_out, float *d_marginals_out,
                                         int8_t *d_labels_out, void *hip_stream);

/* ---- external semantics: replaces Segmenter::processFramesFromQueueExternal (src/segmenter.cpp:445-514), the second
 *      single-frame provider (`external_semantics`, launch/semantics.launch): any per-pixel classifier -- a CNN's
 *      softmax, for instance -- reaches the frame CRF through these calls.  None of them needs a loaded forest.
 *
 * rvseg_rectify_depth: the request's `depth` image (:466-488; srv/SingleFrameSegmentation.srv, TYPE_32FC3).
 *   xyz_out  n x H x W x 3 float32: (R*Kinv)*(d*x, d*y, d) + t with d = depth_mm / 1000.0f; NaN in all three channels
 *            where d < depth_min || d > depth_max (compared in float against the arguments).  The reference hard-codes
 *            0.5 and 15.0 here (:472); they are arguments, and need not be the context's depth_min / depth_max.
 *   Products and sums are rounded one by one, left to right (row . column), like the cloud of the forest path.
 *   Geometry is the context's width / height (the stride plays no part); calib: n x 21 HOST floats in both variants. */
rvseg_status rvseg_rectify_depth(rvseg_ctx *ctx, int32_t n_frames, const uint16_t *depth_mm, const float *calib,
                                 float depth_min, float depth_max, float *xyz_out);
rvseg_status rvseg_rectify_depth_device(rvseg_ctx *ctx, int32_t n_frames, const uint16_t *d_depth_mm, const float *calib,
                                        float depth_min, float depth_max, float *d_xyz_out, void *hip_stream);
/* The layer layout of the external provider's distributions: what single_frame_segmentation_server.py:68-71 reads from
 * `color_codings`.  Limits of the forest loader: 1..8 layers, every count >= 1, sum <= 64 (else RVSEG_ERR_INVALID_ARG, and
 * the previous layout stays).  Independent of any loaded forest: rvseg_forest_load does not disturb it, and it does not
 * disturb the forest -- rvseg_segment_frames and rvseg_segment_external can alternate on one context. */
rvseg_status rvseg_external_layers_set(rvseg_ctx *ctx, int32_t n_layers, const int32_t *class_counts);
/* The frame path with the provider's `float32[] label_distribution` in the place of the forest's posteriors (:505-512):
 *   distributions  one block per frame, layers concatenated, each [y][x][class] float32 -- the layout of `posteriors`
 *                  above.  dist_stride == 1: at full resolution, H x W.  dist_stride == params.stride (> 1): at
 *                  H/stride x W/stride, for a network that predicts at reduced resolution; they are up-sampled exactly
 *                  as the forest path up-samples its low-resolution images (cv::resize INTER_LINEAR, :380-382).  Any
 *                  other value: RVSEG_ERR_INVALID_ARG.
 *   The values are used as the forest's log-posteriors are: unary energy = -value (:642).  This call never takes a
 *   logarithm: whether to supply log-probabilities (what the forest supplies) or probabilities (what the reference's
 *   placeholder server supplies) is the caller's choice, and the CRF sees exp(value) up to normalisation either way.
 *   With use_dense_crf: cloud and lattice from depth + rgb (the context's depth_min / depth_max / dcrf_*), then the mean
 *   field per layer; marginals_out n x sumC*H*W and / or labels_out n x L*H*W under params.label_mode / unknown_label.
 *   Without: labels of the (up-sampled) distributions under label_mode; marginals_out is ignored.
 *   Chunks of max_batch, page-locked buffers, the overflow contract (host entry redoes the chunk, _device reports through
 *   rvseg_poll_status), rvseg_last_schedule and rvseg_last_timing: as for rvseg_segment_frames[_device].
 *   Without a layout set (rvseg_external_layers_set): RVSEG_ERR_INVALID_ARG.  RVSEG_ERR_NO_FOREST does not occur here. */
rvseg_status rvseg_segment_external(rvseg_ctx *ctx, int32_t n_frames, const uint8_t *rgb, const uint16_t *depth_mm,
                                    const float *calib, const float *distributions, int32_t dist_stride,
                                    float *marginals_out, int8_t *labels_out);
rvseg_status rvseg_segment_external_device(rvseg_ctx *ctx, int32_t n_frames, const uint8_t *d_rgb,
                                           const uint16_t *d_depth_mm, const float *calib, const float *d_distributions,
                                           int32_t dist_stride, float *d_marginals_out, int8_t *d_labels_out,
                                           void *hip_stream);

/* Status of the asynchronous work of the last rvseg_segment_frames_device / rvseg_segment_external_device call on this context (the
 * lattice build is the only stage that can fail on the device: hash-table overflow).  wait != 0 blocks
 * until that status is known (it does NOT wait for the outputs: synchronise the stream for those);
 * wait == 0 returns RVSEG_NOT_READY while the build is still running.  RVSEG_ERR_CAPACITY: the outputs
 * of that call are invalid (the kernels after an overflow exit without writing); the context has
 * already raised its capacity, so repeating the call succeeds.  The reference has no counterpart (its
 * hash table grows in place, permutohedral.cpp:59-79). */
rvseg_status rvseg_poll_status(rvseg_ctx *ctx, int32_t wait);

/* ---- CRF: replaces  DenseCRF crf(N,C); crf.setUnaryEnergy(U); crf.addPairwiseEnergy(feat,
 *      new PottsCompatibility(w)); Q = crf.inference(iters);  (src/segmenter.cpp:641-644;
 *      densecrf.cpp:54-60,85-91,115-131) with DIAG_KERNEL + NORMALIZE_SYMMETRIC defaults
 *      (densecrf.h:59).  n_kernels > 1 covers DenseCRF2D::addPairwiseGaussian/Bilateral
 *      (densecrf.cpp:61-81): kernel k has features[k] (N x ds[k]) and Potts weight ws[k].
 *      map_out (optional): labels under label_mode / unknown_label. */
rvseg_status rvseg_crf_infer(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t d,
                             const float *unary_energy, const float *features, float potts_w,
                             int32_t iterations, float *Q_out, int8_t *map_out, int32_t label_mode,
                             int32_t unknown_label);
rvseg_status rvseg_crf_infer_multi(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t n_kernels,
                                   const int32_t *ds, const float *const *features, const float *ws,
                                   const float *unary_energy, int32_t iterations, float *Q_out,
                                   int8_t *map_out, int32_t label_mode, int32_t unknown_label);

/* Host-side feature builders of DenseCRF2D (densecrf.cpp:61-81), for rvseg_crf_infer_multi:
 *   addPairwiseGaussian(sx, sy)                 f = (x / sx, y / sy)                            out: W*H x 2
 *   addPairwiseBilateral(sx, sy, sr, sg, sb, im) f = (x / sx, y / sy, r / sr, g / sg, b / sb)    out: W*H x 5
 * im: H x W x 3 uint8 in the channel order of the caller's image.  No context, no GPU. */
rvseg_status rvseg_crf_features_gaussian(int32_t W, int32_t H, float sx, float sy, float *out);
rvseg_status rvseg_crf_features_bilateral(int32_t W, int32_t H, float sx, float sy, float sr, float sg, float sb,
                                          const uint8_t *im, float *out);

/* ---- learned DenseCRF models: any compatibility, normalisation and kernel parameters per pairwise term.
 *      Replaces  DenseCRF crf(N, C); crf.setUnaryEnergy(U); crf.addPairwiseEnergy(f_k, compat_k, kernel_type_k,
 *      normalization_k) ...; crf.setKernelParameters(p); Q = crf.inference(iters)  (densecrf.cpp:54-60,115-131,343-360),
 *      as examples/dense_learning.cpp:128-182 builds and runs a learnt model.  Per term, t = the lattice-filtered input:
 *        normalisation (pairwise.cpp:40-80; inference applies, never the transpose), n = lattice.compute(ones):
 *          SYMMETRIC  norm = (float)(1 / sqrt((double)n + 1e-20)); input and output scaled by norm
 *          BEFORE     norm = (float)(1 / ((double)n + 1e-20));     input scaled
 *          AFTER      the same norm;                               output scaled
 *          NONE       no scaling (the reference's mean norm is never read by filter, :63-80)
 *        compatibility, then tmp1 -= out in term order (densecrf.cpp:124-127):
 *          POTTS      out[c] = fl(-w * t[c])        (labelcompatibility.cpp:46-48); compat_params: w
 *          DIAGONAL   out[c] = fl(v[c] * t[c])      (:65-67); compat_params: v, C values.  Potts(w) == Diagonal(-w, .., -w)
 *          MATRIX     out[c] = sum_c' W[c][c'] t[c'] (:79-86); compat_params: m, C x C row-major; W = 0.5 (m + m^T),
 *                     elementwise in fp32
 *        kernel parameters (pairwise.cpp:116-152), applied to the term's features before the lattice is built:
 *          CONST      ignored;  DIAG  f'[j] = fl(p[j] f[j]), d values;  FULL  f'[a] = sum_b P[a][b] f[b], d x d values
 *                     column-major (P[a][b] = p[b*d + a], the resize of :147);  kernel_params == NULL: f as passed
 *                     (the constructor's initLattice(f), :110-115)
 *      Every sum is fp32 with separately rounded products and adds, starting at the index-0 product, index ascending.
 *      The reference takes these products from Eigen, whose order is not reproducible here: that parity is unpinned. */
typedef enum rvseg_norm_kind {          /* NormalizationType, pairwise.h:32-37 */
    RVSEG_NO_NORMALIZATION = 0,
    RVSEG_NORMALIZE_BEFORE = 1,
    RVSEG_NORMALIZE_AFTER = 2,
    RVSEG_NORMALIZE_SYMMETRIC = 3
} rvseg_norm_kind;
typedef enum rvseg_kernel_kind {        /* KernelType, pairwise.h:38-42 */
    RVSEG_CONST_KERNEL = 0,
    RVSEG_DIAG_KERNEL = 1,
    RVSEG_FULL_KERNEL = 2
} rvseg_kernel_kind;
typedef enum rvseg_compat_kind {        /* PottsCompatibility, DiagonalCompatibility, MatrixCompatibility (labelcompatibility.h) */
    RVSEG_COMPAT_POTTS = 0,
    RVSEG_COMPAT_DIAGONAL = 1,
    RVSEG_COMPAT_MATRIX = 2
} rvseg_compat_kind;
typedef struct rvseg_crf_term {
    int32_t d, compat, kernel_type, normalization;   /* feature dimension 1..7; rvseg_compat_kind, _kernel_kind, _norm_kind */
    const float *features;        /* N x d, point-major: host memory for rvseg_crf_infer_terms, device memory for _device */
    const float *compat_params;   /* host: POTTS 1 value, DIAGONAL C values, MATRIX C x C row-major (symmetrised here) */
    const float *kernel_params;   /* host: NULL, d values (DIAG) or d x d column-major (FULL) */
} rvseg_crf_term;
/* Host-only validation (no context, no GPU): 1 <= C <= 64, 0 <= n_terms <= 8, N > 0, 1 <= d <= 7, kinds in range,
 * features and compat_params non-NULL.  Both inference entries call it first. */
rvseg_status rvseg_crf_terms_check(int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term *terms);
/* unary_energy: N x C host (the energy; Q0 = expAndNormalize(-U), densecrf.cpp:120).  Q_out: N x C; map_out (optional):
 * labels under label_mode / unknown_label.  A lattice hash overflow is retried once at the safe capacity. */
rvseg_status rvseg_crf_infer_terms(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term *terms,
                                   const float *unary_energy, int32_t iterations, float *Q_out, int8_t *map_out,
                                   int32_t label_mode, int32_t unknown_label);
/* The same on device buffers with the contract of rvseg_crf_infer_device (unary_is_energy, d_Q_out / d_map_out, work on
 * hip_stream, one synchronisation per lattice build for the overflow retry).  Term features are device memory. */
rvseg_status rvseg_crf_infer_terms_device(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term *terms,
                                          const float *d_unary, int32_t unary_is_energy, int32_t iterations, float *d_Q_out,
                                          int8_t *d_map_out, int32_t label_mode, int32_t unknown_label, void *hip_stream);
/* LogisticUnaryEnergy::get (unary.cpp:50-52): U[i][m] = sum_k L[m][k] f[i][k] -- an energy.  L: C x K row-major, host
 * (setUnaryParameters resizes column-major, :58-63: L[m][k] = v[k*C + m]); f: N x K.  The host entry takes host f / U_out;
 * _device takes device f / d_U_out and enqueues on hip_stream. */
rvseg_status rvseg_crf_logistic_unary(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t K, const float *L, const float *f,
                                      float *U_out);
rvseg_status rvseg_crf_logistic_unary_device(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t K, const float *L,
                                             const float *d_f, float *d_U_out, void *hip_stream);

/* ---- A kept DenseCRF model: stepwise inference, energies, KL divergence (densecrf.h:77-94, densecrf.cpp:141-235).
 *      rvseg_crf_model_set builds the model of rvseg_crf_infer_terms once -- lattices, normalisers, compatibilities, the
 *      overflow retry -- and copies the unary into context memory; when it returns, the caller's feature and unary buffers
 *      are no longer referenced.  The model is the state of the context (no handle): it lives until ANY call builds a
 *      lattice on the same context (rvseg_crf_infer*, rvseg_lattice_build, the frame and local-map calls, another
 *      rvseg_crf_model_set).  A model call without a live model returns RVSEG_ERR_INVALID_ARG and rvseg_last_error names
 *      the call that replaced it.  Host entries take host pointers and synchronise; _device entries take device pointers
 *      and enqueue on hip_stream (NULL = the context's stream) -- except rvseg_crf_model_set_device, which waits for each
 *      lattice build like rvseg_crf_infer_terms_device.  Q, out: N x C point-major.
 *
 *      Definitions (fp32 with the library's pinned orders unless stated):
 *        start   Q = expAndNormalize(-U)                                             (startInference, :178-186)
 *        step    tmp = -U; per term in order tmp -= apply_k(Q); Q = expAndNormalize(tmp)   (stepInference, :187-201)
 *                start + k steps == rvseg_crf_infer_terms(iterations = k), bit for bit
 *        apply   pairwise_[term]->apply(out, Q): normalisation scale, lattice filter, compatibility; nothing subtracted
 *        energy  unary_out[i] = U[i][l_i];  pairwise_out[i] = -0.5f * apply_term(onehot(l))[i][l_i];  a label < 0 or >= C
 *                gives a zero one-hot row and 0 in both outputs (:149,:172-175);  term == -1: the terms' energies added in
 *                fp32 from 0.0f, term ascending (:159-162)
 *        kl      parts[0] = sum q log(max(q, 1e-20f)), parts[1] = sum U q, parts[2 + k] = sum q apply_k(Q): every product,
 *                the log and every add in double from the fp32 q, U and apply values; KL = the parts added in that order.
 *                Reduced in a fixed order without atomics: the same input gives the same 64 bits on every call, but the
 *                order is the device's -- against a host sum the parts agree to ~N C 2^-53 of the sum of their absolute
 *                element terms.  The reference takes `log` and its fp32 products from libm / Eigen: unpinned, like the rest
 *                of DenseCRF.
 *        trace   inference from the start; kl_out[it] = the KL sum of Q after the start (it = 0) and after iteration it, the
 *                same bits rvseg_crf_model_kl gives for that Q.  Written on the device, read back once at the end. */
rvseg_status rvseg_crf_model_set(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term *terms,
                                 const float *unary, int32_t unary_is_energy);
rvseg_status rvseg_crf_model_set_device(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t n_terms, const rvseg_crf_term *terms,
                                        const float *d_unary, int32_t unary_is_energy, void *hip_stream);
rvseg_status rvseg_crf_model_start(rvseg_ctx *ctx, float *Q_out);
rvseg_status rvseg_crf_model_start_device(rvseg_ctx *ctx, float *d_Q_out, void *hip_stream);
/* The caller need not have produced Q with this library. */
rvseg_status rvseg_crf_model_step(rvseg_ctx *ctx, float *Q_inout, int32_t n_steps);
rvseg_status rvseg_crf_model_step_device(rvseg_ctx *ctx, float *d_Q_inout, int32_t n_steps, void *hip_stream);
rvseg_status rvseg_crf_model_apply(rvseg_ctx *ctx, int32_t term, const float *Q_in, float *out);
rvseg_status rvseg_crf_model_apply_device(rvseg_ctx *ctx, int32_t term, const float *d_Q_in, float *d_out, void *hip_stream);
/* labels: N int8 (the map_out of an inference fits).  unary_out / pairwise_out: N floats each, either may be NULL. */
rvseg_status rvseg_crf_model_energy(rvseg_ctx *ctx, const int8_t *labels, int32_t term, float *unary_out, float *pairwise_out);
rvseg_status rvseg_crf_model_energy_device(rvseg_ctx *ctx, const int8_t *d_labels, int32_t term, float *d_unary_out,
                                           float *d_pairwise_out, void *hip_stream);
/* parts: 2 + n_terms doubles (entropy, unary, one per term). */
rvseg_status rvseg_crf_model_kl(rvseg_ctx *ctx, const float *Q, double *parts);
rvseg_status rvseg_crf_model_kl_device(rvseg_ctx *ctx, const float *d_Q, double *d_parts, void *hip_stream);
/* kl_out: iterations + 1 doubles.  map_out (optional): labels of the final Q under label_mode / unknown_label. */
rvseg_status rvseg_crf_model_trace(rvseg_ctx *ctx, int32_t iterations, float *Q_out, int8_t *map_out, int32_t label_mode,
                                   int32_t unknown_label, double *kl_out);
rvseg_status rvseg_crf_model_trace_device(rvseg_ctx *ctx, int32_t iterations, float *d_Q_out, int8_t *d_map_out, int32_t label_mode,
                                          int32_t unknown_label, double *d_kl_out, void *hip_stream);
/* Which model the context keeps and its shape: what a caller needs to size the arrays of the model calls and to tell its
 * own model from one that somebody else set.  serial: taken by every successful rvseg_crf_model_set[_device] from one
 * process-wide counter that starts at 1, so it never names two models, not even across contexts or a context address
 * that is reused; the in-place setters (set_compat, set_unary, set_kernel, set_logistic, set_logistic_params,
 * energy_gradient) leave it alone.  K: the kept logistic unary's feature count, 0 without one.  Per term (arrays of the
 * term limit of rvseg_crf_terms_check): the feature dimension, the count of its labelCompatibilityParameters() and of
 * its kernelParameters(); then the two totals.  Host only: it enqueues nothing, waits for nothing and allocates
 * nothing.  *out is zeroed first; without a live model the status and rvseg_last_error are those of any model call
 * (RVSEG_ERR_INVALID_ARG, naming the call that replaced the model). */
struct rvseg_crf_model_info {   /* (a struct tag only: the entry below has the name) */
    uint64_t serial;
    int32_t N, C, n_terms, K;
    int32_t d[8], compat_params[8], kernel_params[8];
    int32_t n_compat_params, n_kernel_params;
};
rvseg_status rvseg_crf_model_info(rvseg_ctx *ctx, struct rvseg_crf_model_info *out);

/* ---- Learning on the kept model: the objectives of objective.cpp:35-108 and the mean-field gradient of DenseCRF::gradient
 *      (densecrf.cpp:238-297) with respect to the unary energy, the label-compatibility parameters and the kernel
 *      parameters (the last under "Kernel-parameter gradient" below: the model keeps the per-point ranks of every term's
 *      lattice and, for DIAG and FULL kernels, a copy of the features as passed).  "The learning loop" below sets parameters in
 *      place, evaluates CRFEnergy::gradient in one call and minimises it.  Same conventions as the model calls above (host entries synchronise, _device entries enqueue
 *      on hip_stream, a stale model is RVSEG_ERR_INVALID_ARG).
 *
 *      Definitions (fp32 with the library's pinned orders unless stated):
 *        apply_transpose   pairwise_[term]->applyTranspose(out, in) (pairwise.cpp:179-183, :63-80 with transpose = true): the
 *                input scaled by norm for SYMMETRIC and AFTER, the lattice filter with the blur axes in reverse order
 *                (d .. 0), the output scaled by norm for SYMMETRIC and BEFORE, then the compatibility as in apply (a Matrix's
 *                W^T is W bit for bit: W is stored symmetrised)
 *        objective   a gt[i] outside 0 .. C-1 skips point i; d_mul_Q is N x C, 0.0f where nothing is written
 *                LOGLIKELIHOOD  QQ = max(q + robust, 1e-20f) in fp32, q = Q[i][gt_i];  d_mul_Q[i][gt_i] = (q / QQ) / (float)N,
 *                               two fp32 divisions;  value = sum of log((double)QQ) / N, each term in double
 *                HAMMING        t = fl(class_weight[gt_i] * q);  d_mul_Q[i][gt_i] = t;  value = sum of (double)t
 *                IOU            in[l] = sum of (double)Q[i][l] over gt_i == l;  un[l] = 1e-20 + sum over valid i of
 *                               (gt_i == l ? 1 : (double)Q[i][l]);  d_mul_Q[i][l] = (float)(q / (un[l] * C)) for l == gt_i,
 *                               else (float)((-q * in[l]) / ((un[l] * un[l]) * C)), in double from q = (double)Q[i][l];
 *                               value = (sum over l ascending of in[l] / un[l]) / C
 *                Every double sum is reduced in a fixed order without atomics, like the KL parts: the same input gives the
 *                same 64 bits on every call; the order is the device's own.
 *        backward   from d_mul_Q and the Q[0 .. n] of a forward pass (densecrf.cpp:258-296), with
 *                sumAndNormalize(x, q): per point s = x[0] + x[1] + .. ascending, out[c] = fl(s * q[c]) - x[c]:
 *                  b = sumAndNormalize(d_mul_Q, Q[n]);  unary_grad = b
 *                  for it = n-1 .. 0:  [compat_grad, see below, from this b and Q[it]]
 *                                      tmp1 = 0.0f; per term in order tmp1 += apply_transpose_k(b)
 *                                      b = sumAndNormalize(fl(tmp1 * Q[it]), Q[it]);  unary_grad += b
 *                unary_grad (N x C) is d value / d U.  compat_grad: doubles, the terms concatenated in the layout of
 *                labelCompatibilityParameters() (POTTS 1, DIAGONAL C, MATRIX C (C + 1) / 2 values: the upper triangle row by
 *                row).  Per it and term, with F = the term's kernel apply of Q[it] (normalisation and filter, no
 *                compatibility, pairwise.cpp:190-195) in fp32:  POTTS -sum b F;  DIAGONAL per class c, sum over i of
 *                b[i][c] F[i][c];  MATRIX g = b^T F packed as g(i,j) + (i != j ? g(j,i) : 0) for j >= i
 *                (labelcompatibility.cpp:57-61, :76-78, :101-108).  Products and sums in double from the fp32 b and F, fixed
 *                order; accumulated over it (n-1 .. 0) in double.
 *        gradient   the forward pass keeping Q[0 .. n] in context memory (the bits of start + n steps), then objective and
 *                backward: the three-call composition bit for bit.  iterations == 0 gives the unary gradient alone
 *                (compat_grad all 0).
 *        set_compat / set_unary   replace a term's compatibility parameters (as rvseg_crf_term.compat_params; the kind
 *                stays) or the unary of the live model without a lattice build; later calls equal a fresh
 *                rvseg_crf_model_set with the new values bit for bit.
 *        logistic_gradient   LogisticUnaryEnergy::gradient (unary.cpp:64-68): out[k*C + m] = sum over i of
 *                (double)g[i][m] (double)f[i][k], column-major like unaryParameters(); g: N x C (a unary_grad), f: N x K,
 *                out: C K doubles.  Fixed order.  Needs a context, not a model. */
typedef enum rvseg_objective_kind {
    RVSEG_OBJECTIVE_LOGLIKELIHOOD = 0,
    RVSEG_OBJECTIVE_HAMMING = 1,
    RVSEG_OBJECTIVE_IOU = 2
} rvseg_objective_kind;
typedef struct rvseg_crf_objective {
    int32_t kind;                /* rvseg_objective_kind */
    const int16_t *gt;           /* N labels (VectorXs); host memory for the host entries, device memory for _device */
    float robust;                /* LOGLIKELIHOOD only */
    const float *class_weight;   /* HAMMING only: C weights, host / device memory like gt */
} rvseg_crf_objective;
/* Host-only validation (no context, no GPU): kind in range, gt non-NULL, class_weight non-NULL for HAMMING, robust finite.
 * Every entry that takes an objective calls it first. */
rvseg_status rvseg_crf_objective_check(const rvseg_crf_objective *obj);
rvseg_status rvseg_crf_model_apply_transpose(rvseg_ctx *ctx, int32_t term, const float *in, float *out);
rvseg_status rvseg_crf_model_apply_transpose_device(rvseg_ctx *ctx, int32_t term, const float *d_in, float *d_out, void *hip_stream);
/* value_out: 1 double; d_mul_Q_out: N x C */
rvseg_status rvseg_crf_model_objective(rvseg_ctx *ctx, const rvseg_crf_objective *obj, const float *Q, double *value_out,
                                       float *d_mul_Q_out);
rvseg_status rvseg_crf_model_objective_device(rvseg_ctx *ctx, const rvseg_crf_objective *obj, const float *d_Q, double *d_value_out,
                                              float *d_d_mul_Q_out, void *hip_stream);
/* Q_all: (iterations + 1) x N x C, Q[0 .. n] as the forward pass produced them.  unary_grad_out (N x C floats) or
 * compat_grad_out (doubles, one per compatibility parameter) may be NULL. */
rvseg_status rvseg_crf_model_backward(rvseg_ctx *ctx, int32_t iterations, const float *Q_all, const float *d_mul_Q,
                                      float *unary_grad_out, double *compat_grad_out);
rvseg_status rvseg_crf_model_backward_device(rvseg_ctx *ctx, int32_t iterations, const float *d_Q_all, const float *d_d_mul_Q,
                                             float *d_unary_grad_out, double *d_compat_grad_out, void *hip_stream);
/* value_out: 1 double.  unary_grad_out, compat_grad_out and Q_out (N x C, Q[n]) may be NULL. */
rvseg_status rvseg_crf_model_gradient(rvseg_ctx *ctx, int32_t iterations, const rvseg_crf_objective *obj, double *value_out,
                                      float *unary_grad_out, double *compat_grad_out, float *Q_out);
rvseg_status rvseg_crf_model_gradient_device(rvseg_ctx *ctx, int32_t iterations, const rvseg_crf_objective *obj, double *d_value_out,
                                             float *d_unary_grad_out, double *d_compat_grad_out, float *d_Q_out, void *hip_stream);
/* params: host memory, consumed before the call returns (it waits for the context's stream). */
rvseg_status rvseg_crf_model_set_compat(rvseg_ctx *ctx, int32_t term, const float *params);
rvseg_status rvseg_crf_model_set_unary(rvseg_ctx *ctx, const float *unary, int32_t unary_is_energy);
rvseg_status rvseg_crf_model_set_unary_device(rvseg_ctx *ctx, const float *d_unary, int32_t unary_is_energy, void *hip_stream);
rvseg_status rvseg_crf_logistic_gradient(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t K, const float *unary_grad, const float *f,
                                         double *out);
rvseg_status rvseg_crf_logistic_gradient_device(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t K, const float *d_unary_grad,
                                                const float *d_f, double *d_out, void *hip_stream);

/* ---- Kernel-parameter gradient on the kept model: DenseCRF::gradient's kernel_grad (densecrf.cpp:238-297) with what is
 *      underneath it -- Permutohedral::gradient (permutohedral.cpp:611-695), DenseKernel::featureGradient / gradient
 *      (pairwise.cpp:82-114, :152-163), PairwisePotential::kernelGradient (:202-207).  a, b: N x C point-major, C the
 *      model's class count.  Conventions and argument rules of the learning calls above (stale model, term out of range and
 *      NULL a / b are RVSEG_ERR_INVALID_ARG).
 *
 *      Definitions (fp32, one rounding per operation written, unless stated):
 *        lattice_gradient   df (N x d) = Permutohedral::gradient(a, b), the reference's formula, with respect to the lattice
 *                features.  With K the term's unnormalised lattice filter it is the exact derivative of b^T K a = a^T K^T b
 *                (K^T: the blur axes in reverse); it equals that of a^T K b only for d = 1, where the two blurs commute, and
 *                featureGradient's normalised kinds below, which mix K and K^T, are the derivative of neither form for
 *                d > 1 (DESIGN section 16 has the measured deviations).  The formula is the contract.  Two
 *                passes, dir = 0, 1:  the ordered splat of a (dir 0) or b (dir 1) -- per vertex, points ascending, each
 *                product rounded; the blur (float)((double)o + 0.5 * (double)(n1 + n2)) over the axes 0 .. d (dir 0) or
 *                d .. 0 (dir 1); then per point i with x = b (dir 0) or a (dir 1), alpha = 1.0f / (1 + powf(2, -d)) / (d + 1),
 *                sf = the lattice's scale factors (permutohedral.cpp:623-625), o(r) the point's vertex of remainder r:
 *                  for j = 0 .. d:  r0 = d - rank[j], r1 = r0 + 1 > d ? 0 : r0 + 1,
 *                                   ra[j][k] = fl(alpha * values[o(r0)][k]) - fl(alpha * values[o(r1)][k])
 *                  sm[k] = ra[0][k]
 *                  for j = 1 .. d:  v = fl(sf[j-1] * fl(sm[k] - fl(j * ra[j][k]))),  grad_j = grad_j + fl(x[i][k] * v) over k
 *                                   ascending from 0.0f, then sm[k] += ra[j][k]
 *                  df[i][j-1] = grad (dir 0), fl(df[i][j-1] + grad) (dir 1)
 *                rank: the d+1 ranks of the point (permutohedral.cpp:223-242), computed with the arithmetic of the lattice
 *                build from the features the lattice was built from (after the kernel parameters).
 *        lbl_Q   compat_apply: compatibility(Q) with no filter (pairwise.cpp:203-205): POTTS fl(-w q), DIAGONAL fl(v[c] q),
 *                MATRIX sum_c' W[c][c'] q[c'] from c' = 0 up, each product and add rounded
 *        featureGradient   fg (N x d), by the term's normalisation; n = the term's norm, K the unnormalised lattice filter
 *                with the blur apply uses for C, K^T the same with the blur axes in reverse, G = lattice_gradient:
 *                  NONE       fg = G(a, b)
 *                  SYMMETRIC  fa = K^T(a n), fb = K(b n), X = fl(fl(0.5f * fl(fl(a fb) + fl(fa b))) * fl(fl(n n) n)),
 *                             fg = fl(G(a n, b n) - G(X, 1))
 *                  AFTER      fb = K(b), X = fl(fl(a fb) * fl(n n)), fg = fl(G(a n, b) - G(X, 1))
 *                  BEFORE     fa = K^T(a), X = fl(fl(fa b) * fl(n n)), fg = fl(G(a, b n) - G(X, 1))
 *        kernel_gradient   DenseKernel::gradient(a, b): CONST 0 values; FULL grad[b*d + a] = sum over i of
 *                (double)fg[i][a] (double)f[i][b], d x d column-major like kernelParameters(); DIAG its diagonal, d values.
 *                f: the features as passed to rvseg_crf_model_set (before the kernel parameters).  Products and sums in double,
 *                reduced in the fixed order of rvseg_crf_logistic_gradient: the same input gives the same 64 bits on every
 *                call.  fg_out (optional, N x d) receives featureGradient for every kernel type.
 *        backward_kernel / gradient_kernel   _backward / _gradient with kernel_grad_out: doubles, the terms concatenated
 *                in the layout of kernelParameters().  Per it = n-1 .. 0 and per term, kernel_gradient(b, lbl_Q(Q[it])) is
 *                accumulated in double, from the same b the compatibility gradient uses.  iterations == 0 gives zeros.  With
 *                kernel_grad_out == NULL they equal _backward / _gradient bit for bit (which are these calls with NULL). */
/* Q, out: N x C */
rvseg_status rvseg_crf_model_compat_apply(rvseg_ctx *ctx, int32_t term, const float *Q, float *out);
rvseg_status rvseg_crf_model_compat_apply_device(rvseg_ctx *ctx, int32_t term, const float *d_Q, float *d_out, void *hip_stream);
/* df_out: N x d floats, d the term's feature dimension */
rvseg_status rvseg_crf_model_lattice_gradient(rvseg_ctx *ctx, int32_t term, const float *a, const float *b, float *df_out);
rvseg_status rvseg_crf_model_lattice_gradient_device(rvseg_ctx *ctx, int32_t term, const float *d_a, const float *d_b, float *d_df_out,
                                                     void *hip_stream);
/* grad_out: doubles (CONST 0, DIAG d, FULL d x d), may be NULL;  fg_out: N x d floats, may be NULL */
rvseg_status rvseg_crf_model_kernel_gradient(rvseg_ctx *ctx, int32_t term, const float *a, const float *b, double *grad_out,
                                             float *fg_out);
rvseg_status rvseg_crf_model_kernel_gradient_device(rvseg_ctx *ctx, int32_t term, const float *d_a, const float *d_b,
                                                    double *d_grad_out, float *d_fg_out, void *hip_stream);
rvseg_status rvseg_crf_model_backward_kernel(rvseg_ctx *ctx, int32_t iterations, const float *Q_all, const float *d_mul_Q,
                                             float *unary_grad_out, double *compat_grad_out, double *kernel_grad_out);
rvseg_status rvseg_crf_model_backward_kernel_device(rvseg_ctx *ctx, int32_t iterations, const float *d_Q_all, const float *d_d_mul_Q,
                                                    float *d_unary_grad_out, double *d_compat_grad_out, double *d_kernel_grad_out,
                                                    void *hip_stream);
rvseg_status rvseg_crf_model_gradient_kernel(rvseg_ctx *ctx, int32_t iterations, const rvseg_crf_objective *obj, double *value_out,
                                             float *unary_grad_out, double *compat_grad_out, double *kernel_grad_out, float *Q_out);
rvseg_status rvseg_crf_model_gradient_kernel_device(rvseg_ctx *ctx, int32_t iterations, const rvseg_crf_objective *obj,
                                                    double *d_value_out, float *d_unary_grad_out, double *d_compat_grad_out,
                                                    double *d_kernel_grad_out, float *d_Q_out, void *hip_stream);

/* ---- The learning loop on the kept model: the parameters of examples/dense_learning.cpp:126-182 changed in place, its
 *      EnergyFunction (:38-85) as one entry, and a minimiser.  Conventions of the learning calls above: a stale model, a
 *      term out of range and a NULL array that is not optional are RVSEG_ERR_INVALID_ARG; host entries synchronise.
 *
 *      Definitions:
 *        set_kernel   replaces the kernel parameters of a DIAG (d values) or FULL (d x d, column-major) term: that term's
 *                lattice, normaliser and point ranks are rebuilt from the features the model keeps; nothing is uploaded but
 *                the parameters, and no other term, the unary or the compatibilities are touched.  params == NULL: the
 *                features as passed.  A CONST term is RVSEG_ERR_INVALID_ARG.  A hash overflow rebuilds this term once at the
 *                capacity that cannot overflow.  The model stays live; afterwards every model call equals a fresh
 *                rvseg_crf_model_set with these kernel_params bit for bit (vertex numbering and capacity do not show).
 *        set_logistic   the model copies f (N x K) and L (C x K row-major, host memory always) and its unary becomes the
 *                energy U = L f of rvseg_crf_logistic_unary, computed into the model's memory: the bits of that call followed
 *                by rvseg_crf_model_set_unary.  Limits of rvseg_crf_logistic_unary (K >= 1).  set_logistic_params: U again
 *                from a new L and the kept f; RVSEG_ERR_INVALID_ARG without a kept logistic unary.  rvseg_crf_model_set,
 *                _set_unary and _set_unary_device drop the kept f.
 *        gradient_params   rvseg_crf_model_gradient_kernel with rvseg_crf_logistic_gradient applied on the device to its
 *                unary gradient and the kept f: unary_grad_out is C K doubles, column-major like unaryParameters(), and must
 *                be NULL on a model without a kept logistic unary.  The two-call composition bit for bit; only the
 *                parameters' doubles are read back.
 *        energy_gradient   CRFEnergy::gradient (dense_learning.cpp:60-84).  learn_mask: 1 unary, 2 pairwise, 4 kernel.  x: the
 *                learned groups in the order unaryParameters() (C K values, column-major; none without a kept logistic
 *                unary) | labelCompatibilityParameters() (per term POTTS 1, DIAGONAL C, MATRIX the C (C + 1) / 2 values of the
 *                upper triangle row by row, W[i][j] = W[j][i] = v) | kernelParameters() (per term CONST 0, DIAG d, FULL d x d);
 *                n must be their count.  Each learned group is set in place (set_logistic_params; set_compat per term;
 *                set_kernel per DIAG / FULL term whose values differ bitwise from those its lattice was built from -- a
 *                lattice built from NULL parameters differs from any values), then gradient_params runs with the outputs of
 *                the groups that are not learned NULL.  With g the gradients in the order of x:
 *                  dx[i] = -(float)g[i];  when l2_norm > 0:  dx[i] = fl(dx[i] + fl(l2_norm * x[i])) in fp32
 *                  value = -objective;    when l2_norm > 0:  value += (0.5 * (double)l2_norm) * S,  S = sum of
 *                                                            (double)x[i] * (double)x[i] from i = 0 up, in double
 *        The minimiser   rvseg_minimize_lbfgs: limited-memory BFGS in double on the host (no context, no GPU), the project's
 *                own and pinned to no other implementation.  From x with f, g = energy(x): stop at once when
 *                ||g|| / max(1, ||x||) < epsilon.  Direction d = -H g by the two-loop recursion over the last m pairs
 *                (s = x' - x, y = g' - g; a pair with s.y <= 0 is left out; H0 = (s.y / y.y) I of the newest pair); the first
 *                direction, and any that is not a descent direction, is -g with the history dropped.  Line search: t = 1 / ||g||
 *                for a -g direction, else 1, clamped to [min_step, max_step], halved until the Armijo condition
 *                f(x + t d) <= f(x) + ftol t g.d holds; at most max_linesearch evaluations, t never below min_step.  After
 *                every accepted step: the progress callback (k = iterations so far from 1, ls = evaluations of this line
 *                search; a non-zero return stops), the convergence test, then max_iterations (0: no limit).  A failed line
 *                search returns the best point evaluated, which is never worse than the start.  A value or gradient that is
 *                not finite ends the run with RVSEG_ERR_INVALID_ARG and x at the best finite point (x unchanged when the
 *                first evaluation is the one).  Every other end returns RVSEG_OK; rvseg_lbfgs_report.status tells which. */
rvseg_status rvseg_crf_model_set_kernel(rvseg_ctx *ctx, int32_t term, const float *params);
/* f: N x K (host / device); L: C x K row-major, host memory, copied before the call returns (the _device entry only enqueues) */
rvseg_status rvseg_crf_model_set_logistic(rvseg_ctx *ctx, int32_t K, const float *L, const float *f);
rvseg_status rvseg_crf_model_set_logistic_device(rvseg_ctx *ctx, int32_t K, const float *L, const float *d_f, void *hip_stream);
rvseg_status rvseg_crf_model_set_logistic_params(rvseg_ctx *ctx, const float *L);
/* value_out: 1 double.  unary_grad_out (C K doubles), compat_grad_out and kernel_grad_out may be NULL. */
rvseg_status rvseg_crf_model_gradient_params(rvseg_ctx *ctx, int32_t iterations, const rvseg_crf_objective *obj, double *value_out,
                                             double *unary_grad_out, double *compat_grad_out, double *kernel_grad_out);
rvseg_status rvseg_crf_model_gradient_params_device(rvseg_ctx *ctx, int32_t iterations, const rvseg_crf_objective *obj,
                                                    double *d_value_out, double *d_unary_grad_out, double *d_compat_grad_out,
                                                    double *d_kernel_grad_out, void *hip_stream);
/* obj, x, value_out, dx_out: host memory; x and dx_out hold n floats */
rvseg_status rvseg_crf_model_energy_gradient(rvseg_ctx *ctx, int32_t iterations, const rvseg_crf_objective *obj, int32_t learn_mask,
                                             float l2_norm, const float *x, int32_t n, double *value_out, float *dx_out);

typedef enum rvseg_lbfgs_status {
    RVSEG_LBFGS_CONVERGED = 0,            /* ||g|| / max(1, ||x||) < epsilon                         */
    RVSEG_LBFGS_MAX_ITERATIONS = 1,
    RVSEG_LBFGS_STOPPED = 2,              /* the progress callback returned non-zero                 */
    RVSEG_LBFGS_LINESEARCH_FAILED = 3,    /* no step satisfied the Armijo condition                  */
    RVSEG_LBFGS_NOT_FINITE = -1,          /* the energy returned a value or gradient that is not finite */
    RVSEG_LBFGS_BAD_ARGUMENTS = -2
} rvseg_lbfgs_status;
typedef struct rvseg_lbfgs_params {
    int32_t m;                /* corrections kept: 6                   */
    int32_t max_iterations;   /* 0: no limit                           */
    int32_t max_linesearch;   /* evaluations per line search: 20       */
    int32_t reserved;
    double epsilon;           /* 1e-5                                  */
    double ftol;              /* Armijo constant: 1e-4                 */
    double min_step;          /* 1e-20                                 */
    double max_step;          /* 1e20                                  */
} rvseg_lbfgs_params;
typedef struct rvseg_lbfgs_report {
    int32_t status;           /* rvseg_lbfgs_status                    */
    int32_t iterations;       /* accepted steps                        */
    int32_t evaluations;      /* calls of the energy                   */
    int32_t reserved;
    double gnorm, xnorm;      /* at the point returned (gnorm: at the last accepted point) */
} rvseg_lbfgs_report;
/* returns f(x) and writes its gradient into g (n doubles) */
typedef double (*rvseg_energy_fn)(void *user, const double *x, double *g, int32_t n);
typedef int32_t (*rvseg_progress_fn)(void *user, const double *x, const double *g, double fx, double xnorm, double gnorm, double step,
                                     int32_t n, int32_t k, int32_t ls);
void rvseg_lbfgs_params_default(rvseg_lbfgs_params *p);
/* x: n doubles, start in, result out.  fx_out, progress, params (defaults) and report_out may be NULL. */
rvseg_status rvseg_minimize_lbfgs(int32_t n, double *x, double *fx_out, rvseg_energy_fn energy, rvseg_progress_fn progress, void *user,
                                  const rvseg_lbfgs_params *params, rvseg_lbfgs_report *report_out);

/* ---- lattice introspection for parity tests: Permutohedral::init + compute
 *      (densecrf permutohedral.cpp:140-321,596-603).  offsets_out / bary_out: N x (d+1);
 *      keys_out: capacity M_cap x d int16; vertex numbering is arbitrary (results do not depend on
 *      it); M_out receives the number of lattice vertices. */
rvseg_status rvseg_lattice_build(rvseg_ctx *ctx, const float *features, int32_t N, int32_t d,
                                 int32_t *offsets_out, float *bary_out, int16_t *keys_out,
                                 int32_t keys_capacity, int32_t *M_out);
/* filter one value matrix (N x C) through the lattice last built on this ctx */
rvseg_status rvseg_lattice_filter(rvseg_ctx *ctx, const float *in, int32_t C, float *out);
/* blur neighbours of the lattice last built (permutohedral.cpp:296-318): n1_out / n2_out are
 * (d+1) x M vertex ids (-1 = absent), in this ctx's vertex numbering.  Optional: the vertex-major
 * entry order used by the ordered splat: csr_point (N*(d+1)), vstart / vend (M). */
rvseg_status rvseg_lattice_neighbours(rvseg_ctx *ctx, int32_t *n1_out, int32_t *n2_out, uint32_t *csr_point,
                                      uint32_t *vstart, uint32_t *vend);

/* Local-map fusion -- replaces the accumulation loop of Segmenter::processMapFromQueue,
 * src/segmenter.cpp:561-616:  unaries[l](c, index) += label_distribution[off_l + pixel*C_l + c]
 * for every image in call order, pixels in raster order (the order fixes the fp32 sums).
 *   index_images  n_images x H x W int32, the projector's IndexImage rows of one camera
 *                 (index_image.ptr<int>(y + i*_camera_h), :601): cloud point seen at the pixel, < 0 = none
 *   posteriors    n_images x (sum C_l * H * W) floats, each image in the layout rvseg_segment_frames
 *                 writes ([layer][y][x][class], segmenter.cpp:413-431)
 *   unaries_out   layers concatenated; layer l is cloud_size x C_l, point-major (== the C_l x cloud_size
 *                 column-major Eigen matrix of :563-567), starting at cloud_size * (C_0 + .. + C_{l-1})
 * H, W are the context's.  An index >= cloud_size is RVSEG_ERR_INVALID_ARG (the reference writes out of
 * bounds).  Feed -unaries_out[l] to rvseg_crf_infer (:642) or label it with the no-CRF rule (:660-681). */
rvseg_status rvseg_fuse_posteriors(rvseg_ctx *ctx, int32_t n_images, const int32_t *index_images,
                                   const float *posteriors, int32_t n_layers, const int32_t *class_counts,
                                   int32_t cloud_size, float *unaries_out);

/* ---- the same consumers with every buffer resident in HBM (device pointers, work enqueued on hip_stream,
 *      no synchronisation, no allocation per call once the context's buffers have grown): the local-map
 *      thread can take d_posteriors_out of rvseg_segment_frames_device as it is, instead of moving
 *      11-21 MB per frame over PCIe twice.  An index >= cloud_size is skipped like "no point" and reported
 *      by rvseg_poll_status (RVSEG_ERR_INVALID_ARG). */
rvseg_status rvseg_fuse_posteriors_device(rvseg_ctx *ctx, int32_t n_images, const int32_t *d_index_images,
                                          const float *d_posteriors, int32_t n_layers, const int32_t *class_counts,
                                          int32_t cloud_size, float *d_unaries_out, void *hip_stream);
/* pairwise = (x,y,z) * dcrf_xyz_kernel ++ (r,g,b) * dcrf_rgb_kernel per point, rgb in [0,1]
 * (src/segmenter.cpp:629-637).  d_features_out: N x 6. */
rvseg_status rvseg_cloud_features_device(rvseg_ctx *ctx, int32_t N, const float *d_xyz, const float *d_rgb,
                                         float *d_features_out, void *hip_stream);
/* DenseCRF call shape of src/segmenter.cpp:641-644 on device buffers, one Potts kernel.  unary_is_energy = 0:
 * d_unary holds the accumulated log-posteriors and the energy is their negative (crf.setUnaryEnergy(-unaries[l]),
 * :642) -- no negated copy is made.  d_Q_out or d_map_out may be NULL (not both).  The lattice build reads
 * its counters back once (one synchronisation of hip_stream) so that a hash overflow is retried here. */
rvseg_status rvseg_crf_infer_device(rvseg_ctx *ctx, int32_t N, int32_t C, int32_t d, const float *d_unary,
                                    int32_t unary_is_energy, const float *d_features, float potts_w,
                                    int32_t iterations, float *d_Q_out, int8_t *d_map_out, int32_t label_mode,
                                    int32_t unknown_label, void *hip_stream);
rvseg_status rvseg_label_values_device(rvseg_ctx *ctx, const float *d_values, int32_t N, int32_t C,
                                       int32_t label_mode, int32_t unknown_label, int8_t *d_labels_out,
                                       void *hip_stream);
/* Replaces the body of Segmenter::processMapFromQueue for one local map (src/segmenter.cpp:561-682) with
 * everything in HBM: fusion through the index images (:561-616), then per label layer of the loaded model
 * either the cloud DenseCRF + "> 2.0/C else Unknown" (params.use_dense_crf, :628-658; one lattice serves all
 * layers -- the reference builds the same one per layer) or the no-CRF rule (:660-681).
 *   d_labels_out   L x cloud_size int8 (result_labels[layer][i], :646-657)
 *   d_unaries_out  optional: the fused unaries, layers concatenated (else they stay in context memory) */
rvseg_status rvseg_process_map_device(rvseg_ctx *ctx, int32_t n_images, const int32_t *d_index_images,
                                      const float *d_posteriors, int32_t cloud_size, const float *d_cloud_xyz,
                                      const float *d_cloud_rgb, int8_t *d_labels_out, float *d_unaries_out,
                                      void *hip_stream);

/* ---- the projector: index images from poses (src/segmenter.cpp:234-240, 576-578) -----------------------------
 * _projector.project(zbuffer, index_image, m_multi->transform().inverse(), *cloud), set up by initializeProjector
 * from the cameras' intrinsics, the image size, depth_min and depth_max.  fps_mapper::MultiProjector is not in the
 * reference tree, so the projection is a BUILD-OWNED definition (parity with fps_mapper is unpinned):
 *
 * Inputs: a cloud of N points, xyz fp32 in the map frame.  For each of the n_images sub-images (one camera of one
 * node, in the order the fusion uses), one projection matrix P: 3x4, fp32, row-major, mapping the map frame to
 * homogeneous pixels, K * [R | t] of that view.  W, H, depth_min, depth_max are the context's (rvseg_params;
 * setImageSize / setMinDistance / setMaxDistance, :237-240).  depth_min must be > 0, otherwise the call returns
 * RVSEG_ERR_INVALID_ARG.
 *
 * Per point i and image m, all in fp32, every product and sum rounded separately (no FMA):
 *     px = ((P00*x + P01*y) + P02*z) + P03      (same shape for py with row 1, w with row 2)
 *     keep only if  w >= depth_min && w <= depth_max     (NaN fails both tests: skipped)
 *     u = px / w ; v = py / w                    (IEEE division)
 *     cu = rintf(u) ; cv = rintf(v)              (nearest, ties to even)
 *     keep only if  cu >= 0 && cu < W && cv >= 0 && cv < H   (tested on the floats, then converted; -0.0 is
 *                                                             column / row 0)
 * A pixel's winner is the kept point with the smallest w.  Among equal w, the smallest index wins.  This is exactly
 * what the sequential loop "if (z < zbuffer(r,c)) { zbuffer = z; index = i; }" over ascending i produces, so the
 * result does not depend on any execution order.
 *
 * Outputs: index (int32, n_images x H x W) holds the winner, or -1 where no point lands -- the convention the
 * fusion reads (:601-607).  The optional zbuffer (fp32, same shape) holds the winner's w, or +inf where no point
 * lands.
 *
 * The same call limit as the fusion applies: n_images * W * H < 2^32 - 1.  N == 0 or n_images == 0 is not an error
 * (the output is all -1).  `proj` is HOST memory (n_images x 12 floats) in both entries; it is consumed before the
 * call returns. */
/* (segmenter.cpp:234-240, 576-578) device buffers, work enqueued on hip_stream, no synchronisation, no allocation per
 * call once the context's key image has grown (at most 32 x W x H x 8 bytes: larger calls run in groups of 32 images) */
rvseg_status rvseg_project_cloud_device(rvseg_ctx *ctx, int32_t n_images, const float *proj, int32_t N,
                                        const float *d_cloud_xyz, int32_t *d_index_out, float *d_zbuffer_out,
                                        void *hip_stream);
/* (segmenter.cpp:234-240, 576-578) host buffers, staged through context memory, synchronous; zbuffer_out may be NULL */
rvseg_status rvseg_project_cloud(rvseg_ctx *ctx, int32_t n_images, const float *proj, int32_t N,
                                 const float *cloud_xyz, int32_t *index_out, float *zbuffer_out);
/* (segmenter.cpp:234-240, 576-578, then :561-682) rvseg_process_map_device with the index images produced in context
 * memory by the projector instead of passed in: the same fusion, CRF and labels through the same internal function.
 * d_cloud_xyz is needed with or without use_dense_crf.  d_index_out (optional, n_images x H x W int32) receives
 * the index images. */
rvseg_status rvseg_process_map_poses_device(rvseg_ctx *ctx, int32_t n_images, const float *proj,
                                            const float *d_posteriors, int32_t cloud_size, const float *d_cloud_xyz,
                                            const float *d_cloud_rgb, int8_t *d_labels_out, float *d_unaries_out,
                                            int32_t *d_index_out, void *hip_stream);
/* (segmenter.cpp:234-240, 576-578) Host only, no context: P = K * [R_c^T | -R_c^T t_c] * T^-1 for one camera
 * (calib_R_t: the extrinsic camera -> base link, R row-major then t, floats 9..20 of a calibration) and one node pose
 * T (base link -> map, 3x4 row-major [R_n | t_n], rotation assumed orthonormal, so T^-1 = [R_n^T | -R_n^T t_n]).
 * Computed in double in this order, every dot product summed left to right ((a0*b0 + a1*b1) + a2*b2):
 *     A = R_c^T * R_n^T ;  b = R_n^T * t_n ;  c = R_c^T * (b + t_c)  (so the view is [A | -c]) ;
 *     P[r][j] = K[r] . A[:, j]  (j < 3) ;  P[r][3] = -(K[r] . c) ;  each of the 12 values rounded to fp32 once.
 * A convenience: the projector's contract starts at P. */
rvseg_status rvseg_projection_matrix(const float K[9], const float calib_R_t[12], const float node_pose[12],
                                     float P_out[12]);

/* One of the label rules above over a host matrix of N points x C classes (class-contiguous); the
 * no-CRF branch of processMapFromQueue applies RVSEG_LABEL_NOCRF to the fused unaries
 * (src/segmenter.cpp:660-681). */
rvseg_status rvseg_label_values(rvseg_ctx *ctx, const float *values, int32_t N, int32_t C, int32_t label_mode,
                                int32_t unknown_label, int8_t *labels_out);

/* ---- multi-GPU: the local-map gather over RCCL.  The reference is a single process; the build
 *      shards key frames over the GPUs of a node (one context per GPU, each in its own process or thread, no
 *      data-path collective) and sends every rank's fixed-size block -- int8 labels n x L x H x W, or fp32
 *      posteriors for the order-preserving fusion of src/segmenter.cpp:599-616 -- to the fusion rank: one
 *      direct transfer per peer over xGMI.  librccl.so is opened on first use.
 *        rvseg_comm_unique_id  rank 0 creates the 128-byte id; the host distributes it (any channel)
 *        rvseg_comm_init       collective over all ranks (ncclCommInitRank)
 *        rvseg_gather_frames   rank r's bytes_per_rank bytes land at d_recv + r * bytes_per_rank on `root`
 *                              (d_recv is ignored elsewhere); enqueued on hip_stream, not waited for */
#define RVSEG_COMM_ID_BYTES 128
rvseg_status rvseg_comm_unique_id(uint8_t id_out[RVSEG_COMM_ID_BYTES]);
rvseg_status rvseg_comm_init(rvseg_ctx *ctx, int32_t rank, int32_t world, const uint8_t id[RVSEG_COMM_ID_BYTES]);
void rvseg_comm_destroy(rvseg_ctx *ctx);
rvseg_status rvseg_gather_frames(rvseg_ctx *ctx, const void *d_local, size_t bytes_per_rank, void *d_recv,
                                 int32_t root, void *hip_stream);

/* ---- scoring: replaces RgbLabelConversion (include/rgb_label_conversion.h) and the confusion / score block of
 *      src/test.cpp:182-228 and src/test_multi.cpp:222-268.  L and C_l are the loaded model's (rvseg_forest_info);
 *      every call below except rvseg_eval_scores_from_counts needs a loaded model (else RVSEG_ERR_INVALID_ARG), and
 *      rvseg_forest_load discards colour codings and counters.  Label images are the layout of labels_out above:
 *      n x L x H x W int8 (layer < 0), or n x H x W of one layer (layer >= 0); RGB8 images add a trailing R, G, B byte
 *      triple per pixel -- the bytes of the PNG the reference reads or writes (it swaps to BGR and back,
 *      rgb_label_conversion.h:47-49,67-69,80-88, test.cpp:199).
 *
 * Colour coding of one layer: n entries (n <= 256, else RVSEG_ERR_CAPACITY) in config.json's color_codings[l].coding
 * order, rgb n x 3 and labels n, negative labels included (Void = -1, Other = -2).  Replaces the RgbLabelConversion
 * constructor (rgb_label_conversion.h:20-39):
 *   decode  a colour maps to the label of the LAST entry with that colour; a colour not in the table maps to
 *           missing_label.  The reference's std::map::operator[] gives 0 there (:86-88): pass 0 for its behaviour,
 *           -1 to leave unknown colours unscored.
 *   encode  a label maps to the colour of the LAST entry with that label; a label not in the table to (0, 0, 0) (:80-84). */
rvseg_status rvseg_color_coding_set(rvseg_ctx *ctx, int32_t layer, int32_t n, const uint8_t *rgb, const int8_t *labels,
                                    int8_t missing_label);
/* RgbLabelConversion::rgbToLabel / labelToRgb (rgb_label_conversion.h:42-78) over n_images label images.  _device:
 * device buffers, enqueued on hip_stream, not waited for.  Host variants stage through the context's stream. */
rvseg_status rvseg_labels_from_rgb_device(rvseg_ctx *ctx, int32_t layer, int32_t n_images, const uint8_t *d_rgb,
                                          int8_t *d_labels, void *hip_stream);
rvseg_status rvseg_labels_to_rgb_device(rvseg_ctx *ctx, int32_t layer, int32_t n_images, const int8_t *d_labels,
                                        uint8_t *d_rgb, void *hip_stream);
rvseg_status rvseg_labels_from_rgb(rvseg_ctx *ctx, int32_t layer, int32_t n_images, const uint8_t *rgb, int8_t *labels);
rvseg_status rvseg_labels_to_rgb(rvseg_ctx *ctx, int32_t layer, int32_t n_images, const int8_t *labels, uint8_t *rgb);

/* Confusion matrix per layer, uint64 counts on the device (the reference's int counters overflow after ~7 000 VGA
 * frames).  The accumulate calls replace the counting loop of test.cpp:186-195 (test_multi.cpp:222-233) over every
 * full-resolution pixel of every layer: count[gt][pred] += 1 where pred >= 0 and gt >= 0.  A pair with pred >= C_l or
 * gt >= C_l (the reference indexes past its arrays) goes to the layer's out-of-range counter instead.
 *   d_pred   n_frames x L x H x W int8: labels_out of rvseg_segment_frames[_device] as it is.  test.cpp scores
 *            multi_layer = 0, fill_value = -1000, RVSEG_LABEL_EVAL, no CRF, stride 2 (its "/2" is hard-coded,
 *            :141,152); test_multi.cpp the same with multi_layer = 1 at the configured stride
 *   d_gt     RVSEG_GT_LABELS: n_frames x L x H x W int8; RVSEG_GT_RGB: the colour-coded images (x 3 bytes), decoded on
 *            the fly through each layer's colour coding (no int8 image is written)
 * _device: enqueued on hip_stream (NULL = the context's stream, as for rvseg_segment_frames_device) without
 * synchronising; the context records an event there, and
 * rvseg_eval_confusion waits for it, so segment_frames_device -> eval_accumulate_device can share one stream with no
 * host synchronisation in between.  Counts are integers: the result does not depend on the order of the work. */
typedef enum rvseg_gt_format {
    RVSEG_GT_LABELS = 0,
    RVSEG_GT_RGB = 1
} rvseg_gt_format;
rvseg_status rvseg_eval_reset(rvseg_ctx *ctx);
rvseg_status rvseg_eval_accumulate_device(rvseg_ctx *ctx, int32_t n_frames, const int8_t *d_pred, const void *d_gt,
                                          int32_t gt_format, void *hip_stream);
rvseg_status rvseg_eval_accumulate(rvseg_ctx *ctx, int32_t n_frames, const int8_t *pred, const void *gt,
                                   int32_t gt_format);
/* Counts of one layer since the last reset: counts_out C_l x C_l, row = ground truth, column = prediction
 * (label_count of test.cpp:186-195).  Either output may be NULL. */
rvseg_status rvseg_eval_confusion(rvseg_ctx *ctx, int32_t layer, uint64_t *counts_out, uint64_t *out_of_range);
/* The scores of test.cpp:203-228 from a C x C count matrix, in the reference's types and order: float accumulators
 * of double expressions over static_cast<float>(count), divisors converted to double, C counting every class (empty
 * ones included).  global_acc = 100.0 * (float)sum(diag) / total (NaN when total == 0, as in the reference);
 * class_avg_acc and iou as printed at :226-227; row_pct_out (optional, C x C) = the printed table,
 * 100.0 * (float)count / row total (row total 0 -> 1).  Host only: no context, no GPU. */
rvseg_status rvseg_eval_scores_from_counts(const uint64_t *counts, int32_t C, double *global_acc, float *class_avg_acc,
                                           float *iou, double *row_pct_out);

/* ---- launch schedules.  The library picks the schedule of the ordered splat (the dominant kernel) and the stream
 *      overlaps from the shape of the work; this block overrides those choices for tests, profiling and tuning.
 *      Nothing on the call path reads the environment.  The reference has no counterpart (single thread). */
typedef struct rvseg_schedule {
    int32_t splat;               /* 0 = chosen from the chunk (default), 1 = list-major walk, 2 = resident bands
                                    (forced wherever its tables fit)                                              */
    int32_t resident_blocks;     /* resident bands: blocks per frame, 0 = CUs / frames (2..12)                    */
    int32_t resident_band;       /* wave-blocks of 256 points per band (default 16 = 4096 points)                 */
    int32_t resident_chunk;      /* entries per slot and tile: 64 or 128 (default 128)                            */
    int32_t resident_window;     /* pacing window in bands, -1 = no pacing (default)                              */
    int32_t resident_cap_tiles;  /* tile table per frame, 0 = N / 8 + 1024 (tests shrink it: planner fall-back)   */
    int32_t group_vertices;      /* list-major walk, C = 8 / 9: vertices per block, 0 = by the chunk, 6 or 7      */
    int32_t overlap_build;       /* 1 (default): lattice build on a side stream beside features + forest          */
    int32_t overlap_layers;      /* 1 (default): the label layers' mean fields on two streams                     */
    int32_t build_priority_high; /* 0 (default): the build stream has the lowest priority                         */
    int32_t trace;               /* 1: per-block trace of the resident splat (debugging); 2: + synchronous stderr marks */
    int32_t serial_chains;       /* 0 (default): the normaliser's ordered sums by exact wave scans (kernels_splat.hip:
                                    ordered_tile_sum); 1: one dependent addition per entry, like the reference loop.
                                    Results are bit-identical; 1 exists for tests and timing                        */
    int32_t csr_block;           /* points per wave-block of the counting sort: 0 = by the chunk (256 for <= 8 frames,
                                    else 1024), or 256 / 512 / 1024 / 2048 / 4096                                     */
} rvseg_schedule;
void rvseg_schedule_default(rvseg_schedule *s);
/* Applies to every later call on ctx (buffers of a schedule are allocated on first use). */
rvseg_status rvseg_set_schedule(rvseg_ctx *ctx, const rvseg_schedule *s);

/* What the last lattice build + mean field on this context ran with.  `planner_fallback`, `vertices` and
 * `longest_list` come from the device with the build's status: they are valid once rvseg_poll_status(ctx, 1) has returned (host entry points:
 * on return), -1 before.  A planner fall-back is not an error -- the same grid walks the lists the list-major way,
 * results are identical -- but it is slower, so it is reported here instead of staying silent. */
typedef struct rvseg_schedule_info {
    int32_t splat;               /* 0 = no lattice built yet, 1 = list-major walk, 2 = resident bands             */
    int32_t planner_fallback;    /* resident bands planned, but the planner gave up on this many frames           */
    int32_t csr_path;            /* 1 = counting sort, 2 = radix sort                                             */
    int32_t n_frames;            /* frames (1 for a cloud) and points per frame of that lattice                   */
    int32_t points_per_frame;
    int32_t vertices;            /* lattice vertices over all frames                                              */
    int32_t longest_list;        /* entries of the longest vertex list: the longest ordered chain of the splat    */
    int32_t resident_blocks, resident_band, resident_chunk;   /* the resident schedule's shape (0 when not used)  */
    int32_t capacity_log2;       /* hash slots per frame                                                          */
} rvseg_schedule_info;
rvseg_status rvseg_last_schedule(rvseg_ctx *ctx, rvseg_schedule_info *out);

/* ---- timing of the last segment_frames / crf_infer call, measured with HIP events on the
 *      stream the kernels ran on.  names_out receives a ';'-separated list of stage names,
 *      ms_out up to max_stages durations.  Returns the number of stages. */
int32_t rvseg_last_timing(const rvseg_ctx *ctx, char *names_out, size_t names_cap, float *ms_out,
                          int32_t max_stages);

#ifdef __cplusplus
}
#endif
#endif /* RVSEG_H */
