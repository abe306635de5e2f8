// rvseg_segmenter.hpp -- C++ host-side mirror of the reference's `class Segmenter` for the hot
// path, over the C ABI of librvseg.so (include/rvseg.h).  Header only; no ROS, OpenCV or Eigen.
//
// It keeps the reference's names, argument meaning and error behaviour for this path so that
// src/segmenter.cpp can be re-pointed at it:
//
//   reference (include/segmenter.h, src/segmenter.cpp)        here
//   ---------------------------------------------------------------------------------------------
//   Segmenter::Segmenter(..., config_file, ...)   :38-129     Segmenter(const Config&)
//       throws std::runtime_error                 :65,198          throws std::runtime_error
//       loads forest.dat, silently continues if missing :106-115   throws (RVSEG_ERR_IO)
//   onNewNode(): (seq, depth, colour) per camera  :245-293    enqueueFrame(camera, seq, colour, depth)
//       pushed onto _image_queues[camera]         :283
//   processFramesFromQueueInternalRF()            :323-443    processFramesFromQueueInternalRF(): the worker's loop
//       pops ONE frame per iteration              :340-346        body; pops up to max_batch frames over all cameras into
//       pushes (seq, posteriors) per camera       :434            ONE rvseg_segment_frames call, pushes per camera in order
//       posteriors vector [layer][y][x][class]    :413-431    processFrames(): the body for an explicit batch, same layout
//   processFramesFromQueueExternal()              :445-514    Config::external_semantics: no forest; rectifyDepth() builds the
//       rectified 32FC3 xyz image, calls the      :466-488        request's depth image, processFramesExternal[Device]() takes
//       SingleFrameSegmentation service, stores   :490-512        the provider's label_distribution into the frame CRF / label
//       its label_distribution as the posteriors                  rules (rvseg_segment_external); SingleFrameSegmentation* structs
//   onNewLocalMap(): push onto _local_map_queue   :300-304    onNewLocalMap(LocalMap)
//   processMapFromQueue(): wait for the newest    :518-719    processMapFromQueue(): false while the map has to be postponed
//       result of every camera, drop skipped      :527-553        (:527-553), else drops skipped results, matches by seq
//       results, match by seq, fuse, label, store :589-616        (:589-597), fuses, labels, stores under the map id
//   the two detached worker threads               :227-232    start() / stop(): the same two loops, joined on stop
//   (no counterpart: single process)                          commInit() / gatherLabels(): the local-map label gather over
//                                                                 RCCL when key frames are sharded over several GPUs
//   processMapFromQueue() CRF branch              :628-658    processCloud(): DenseCRF per layer
//       label = max marginal > 2.0/C else Unknown :646-657        same rule (RVSEG_LABEL_CRF)
//   processMapFromQueue() no-CRF branch           :660-681    labelCloud(): RVSEG_LABEL_NOCRF rule
//   processMapFromQueue() accumulation loop       :561-616    fusePosteriors(), processMap()
//   srvSegmentationInformation()                  :776-791    srvSegmentationInformation()
//   _cloud_results + srvStoredSemanticsIds()      :711-729    storeMapResult(), srvStoredSemanticsIds()
//   srvGetLocalMapSegmentation()                  :731-774    srvGetLocalMapSegmentation(): false for an unknown
//                                                                 layer name or map id, layers concatenated
//   /tmp/cloud<ID>_rgb.cld, _layer_<l>.cld dumps  :684-706    dumpClouds()
//   DenseCRF2D::addPairwiseGaussian/Bilateral     densecrf.cpp:61-81   DenseCRF2D (rvseg_crf_features_*)
//   DenseCRF + learned models (dense_learning)    densecrf.cpp:54-60,294-360   DenseCRF: compatibilities, kernel / unary parameters
//   RgbLabelConversion (rgb_label_conversion.h)                RgbLabelConversion: full coding, negative labels included
//   test.cpp / test_multi.cpp confusion + scores  :182-228    Evaluator: counts on the GPU, scores(), report()
//
// Thread rule as in the reference: one thread drives one Segmenter (the RF worker owns the frame
// context, the fusion thread the cloud context); create one object per thread and GPU.
#ifndef RVSEG_SEGMENTER_HPP
#define RVSEG_SEGMENTER_HPP

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <fstream>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "rvseg.h"

namespace rvseg {

// One entry of config.json "color_codings" (resources/config.json:50-79) with label >= 0
struct LabelClass {
    std::string name;
    uint8_t color[3];
};

struct Layer {
    std::string name;                 // "material", "object"
    std::vector<LabelClass> classes;  // ordered by label id (segmenter.cpp:73-98)
    int unknown_label = 0;            // index of the class named "Unknown" (segmenter.cpp:88-96)
};

// The hot-path keys of resources/config.json plus the camera size that the
// node infers from the intrinsics (segmenter.cpp:194-199).
struct Config {
    int width = 640, height = 480;
    std::string forest_file_name;     // config.json:48 ("forest_file_name", resolved against root_dir)
    std::vector<Layer> layers;
    int rf_prediction_stride = 2;
    float depth_min = 0.5f, depth_max = 15.0f;
    int patch_size = 77, patch_size_reduce = 11;
    bool feature_color_patch = true, feature_depth = true, feature_height = true, feature_normal = true;
    bool use_dense_crf = false;
    float dcrf_xyz_kernel = 0.5f, dcrf_rgb_kernel = 4.0f, dcrf_kernel_weight = 10.0f;
    int dcrf_iterations = 10;
    int max_batch = 8;
    int device = 0;
    // launch/semantics.launch `external_semantics` (segmenter.cpp:101-103, 227-228): the single-frame semantics come
    // from an external provider.  No forest is loaded (forest_file_name is not read); `layers` alone gives the layout,
    // as single_frame_segmentation_server.py:68-71 takes it from the config.  processFrames* then throw; use
    // processFramesExternal*.  per_frame_crf / label_mode: the frame CRF and label rule of those calls.
    bool external_semantics = false;
    bool per_frame_crf = false;
    int label_mode = RVSEG_LABEL_NOCRF;
};

// srv/SegmentationInformationSrv.srv response (segmenter.cpp:776-791)
struct SegmentationInformation {
    std::vector<std::string> layer_names;
    std::vector<uint32_t> class_counts;
    std::vector<std::string> class_names;   // flattened
    std::vector<uint8_t> class_colors;      // flattened RGB
};

// srv/IdsSrv.srv response
struct IdsSrvResponse {
    std::vector<int32_t> local_map_ids;
};

// srv/SingleFrameSegmentation.srv: `sensor_msgs/Image rgb`, `sensor_msgs/Image depth` --- `float32[] label_distribution`.
// Image carries the sensor_msgs/Image fields the request fills (segmenter.cpp:490-502), in message order (the header's
// seq is the frame's sequence number, :492).
struct Image {
    uint32_t seq = 0;           // header.seq
    uint32_t height = 0, width = 0;
    std::string encoding;       // "rgb8" (RGB8) / "32FC3" (TYPE_32FC3)
    uint8_t is_bigendian = 0;
    uint32_t step = 0;          // bytes per row
    std::vector<uint8_t> data;
};
struct SingleFrameSegmentationRequest {
    Image rgb;                  // RGB8, H x W x 3 uint8
    Image depth;                // TYPE_32FC3: the rectified xyz image, NaN outside 0.5 .. 15 m (:472)
};
struct SingleFrameSegmentationResponse {
    std::vector<float> label_distribution;   // layers concatenated, each [y][x][class]
};

// srv/LocalMapSegmentationSrv.srv
struct LocalMapSegmentationRequest {
    int32_t local_map_id = 0;
    std::vector<std::string> segmentation_layers;
};
struct LocalMapSegmentationResponse {
    int32_t local_map_id = 0;
    std::vector<uint8_t> point_labels;   // requested layers concatenated, each cloud_size long (segmenter.cpp:757-768)
};

// One fps_mapper::MultiImageMapNode of a local map as the fusion loop needs it (segmenter.cpp:571-621).  The projector is
// external to the reference (fps_mapper::MultiProjector::project, :578): the caller either hands over its result
// (index_image) or the node's pose, from which the library's own projector (include/rvseg.h, a build-owned definition)
// makes the index images of every camera (Segmenter::setCameraMatrices).
struct LocalMapNode {
    std::vector<int> subimage_seqs;        // m_multi->subimageSeqs(): the depth sequence number of every camera's sub-image
    std::vector<int32_t> index_image;      // IndexImage, cameras stacked row-wise: (n_cameras * H) x W, < 0 = no cloud point (:601-604)
    std::vector<float> pose;               // m_multi->transform(): base link -> map, 3 x 4 row-major (12 floats); empty = not given
};
// One fps_mapper::LocalMap: its id, nodes and cloud (xyz in the map frame, rgb in [0, 1]; :560, :629-637)
struct LocalMap {
    int32_t id = 0;
    std::vector<LocalMapNode> nodes;
    size_t cloud_size = 0;
    std::vector<float> cloud_xyz, cloud_rgb;   // cloud_size x 3 each (only read with use_dense_crf)
};

// One point of the cloud as the debug dumps write it.  fps_mapper's Cloud::write is not in the reference tree
// (external dependency), so the record below is this build's own: size_t count, then per point
// 9 little-endian floats (x, y, z, nx, ny, nz, r, g, b), rgb in [0, 1].
struct CloudPoint {
    float xyz[3];
    float normal[3];
    float rgb[3];
};

// The node's result store and the two services that read it (segmenter.cpp:711-774), free of any device
// state: (map id, result_labels[layer][point]) pairs in arrival order behind one mutex.
class LocalMapStore {
public:
    explicit LocalMapStore(std::vector<std::string> layer_names = {}) : layer_names_(std::move(layer_names)) {}

    // "Save data for the service based on the map id" (segmenter.cpp:711-713)
    void store(int32_t local_map_id, const std::vector<std::vector<unsigned char>>& result_labels) {
        std::lock_guard<std::mutex> g(mtx_);
        results_.emplace_back(local_map_id, result_labels);
    }

    bool srvStoredSemanticsIds(IdsSrvResponse& resp) const {   // segmenter.cpp:722-729
        std::lock_guard<std::mutex> g(mtx_);
        for (const auto& m : results_) resp.local_map_ids.push_back(m.first);
        return true;
    }

    bool srvGetLocalMapSegmentation(const LocalMapSegmentationRequest& req, LocalMapSegmentationResponse& resp) const {   // :731-774
        std::vector<int> layer_indices;
        for (const std::string& l : req.segmentation_layers)
            for (size_t i = 0; i < layer_names_.size(); i++)
                if (l == layer_names_[i]) { layer_indices.push_back((int)i); break; }
        if (req.segmentation_layers.size() != layer_indices.size()) return false;   // an unknown layer name (:744-746)
        std::lock_guard<std::mutex> g(mtx_);
        for (const auto& m : results_) {
            if (m.first != req.local_map_id) continue;
            const std::vector<std::vector<unsigned char>>& result_labels = m.second;
            resp.local_map_id = m.first;
            const size_t point_count = result_labels.empty() ? 0 : result_labels[0].size();
            resp.point_labels.reserve(point_count * layer_indices.size());
            for (int l : layer_indices)
                resp.point_labels.insert(resp.point_labels.end(), result_labels[(size_t)l].begin(), result_labels[(size_t)l].end());
            return true;   // the first stored result of that id, like the reference's linear search
        }
        return false;      // an unknown map id (:773)
    }

private:
    std::vector<std::string> layer_names_;
    mutable std::mutex mtx_;
    std::vector<std::pair<int32_t, std::vector<std::vector<unsigned char>>>> results_;
};

// The debug dumps of processMapFromQueue (segmenter.cpp:684-706): <dir>/cloud<ID>_rgb.cld with the cloud's own
// colours, then per layer <dir>/cloud<ID>_layer_<l>.cld with every point painted in its class colour and
// near-zero normals replaced by (0,0,1) (kept for the following layers, as in the reference, which edits the
// cloud in place).  The reference's directory is fixed to /tmp.
inline void dump_clouds(int32_t local_map_id, std::vector<CloudPoint> cloud, const std::vector<std::vector<unsigned char>>& result_labels,
                        const std::vector<Layer>& layers, const std::string& dir = "/tmp") {
    auto write = [&](const std::string& path) {
        std::ofstream os(path, std::ios::binary);
        if (!os.is_open()) throw std::runtime_error("Could not open file. (" + path + ")");
        const size_t n = cloud.size();
        os.write(reinterpret_cast<const char*>(&n), sizeof(n));
        os.write(reinterpret_cast<const char*>(cloud.data()), (std::streamsize)(n * sizeof(CloudPoint)));
    };
    const std::string base = dir + "/cloud" + std::to_string(local_map_id);
    write(base + "_rgb.cld");
    for (size_t layer = 0; layer < result_labels.size() && layer < layers.size(); layer++) {
        for (size_t i = 0; i < cloud.size() && i < result_labels[layer].size(); i++) {
            CloudPoint& pt = cloud[i];
            const float n2 = pt.normal[0] * pt.normal[0] + pt.normal[1] * pt.normal[1] + pt.normal[2] * pt.normal[2];
            if (n2 < 0.1f) { pt.normal[0] = 0.f; pt.normal[1] = 0.f; pt.normal[2] = 1.f; }
            const LabelClass& c = layers[layer].classes.at(result_labels[layer][i]);
            for (int k = 0; k < 3; k++) pt.rgb[k] = static_cast<float>(c.color[k]) / 255.0f;
        }
        write(base + "_layer_" + std::to_string(layer) + ".cld");
    }
}

class Segmenter {
public:
    explicit Segmenter(const Config& conf) : conf_(conf), store_(layer_names_of(conf)) {
        rvseg_params p;
        rvseg_params_default(&p);
        p.width = conf.width; p.height = conf.height;
        p.stride = conf.rf_prediction_stride;
        p.depth_min = conf.depth_min; p.depth_max = conf.depth_max;
        p.patch_size = conf.patch_size; p.patch_size_reduce = conf.patch_size_reduce;
        p.feature_color_patch = conf.feature_color_patch; p.feature_depth = conf.feature_depth;
        p.feature_height = conf.feature_height; p.feature_normal = conf.feature_normal;
        p.fill_value = 0.0f;            // the node zero-fills its low-res images (segmenter.cpp:358-362)
        p.use_dense_crf = 0;            // the node runs the CRF on the fused cloud, not per frame
        p.dcrf_xyz_kernel = conf.dcrf_xyz_kernel; p.dcrf_rgb_kernel = conf.dcrf_rgb_kernel;
        p.dcrf_kernel_weight = conf.dcrf_kernel_weight; p.dcrf_iterations = conf.dcrf_iterations;
        p.multi_layer = 1;              // shared forest, multiClassLogPosterior (segmenter.cpp:368)
        p.label_mode = RVSEG_LABEL_NOCRF;
        if (conf.external_semantics) { p.use_dense_crf = conf.per_frame_crf ? 1 : 0; p.label_mode = conf.label_mode; }
        if (conf.layers.size() > RVSEG_MAX_LAYERS) throw std::runtime_error("too many label layers");
        for (size_t l = 0; l < conf.layers.size(); l++) p.unknown_label[l] = conf.layers[l].unknown_label;
        p.max_batch = conf.max_batch;
        p.device = conf.device;
        if (rvseg_create(&p, &ctx_) != RVSEG_OK) throw std::runtime_error(std::string("rvseg_create: ") + rvseg_last_error(nullptr));
        if (conf.external_semantics) {   // the layout comes from the config, not from a model
            std::vector<int32_t> counts;
            total_labels_ = 0;
            for (const Layer& l : conf.layers) { counts.push_back((int32_t)l.classes.size()); total_labels_ += (unsigned)l.classes.size(); }
            if (rvseg_external_layers_set(ctx_, (int32_t)counts.size(), counts.data()) != RVSEG_OK) fail(std::string("layers: ") + rvseg_last_error(ctx_));
            return;
        }
        if (rvseg_forest_load(ctx_, conf.forest_file_name.c_str()) != RVSEG_OK) {
            const std::string msg = rvseg_last_error(ctx_);
            rvseg_destroy(ctx_);
            ctx_ = nullptr;
            throw std::runtime_error("forest: " + msg);
        }
        int32_t n_layers = 0, cc[RVSEG_MAX_LAYERS];
        rvseg_forest_info(ctx_, nullptr, nullptr, nullptr, &n_layers, cc);
        if ((size_t)n_layers != conf.layers.size()) fail("model / config mismatch: layer count");   // README.md:30
        total_labels_ = 0;
        for (int l = 0; l < n_layers; l++) {
            if ((size_t)cc[l] != conf.layers[l].classes.size()) fail("model / config mismatch: class count of layer " + conf.layers[l].name);
            total_labels_ += cc[l];
        }
    }
    ~Segmenter() {
        stop();
        if (map_ctx_) rvseg_destroy(map_ctx_);
        if (ctx_) rvseg_destroy(ctx_);
    }

    // ---- the queue layer (segmenter.h:94-108): _image_queues / _result_queues under _frame_mtx, _local_map_queue under
    //      _cloud_processing_mtx ---------------------------------------------------------------------------------------
    // initializeProjector's camera table (segmenter.cpp:161-205): one calibration (K^-1, R, t: 21 floats) per camera, in the
    // mapper's camera order; sizes the queues (:207-225).
    void setCameras(int n_cameras, const float* calib) {
        std::lock_guard<std::mutex> g(frame_mtx_);
        camera_calib_.assign(calib, calib + (size_t)n_cameras * 21);
        image_queues_.assign((size_t)n_cameras, {});
        result_queues_.assign((size_t)n_cameras, {});
    }
    int cameraCount() const { return (int)image_queues_.size(); }
    // initializeProjector's intrinsics (segmenter.cpp:234-240): one K (3 x 3 row-major) per camera of setCameras, for the
    // nodes that arrive with a pose instead of an index image
    void setCameraMatrices(const float* K) {
        std::lock_guard<std::mutex> g(frame_mtx_);
        camera_K_.assign(K, K + image_queues_.size() * 9);
    }

    // onNewNode for one camera's sub-image (segmenter.cpp:271-284): the frames are copied (the reference holds cv::Mat
    // references) and pushed with their depth sequence number.
    void enqueueFrame(int camera, int seq, const uint8_t* color, const uint16_t* depth) {
        const size_t npix = (size_t)conf_.width * conf_.height;
        QueuedFrame f;
        f.seq = seq;
        f.color.assign(color, color + npix * 3);
        f.depth.assign(depth, depth + npix);
        std::lock_guard<std::mutex> g(frame_mtx_);
        if (camera < 0 || (size_t)camera >= image_queues_.size()) throw std::runtime_error("Found a frame for an unknown camera!");   // :203
        image_queues_[(size_t)camera].push_back(std::move(f));
    }

    // One iteration of the RF worker (segmenter.cpp:334-443).  The reference pops ONE frame per iteration and holds
    // _frame_mtx while it extracts and classifies; here up to max_batch queued frames -- cameras visited round robin like
    // the reference's `for i < max` loop, every camera in FIFO order -- go through ONE rvseg_segment_frames call (a
    // chunk of 64 frames runs at 12x the per-frame rate of single-frame calls on MI355X), the mutex is held only to pop
    // and to push.  Returns the number of frames processed (0: nothing queued; the reference sleeps 1 ms then, :438-439).
    int processFramesFromQueueInternalRF() {
        std::vector<QueuedFrame> batch;
        std::vector<int> cams;
        {
            std::lock_guard<std::mutex> g(frame_mtx_);
            bool any = true;
            while (any && (int)batch.size() < conf_.max_batch) {
                any = false;
                for (size_t i = 0; i < image_queues_.size() && (int)batch.size() < conf_.max_batch; i++) {
                    if (image_queues_[i].empty()) continue;
                    batch.push_back(std::move(image_queues_[i].front()));   // :340-341
                    image_queues_[i].pop_front();
                    cams.push_back((int)i);
                    any = true;
                }
            }
        }
        if (batch.empty()) return 0;
        const size_t npix = (size_t)conf_.width * conf_.height;
        const int n = (int)batch.size();
        std::vector<uint8_t> color((size_t)n * npix * 3);
        std::vector<uint16_t> depth((size_t)n * npix);
        std::vector<float> calib((size_t)n * 21);
        for (int k = 0; k < n; k++) {
            std::memcpy(color.data() + (size_t)k * npix * 3, batch[(size_t)k].color.data(), npix * 3);
            std::memcpy(depth.data() + (size_t)k * npix, batch[(size_t)k].depth.data(), npix * 2);
            std::memcpy(calib.data() + (size_t)k * 21, camera_calib_.data() + (size_t)cams[(size_t)k] * 21, 21 * sizeof(float));   // :349
        }
        std::vector<std::vector<float>> post = processFrames(n, color.data(), depth.data(), calib.data());
        std::lock_guard<std::mutex> g(frame_mtx_);
        for (int k = 0; k < n; k++)   // per camera the pop order is the push order: sequence numbers stay ascending (:434)
            result_queues_[(size_t)cams[(size_t)k]].emplace_back(batch[(size_t)k].seq, std::move(post[(size_t)k]));
        return n;
    }

    // read access for tests / monitoring: (seq, posteriors) pairs waiting for the fusion thread
    size_t resultCount(int camera) const { std::lock_guard<std::mutex> g(frame_mtx_); return result_queues_.at((size_t)camera).size(); }
    std::pair<int, std::vector<float>> resultAt(int camera, size_t k) const { std::lock_guard<std::mutex> g(frame_mtx_); return result_queues_.at((size_t)camera).at(k); }

    void onNewLocalMap(LocalMap lmap) {   // segmenter.cpp:300-304
        std::lock_guard<std::mutex> g(cloud_processing_mtx_);
        local_map_queue_.push_back(std::move(lmap));
    }

    // One iteration of the fusion worker (segmenter.cpp:521-719).  false: no map queued, or the front map has to be
    // postponed because some camera's newest result is older than the map's last sub-image (:527-553; an empty result
    // queue counts as "not there yet" -- the reference reads .back() of an empty deque).  true: the front map was
    // processed: per node and camera results older than the wanted sequence number are dropped (:589-592), an exact
    // match is fused (:594-616), a missing one is skipped with a message (:618-621); then CRF / no-CRF labelling and
    // the store under the map id (:628-713).
    bool processMapFromQueue() {
        LocalMap lmap;
        {
            std::lock_guard<std::mutex> g(cloud_processing_mtx_);
            if (local_map_queue_.empty()) return false;
            const LocalMap& front = local_map_queue_.front();
            std::vector<int> last_ids;
            for (const LocalMapNode& nd : front.nodes) last_ids = nd.subimage_seqs;   // :531-538: the LAST node's ids
            {
                std::lock_guard<std::mutex> f(frame_mtx_);
                for (size_t i = 0; i < last_ids.size() && i < result_queues_.size(); i++)
                    if (result_queues_[i].empty() || result_queues_[i].back().first < last_ids[i]) return false;   // :541-546
            }
            lmap = std::move(local_map_queue_.front());
            local_map_queue_.pop_front();   // :556
        }
        const size_t npix = (size_t)conf_.width * conf_.height;
        const size_t per = (size_t)total_labels_ * npix;
        std::vector<int32_t> index_images;
        std::vector<float> posteriors;
        std::vector<float> projections;      // of the sub-images whose node has a pose and no index image ...
        std::vector<int> projected_slots;    // ... and their places in index_images
        int n_images = 0;
        for (const LocalMapNode& nd : lmap.nodes) {
            for (size_t i = 0; i < nd.subimage_seqs.size() && i < result_queues_.size(); i++) {
                std::lock_guard<std::mutex> f(frame_mtx_);
                std::deque<std::pair<int, std::vector<float>>>& q = result_queues_[i];
                while (!q.empty() && q.front().first < nd.subimage_seqs[i]) q.pop_front();   // "Drop skipped maps", :589-592
                if (!q.empty() && q.front().first == nd.subimage_seqs[i]) {
                    if (nd.index_image.empty() && nd.pose.size() == 12 && camera_K_.size() >= (i + 1) * 9) {   // the projector's job, :576-578
                        float P[12];
                        if (rvseg_projection_matrix(camera_K_.data() + i * 9, camera_calib_.data() + i * 21 + 9, nd.pose.data(), P) != RVSEG_OK)
                            throw std::runtime_error("rvseg_projection_matrix failed");
                        projections.insert(projections.end(), P, P + 12);
                        projected_slots.push_back(n_images);
                        index_images.insert(index_images.end(), npix, -1);
                    } else {
                        if (nd.index_image.size() < (i + 1) * npix) throw std::runtime_error("index image smaller than n_cameras * H x W");
                        index_images.insert(index_images.end(), nd.index_image.begin() + (std::ptrdiff_t)(i * npix),
                                            nd.index_image.begin() + (std::ptrdiff_t)((i + 1) * npix));   // rows y + i*_camera_h, :601
                    }
                    posteriors.insert(posteriors.end(), q.front().second.begin(), q.front().second.end());
                    q.pop_front();
                    n_images++;
                } else {
                    std::fprintf(stderr, "Couldn't find a semantic map for key frame: %d\n", nd.subimage_seqs[i]);   // :618-621
                }
            }
        }
        if (posteriors.size() != (size_t)n_images * per) throw std::runtime_error("result queue entry of the wrong size");
        if (!projected_slots.empty()) {   // the queue layer works on host buffers like its neighbours; processMapPosesDevice stays in HBM
            const std::vector<int32_t> made = projectCloud((int)projected_slots.size(), projections.data(), lmap.cloud_size, lmap.cloud_xyz.data());
            for (size_t k = 0; k < projected_slots.size(); k++)
                std::memcpy(index_images.data() + (size_t)projected_slots[k] * npix, made.data() + k * npix, npix * sizeof(int32_t));
        }
        processMap(lmap.id, n_images, index_images.data(), posteriors.data(), lmap.cloud_size, lmap.cloud_xyz.data(), lmap.cloud_rgb.data());
        return true;
    }

    // The two worker threads of initializeProjector (segmenter.cpp:227-232), joinable instead of detached.  Each loop
    // sleeps 1 ms when it has nothing to do (:438-439, :549-551).  An exception of a worker ends that worker and is
    // re-thrown by stop().
    void start() {
        if (running_.exchange(true)) return;
        rf_thread_ = std::thread([this] { worker([this] { return processFramesFromQueueInternalRF() > 0; }, rf_error_); });
        map_thread_ = std::thread([this] { worker([this] { return processMapFromQueue(); }, map_error_); });
    }
    void stop() {
        if (!running_.exchange(false)) return;
        if (rf_thread_.joinable()) rf_thread_.join();
        if (map_thread_.joinable()) map_thread_.join();
        std::string err = rf_error_.empty() ? map_error_ : rf_error_;
        rf_error_.clear(); map_error_.clear();
        if (!err.empty()) throw std::runtime_error(err);
    }

    // ---- key frames sharded over several GPUs (one Segmenter per GPU, in its own process or thread): the local-map label
    //      gather to the fusion rank over RCCL / xGMI (rvseg_comm_*, include/rvseg.h) ------------------------------------------
    static std::array<uint8_t, RVSEG_COMM_ID_BYTES> commUniqueId() {   // rank 0 creates it, the host distributes it
        std::array<uint8_t, RVSEG_COMM_ID_BYTES> id{};
        if (rvseg_comm_unique_id(id.data()) != RVSEG_OK) throw std::runtime_error("rvseg_comm_unique_id failed (librccl.so missing?)");
        return id;
    }
    void commInit(int rank, int world, const std::array<uint8_t, RVSEG_COMM_ID_BYTES>& id) { check(rvseg_comm_init(ctx_, rank, world, id.data())); }
    // every rank's bytes_per_rank bytes of device memory (int8 labels n x L x H x W, or fp32 posteriors for the
    // order-preserving fusion) land at d_recv + rank * bytes_per_rank on `root`; enqueued on hip_stream
    void gatherLabels(const void* d_local, size_t bytes_per_rank, void* d_recv, int root, void* hip_stream) {
        check(rvseg_gather_frames(ctx_, d_local, bytes_per_rank, d_recv, root, hip_stream));
    }
    Segmenter(const Segmenter&) = delete;
    Segmenter& operator=(const Segmenter&) = delete;

    // Body of processFramesFromQueueInternalRF for n dequeued frames: color = rgb8 (n x H x W x 3),
    // depth = 16UC1 millimetres, calib = n x 21 floats (K^-1, R, t).  Returns one `posteriors`
    // vector per frame, layout [layer][y][x][class] (segmenter.cpp:413-431).
    std::vector<std::vector<float>> processFrames(int n, const uint8_t* color, const uint16_t* depth, const float* calib) {
        const size_t per = (size_t)total_labels_ * conf_.width * conf_.height;
        std::vector<float> flat((size_t)n * per);
        check(rvseg_segment_frames(ctx_, n, color, depth, calib, flat.data(), nullptr, nullptr));
        std::vector<std::vector<float>> out((size_t)n);
        for (int i = 0; i < n; i++) out[i].assign(flat.begin() + (size_t)i * per, flat.begin() + (size_t)(i + 1) * per);
        return out;
    }

    // ---- the external provider (processFramesFromQueueExternal, segmenter.cpp:445-514) ---------------------------------
    // The rectified xyz image of :466-488 for n frames: n x H x W x 3 floats, NaN where the depth is outside
    // [depth_min, depth_max] (the reference's 0.5 / 15.0 by default).
    std::vector<float> rectifyDepth(int n, const uint16_t* depth, const float* calib, float depth_min = 0.5f, float depth_max = 15.0f) {
        std::vector<float> xyz((size_t)n * conf_.width * conf_.height * 3);
        check(rvseg_rectify_depth(ctx_, n, depth, calib, depth_min, depth_max, xyz.data()));
        return xyz;
    }
    // The request of :490-502 for one frame
    SingleFrameSegmentationRequest externalRequest(int seq, const uint8_t* color, const uint16_t* depth, const float* calib) {
        SingleFrameSegmentationRequest req;
        const uint32_t W = (uint32_t)conf_.width, H = (uint32_t)conf_.height;
        req.rgb.seq = req.depth.seq = (uint32_t)seq;
        req.rgb.height = req.depth.height = H;
        req.rgb.width = req.depth.width = W;
        req.rgb.encoding = "rgb8";
        req.rgb.step = W * 3;
        req.rgb.data.assign(color, color + (size_t)W * H * 3);
        req.depth.encoding = "32FC3";
        req.depth.step = W * 12;
        const std::vector<float> xyz = rectifyDepth(1, depth, calib);
        req.depth.data.resize(xyz.size() * sizeof(float));
        std::memcpy(req.depth.data.data(), xyz.data(), req.depth.data.size());
        return req;
    }
    // The layer layout of the provider (also set by the constructor with Config::external_semantics)
    void setExternalLayers(const std::vector<int32_t>& class_counts) {
        check(rvseg_external_layers_set(ctx_, (int32_t)class_counts.size(), class_counts.data()));
    }
    // The provider's distributions of n frames (n x S x h x w floats; dist_stride 1: h x w = H x W, rf_prediction_stride:
    // H/stride x W/stride) through the frame CRF (Config::per_frame_crf) and the label rule.  marginals_out (n x S x H x W)
    // and labels_out (n x L x H x W) are optional.
    void processFramesExternal(int n, const uint8_t* color, const uint16_t* depth, const float* calib, const float* label_distribution,
                               int dist_stride, float* marginals_out, int8_t* labels_out) {
        check(rvseg_segment_external(ctx_, n, color, depth, calib, label_distribution, dist_stride, marginals_out, labels_out));
    }
    void processFramesExternalDevice(int n, const uint8_t* d_color, const uint16_t* d_depth, const float* calib,
                                     const float* d_label_distribution, int dist_stride, float* d_marginals_out, int8_t* d_labels_out,
                                     void* hip_stream) {
        check(rvseg_segment_external_device(ctx_, n, d_color, d_depth, calib, d_label_distribution, dist_stride, d_marginals_out,
                                            d_labels_out, hip_stream));
    }

    // CRF branch of processMapFromQueue for one layer: `unaries` is the accumulated posterior
    // matrix C x cloud_size (Eigen column-major == cloud_size x C point-major), `pairwise` the
    // 6 x cloud_size feature matrix of segmenter.cpp:629-637.  Returns result_labels[l].
    std::vector<unsigned char> processCloud(size_t layer, size_t cloud_size, const float* unaries, const float* pairwise) {
        const int C = (int)conf_.layers.at(layer).classes.size();
        std::vector<float> energy(cloud_size * (size_t)C), Q(cloud_size * (size_t)C);
        for (size_t i = 0; i < energy.size(); i++) energy[i] = -unaries[i];   // crf.setUnaryEnergy(-unaries[l]), :642
        std::vector<int8_t> map(cloud_size);
        rvseg_ctx* mc = map_ctx();   // the fusion thread's context: the RF worker may be inside ctx_ at this moment
        check(rvseg_crf_infer(mc, (int32_t)cloud_size, C, 6, energy.data(), pairwise, conf_.dcrf_kernel_weight,
                              conf_.dcrf_iterations, Q.data(), map.data(), RVSEG_LABEL_CRF, conf_.layers[layer].unknown_label), mc);
        return std::vector<unsigned char>(map.begin(), map.end());
    }

    // no-CRF branch (segmenter.cpp:660-681): strict '>' from -1000 with the sum != 0 guard
    std::vector<unsigned char> labelCloud(size_t layer, size_t cloud_size, const float* unaries) {
        const int C = (int)conf_.layers.at(layer).classes.size();
        std::vector<int8_t> map(cloud_size);
        rvseg_ctx* mc = map_ctx();
        check(rvseg_label_values(mc, unaries, (int32_t)cloud_size, C, RVSEG_LABEL_NOCRF, conf_.layers[layer].unknown_label, map.data()), mc);
        return std::vector<unsigned char>(map.begin(), map.end());
    }

    // Accumulation loop of processMapFromQueue (segmenter.cpp:561-616): index_images holds one
    // H x W IndexImage per (map node, camera) that has a segmentation, posteriors the matching
    // label distributions (processFrames output) in the same order.  Returns unaries[layer], each
    // C_l x cloud_size column-major like the Eigen matrices of :563-567.
    std::vector<std::vector<float>> fusePosteriors(int n_images, const int32_t* index_images, const float* posteriors, size_t cloud_size) {
        std::vector<int32_t> cc;
        for (const Layer& l : conf_.layers) cc.push_back((int32_t)l.classes.size());
        std::vector<float> flat(cloud_size * (size_t)total_labels_);
        rvseg_ctx* mc = map_ctx();
        check(rvseg_fuse_posteriors(mc, n_images, index_images, posteriors, (int32_t)cc.size(), cc.data(), (int32_t)cloud_size, flat.data()), mc);
        std::vector<std::vector<float>> out(cc.size());
        size_t off = 0;
        for (size_t l = 0; l < cc.size(); l++) {
            out[l].assign(flat.begin() + off, flat.begin() + off + cloud_size * (size_t)cc[l]);
            off += cloud_size * (size_t)cc[l];
        }
        return out;
    }

    // processMapFromQueue for one local map (segmenter.cpp:561-682): fusion, then per layer the cloud
    // CRF (:628-658) or the no-CRF rule (:660-681).  cloud_xyz / cloud_rgb: cloud_size x 3, rgb in [0,1].
    std::vector<std::vector<unsigned char>> processMap(int n_images, const int32_t* index_images, const float* posteriors,
                                                       size_t cloud_size, const float* cloud_xyz, const float* cloud_rgb) {
        const std::vector<std::vector<float>> unaries = fusePosteriors(n_images, index_images, posteriors, cloud_size);
        std::vector<std::vector<unsigned char>> result_labels(unaries.size());
        std::vector<float> pairwise;
        if (conf_.use_dense_crf) {
            pairwise.resize(cloud_size * 6);
            for (size_t i = 0; i < cloud_size; i++) {            // segmenter.cpp:629-637
                for (int k = 0; k < 3; k++) pairwise[i * 6 + k] = cloud_xyz[i * 3 + k] * conf_.dcrf_xyz_kernel;
                for (int k = 0; k < 3; k++) pairwise[i * 6 + 3 + k] = cloud_rgb[i * 3 + k] * conf_.dcrf_rgb_kernel;
            }
        }
        for (size_t l = 0; l < unaries.size(); l++)
            result_labels[l] = conf_.use_dense_crf ? processCloud(l, cloud_size, unaries[l].data(), pairwise.data())
                                                   : labelCloud(l, cloud_size, unaries[l].data());
        return result_labels;
    }

    // processMapFromQueue with every buffer in HBM (device pointers; work is enqueued on hip_stream and
    // not waited for): d_posteriors is what rvseg_segment_frames_device wrote, d_labels_out receives
    // L x cloud_size labels.  Nothing crosses PCIe.
    void processMapDevice(int n_images, const int32_t* d_index_images, const float* d_posteriors, size_t cloud_size,
                          const float* d_cloud_xyz, const float* d_cloud_rgb, int8_t* d_labels_out, void* hip_stream) {
        rvseg_ctx* mc = map_ctx();
        check(rvseg_process_map_device(mc, n_images, d_index_images, d_posteriors, (int32_t)cloud_size, d_cloud_xyz, d_cloud_rgb,
                                       d_labels_out, nullptr, hip_stream), mc);
    }

    // The projector (segmenter.cpp:234-240, 576-578; the definition is include/rvseg.h's): one 3 x 4 projection matrix per
    // sub-image (rvseg_projection_matrix), cloud_xyz in the map frame.  Returns n_images x H x W indices, -1 = no point;
    // zbuffer (optional) receives the winners' depths, +inf = no point.
    std::vector<int32_t> projectCloud(int n_images, const float* projections, size_t cloud_size, const float* cloud_xyz,
                                      std::vector<float>* zbuffer = nullptr) {
        const size_t n = (size_t)(n_images > 0 ? n_images : 0) * (size_t)conf_.width * conf_.height;
        std::vector<int32_t> index(n, -1);
        if (zbuffer) zbuffer->assign(n, std::numeric_limits<float>::infinity());
        rvseg_ctx* mc = map_ctx();
        check(rvseg_project_cloud(mc, n_images, projections, (int32_t)cloud_size, cloud_xyz, index.data(), zbuffer ? zbuffer->data() : nullptr), mc);
        return index;
    }

    // processMapDevice with the index images made in HBM by the projector from one projection matrix per sub-image
    // (host array, n_images x 12); d_index_out (optional) receives them.
    void processMapPosesDevice(int n_images, const float* projections, const float* d_posteriors, size_t cloud_size, const float* d_cloud_xyz,
                               const float* d_cloud_rgb, int8_t* d_labels_out, int32_t* d_index_out, void* hip_stream) {
        rvseg_ctx* mc = map_ctx();
        check(rvseg_process_map_poses_device(mc, n_images, projections, d_posteriors, (int32_t)cloud_size, d_cloud_xyz, d_cloud_rgb,
                                             d_labels_out, nullptr, d_index_out, hip_stream), mc);
    }

    // "Save data for the service based on the map id" (segmenter.cpp:711-713)
    void storeMapResult(int32_t local_map_id, const std::vector<std::vector<unsigned char>>& result_labels) { store_.store(local_map_id, result_labels); }

    // processMap + storeMapResult: what processMapFromQueue does for one dequeued local map
    std::vector<std::vector<unsigned char>> processMap(int32_t local_map_id, int n_images, const int32_t* index_images,
                                                       const float* posteriors, size_t cloud_size, const float* cloud_xyz,
                                                       const float* cloud_rgb) {
        std::vector<std::vector<unsigned char>> r = processMap(n_images, index_images, posteriors, cloud_size, cloud_xyz, cloud_rgb);
        storeMapResult(local_map_id, r);
        return r;
    }

    bool srvStoredSemanticsIds(IdsSrvResponse& resp) const { return store_.srvStoredSemanticsIds(resp); }
    bool srvGetLocalMapSegmentation(const LocalMapSegmentationRequest& req, LocalMapSegmentationResponse& resp) const {
        return store_.srvGetLocalMapSegmentation(req, resp);
    }
    void dumpClouds(int32_t local_map_id, const std::vector<CloudPoint>& cloud, const std::vector<std::vector<unsigned char>>& result_labels,
                    const std::string& dir = "/tmp") const {
        dump_clouds(local_map_id, cloud, result_labels, conf_.layers, dir);
    }

    // Device-resident twin of processFrames: rgb / depth / posteriors are device pointers, work is enqueued on
    // hip_stream (rvseg_segment_frames_device); calib stays a host array.
    void processFramesDevice(int n, const uint8_t* d_color, const uint16_t* d_depth, const float* calib, float* d_posteriors_out,
                             void* hip_stream) {
        check(rvseg_segment_frames_device(ctx_, n, d_color, d_depth, calib, d_posteriors_out, nullptr, nullptr, hip_stream));
    }

    bool srvSegmentationInformation(SegmentationInformation& resp) const {
        resp = SegmentationInformation();
        for (const Layer& l : conf_.layers) {
            resp.layer_names.push_back(l.name);
            resp.class_counts.push_back((uint32_t)l.classes.size());
            for (const LabelClass& c : l.classes) {
                resp.class_names.push_back(c.name);
                resp.class_colors.insert(resp.class_colors.end(), c.color, c.color + 3);
            }
        }
        return true;
    }

    unsigned totalLabels() const { return total_labels_; }
    rvseg_ctx* context() { return ctx_; }
    // The fusion thread's context: same model and parameters, CRF switch as configured (the frame context keeps
    // use_dense_crf = 0 because the node runs the CRF on the fused cloud only).  Created on first use; everything the
    // fusion thread calls (fusePosteriors, processCloud, labelCloud, processMap*) runs on it, everything the RF worker
    // calls (processFrames*) on the frame context -- one context per thread, as include/rvseg.h requires.
    rvseg_ctx* map_ctx() {
        std::lock_guard<std::mutex> g(map_ctx_mtx_);
        if (map_ctx_) return map_ctx_;
        rvseg_params p;
        rvseg_params_default(&p);
        p.width = conf_.width; p.height = conf_.height;
        p.depth_min = conf_.depth_min; p.depth_max = conf_.depth_max;   // the projector's setMinDistance / setMaxDistance (:239-240)
        p.use_dense_crf = conf_.use_dense_crf ? 1 : 0;
        p.dcrf_xyz_kernel = conf_.dcrf_xyz_kernel; p.dcrf_rgb_kernel = conf_.dcrf_rgb_kernel;
        p.dcrf_kernel_weight = conf_.dcrf_kernel_weight; p.dcrf_iterations = conf_.dcrf_iterations;
        p.patch_size = conf_.patch_size; p.patch_size_reduce = conf_.patch_size_reduce;
        p.feature_color_patch = conf_.feature_color_patch; p.feature_depth = conf_.feature_depth;
        p.feature_height = conf_.feature_height; p.feature_normal = conf_.feature_normal;
        p.multi_layer = 1;
        for (size_t l = 0; l < conf_.layers.size(); l++) p.unknown_label[l] = conf_.layers[l].unknown_label;
        p.device = conf_.device;
        if (rvseg_create(&p, &map_ctx_) != RVSEG_OK) throw std::runtime_error(std::string("rvseg_create: ") + rvseg_last_error(nullptr));
        // (with external semantics there is no model: the calls that take the layout from one -- processMapDevice -- refuse)
        if (!conf_.external_semantics && rvseg_forest_load(map_ctx_, conf_.forest_file_name.c_str()) != RVSEG_OK) {
            const std::string msg = rvseg_last_error(map_ctx_);
            rvseg_destroy(map_ctx_);
            map_ctx_ = nullptr;
            throw std::runtime_error("forest: " + msg);
        }
        return map_ctx_;
    }

private:
    struct QueuedFrame {
        int seq = 0;
        std::vector<uint8_t> color;
        std::vector<uint16_t> depth;
    };
    template <class Step>
    void worker(Step step, std::string& error) {
        try {
            while (running_.load()) {
                if (!step()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
            }
        } catch (const std::exception& e) {
            error = e.what();
        }
    }
    void check(rvseg_status st, const rvseg_ctx* c = nullptr) const {
        if (st != RVSEG_OK) throw std::runtime_error(std::string(rvseg_status_string(st)) + ": " + rvseg_last_error(c ? c : ctx_));
    }
    [[noreturn]] void fail(const std::string& msg) {
        rvseg_destroy(ctx_);
        ctx_ = nullptr;
        throw std::runtime_error(msg);
    }
    static std::vector<std::string> layer_names_of(const Config& c) {
        std::vector<std::string> n;
        for (const Layer& l : c.layers) n.push_back(l.name);
        return n;
    }
    Config conf_;
    rvseg_ctx* ctx_ = nullptr;
    rvseg_ctx* map_ctx_ = nullptr;
    unsigned total_labels_ = 0;
    LocalMapStore store_;   // _cloud_results / _cloud_mtx (segmenter.h:94-108)
    // queue layer
    mutable std::mutex frame_mtx_;            // _frame_mtx: image and result queues
    std::mutex cloud_processing_mtx_;         // _cloud_processing_mtx: the local-map queue
    std::vector<float> camera_calib_;         // 21 floats per camera
    std::vector<float> camera_K_;             // 9 floats per camera (setCameraMatrices), or empty
    std::vector<std::deque<QueuedFrame>> image_queues_;                               // _image_queues
    std::vector<std::deque<std::pair<int, std::vector<float>>>> result_queues_;      // _result_queues
    std::deque<LocalMap> local_map_queue_;                                            // _local_map_queue
    std::mutex map_ctx_mtx_;
    std::atomic<bool> running_{false};
    std::thread rf_thread_, map_thread_;
    std::string rf_error_, map_error_;
};

// Label compatibilities of a learned model (labelcompatibility.h): Potts (1 value), Diagonal (M values), Matrix (M x M,
// symmetrised W = 0.5 (m + m^T) in fp32 when created, labelcompatibility.cpp:79).  parameters() / setParameters() pack
// them as the reference does (Matrix: the upper triangle of W row by row, :88-100).
struct LabelCompatibility {
    int32_t kind = RVSEG_COMPAT_POTTS;
    int M = 0;                   // Matrix: the class count
    std::vector<float> params;   // Potts {w}; Diagonal v; Matrix W row-major
    std::vector<float> parameters() const {
        if (kind != RVSEG_COMPAT_MATRIX) return params;
        std::vector<float> r;
        for (int i = 0; i < M; i++)
            for (int j = i; j < M; j++) r.push_back(params[(size_t)i * M + j]);
        return r;
    }
    void setParameters(const float* v) {
        if (kind != RVSEG_COMPAT_MATRIX) { std::copy(v, v + params.size(), params.begin()); return; }
        for (int i = 0, k = 0; i < M; i++)
            for (int j = i; j < M; j++, k++) params[(size_t)i * M + j] = params[(size_t)j * M + i] = v[k];
    }
};
struct PottsCompatibility : LabelCompatibility {
    explicit PottsCompatibility(float w) { kind = RVSEG_COMPAT_POTTS; params = {w}; }
};
struct DiagonalCompatibility : LabelCompatibility {
    explicit DiagonalCompatibility(std::vector<float> v) { kind = RVSEG_COMPAT_DIAGONAL; params = std::move(v); }
};
struct MatrixCompatibility : LabelCompatibility {
    MatrixCompatibility(const float* m /* M x M row-major */, int classes) {
        kind = RVSEG_COMPAT_MATRIX;
        M = classes;
        params.resize((size_t)M * M);
        for (int i = 0; i < M; i++)
            for (int j = 0; j < M; j++) {
                const float sum = m[(size_t)i * M + j] + m[(size_t)j * M + i];
                params[(size_t)i * M + j] = 0.5f * sum;
            }
    }
};

// Learning objectives (objective.h) over ground-truth labels gt (N values; a label outside 0 .. M-1 skips its point).
// Hamming takes the class weights themselves (M values); the reference's Hamming(gt, class_weight_pow) constructor
// (objective.cpp:51-63) is a few host lines the caller keeps.
struct ObjectiveFunction {
    int32_t kind = RVSEG_OBJECTIVE_LOGLIKELIHOOD;
    std::vector<int16_t> gt;
    float robust = 0.f;
    std::vector<float> class_weight;
    rvseg_crf_objective record() const { return rvseg_crf_objective{kind, gt.data(), robust, class_weight.empty() ? nullptr : class_weight.data()}; }
};
struct LogLikelihood : ObjectiveFunction {
    explicit LogLikelihood(std::vector<int16_t> g, float robust_ = 0.f) { kind = RVSEG_OBJECTIVE_LOGLIKELIHOOD; gt = std::move(g); robust = robust_; }
};
struct Hamming : ObjectiveFunction {
    Hamming(std::vector<int16_t> g, std::vector<float> weights) { kind = RVSEG_OBJECTIVE_HAMMING; gt = std::move(g); class_weight = std::move(weights); }
};
struct IntersectionOverUnion : ObjectiveFunction {
    explicit IntersectionOverUnion(std::vector<int16_t> g) { kind = RVSEG_OBJECTIVE_IOU; gt = std::move(g); }
};

// DenseCRF (densecrf.h:36-121) over feature matrices the caller builds: N points, M labels.  addPairwiseEnergy with a bare
// weight is PottsCompatibility; a model of bare weights with NORMALIZE_SYMMETRIC and no kernel parameters runs through
// rvseg_crf_infer_multi as before, every other model (learned compatibilities, normalisations, kernel parameters, a
// logistic unary) through rvseg_crf_infer_terms.
class DenseCRF {
public:
    DenseCRF(rvseg_ctx* ctx, int N, int M) : ctx_(ctx), N_(N), M_(M) {}
    void setUnaryEnergy(const float* unary /* N x M */) { model_serial_ = 0; unary_.assign(unary, unary + (size_t)N_ * M_); logistic_f_.clear(); }
    // LogisticUnaryEnergy (unary.cpp:44-63): L M x K row-major, f N x K point-major
    // A live model of this object keeps f and computes L f itself (rvseg_crf_model_set_logistic): no lattice is built again.
    void setUnaryEnergy(const float* L, const float* f, int K) {
        K_ = K;
        logistic_L_.assign(L, L + (size_t)M_ * K);
        logistic_f_.assign(f, f + (size_t)N_ * K);
        unary_.clear();
        inPlace([&] { return rvseg_crf_model_set_logistic(ctx_, K_, logistic_L_.data(), logistic_f_.data()); });
    }
    void addPairwiseEnergy(const float* features /* N x d */, int d, float potts_w) {                       // densecrf.cpp:54-60
        addTerm(features, d, PottsCompatibility(potts_w), RVSEG_DIAG_KERNEL, RVSEG_NORMALIZE_SYMMETRIC, true);
    }
    void addPairwiseEnergy(const float* features, int d, const LabelCompatibility& function, int kernel_type = RVSEG_DIAG_KERNEL,
                           int normalization = RVSEG_NORMALIZE_SYMMETRIC) {
        addTerm(features, d, function, kernel_type, normalization, false);
    }
    // ---- parameters (densecrf.cpp:294-360) ----
    std::vector<float> unaryParameters() const {   // L column-major (unary.cpp:53-57)
        std::vector<float> r;
        if (logistic_f_.empty()) return r;
        for (int k = 0; k < K_; k++)
            for (int m = 0; m < M_; m++) r.push_back(logistic_L_[(size_t)m * K_ + k]);
        return r;
    }
    // The set*Parameters calls change a live model of this object in place (rvseg_crf_model_set_logistic_params, _set_compat,
    // _set_kernel for the terms whose values changed); without one, the next call that needs the model sets it.
    void setUnaryParameters(const std::vector<float>& v) {
        if (logistic_f_.empty()) return;
        assignUnary(v.data(), v.size());
        inPlace([&] { return rvseg_crf_model_set_logistic_params(ctx_, logistic_L_.data()); });
    }
    std::vector<float> labelCompatibilityParameters() const {
        std::vector<float> r;
        for (const auto& t : terms_) { const auto p = t.compat.parameters(); r.insert(r.end(), p.begin(), p.end()); }
        return r;
    }
    void setLabelCompatibilityParameters(const std::vector<float>& v) {
        assignCompat(v.data(), v.size());
        inPlace([&] {
            rvseg_status st = RVSEG_OK;
            for (size_t t = 0; t < terms_.size() && st == RVSEG_OK; t++) st = rvseg_crf_model_set_compat(ctx_, (int32_t)t, terms_[t].compat.params.data());
            return st;
        });
    }
    std::vector<float> kernelParameters() const {   // DenseKernel::parameters (pairwise.cpp:116-125)
        std::vector<float> r;
        for (const auto& t : terms_) { const auto p = kernelParams(t); r.insert(r.end(), p.begin(), p.end()); }
        return r;
    }
    void setKernelParameters(const std::vector<float>& v) {   // pairwise.cpp:140-152
        const std::vector<int> changed = assignKernel(v.data(), v.size());
        inPlace([&] {
            rvseg_status st = RVSEG_OK;
            for (size_t c = 0; c < changed.size() && st == RVSEG_OK; c++) st = rvseg_crf_model_set_kernel(ctx_, changed[c], terms_[(size_t)changed[c]].kp.data());
            return st;
        });
    }
    // CRFEnergy::gradient (dense_learning.cpp:60-84) as one rvseg_crf_model_energy_gradient: x (the learned groups in the order
    // unary | label compatibility | kernel) becomes this object's parameters and the live model's, dx receives the negated
    // gradient plus l2_norm x, the value returned is the negated objective plus the L2 term (definitions in rvseg.h)
    double energyGradient(int n_iterations, const ObjectiveFunction& objective, bool unary, bool pairwise, bool kernel, float l2_norm,
                          const std::vector<float>& x, std::vector<float>& dx) {
        check(objective.gt.size() == (size_t)N_ && (objective.kind != RVSEG_OBJECTIVE_HAMMING || objective.class_weight.size() == (size_t)M_));
        const size_t nu = unary ? unaryParameters().size() : 0, nc = pairwise ? labelCompatibilityParameters().size() : 0,
                     nk = kernel ? kernelParameters().size() : 0;
        check(x.size() == nu + nc + nk);
        const rvseg_crf_objective rec = objective.record();
        double value = 0;
        dx.assign(x.size() + 1, 0.f);
        try {
            if (nu) assignUnary(x.data(), nu);
            if (pairwise) assignCompat(x.data() + nu, nc);
            if (kernel) assignKernel(x.data() + nu + nc, nk);
            const int32_t mask = (unary ? 1 : 0) | (pairwise ? 2 : 0) | (kernel ? 4 : 0);
            onModel([&] { return rvseg_crf_model_energy_gradient(ctx_, n_iterations, &rec, mask, l2_norm, x.data(), (int32_t)x.size(), &value, dx.data()); });
        } catch (...) {
            model_serial_ = 0;   // the model may hold a part of x only
            throw;
        }
        dx.pop_back();
        return value;
    }
    // DenseCRF::inference (densecrf.cpp:115-131); map_out (optional) = DenseCRF::map (:132-137).  A logistic unary is
    // computed on the GPU and read back (N x M floats), then uploaded with the model like a constant unary; callers that
    // keep everything in device memory use rvseg_crf_logistic_unary_device + rvseg_crf_infer_terms_device instead.
    std::vector<float> inference(int n_iterations, std::vector<int8_t>* map_out = nullptr) {
        const size_t N = (size_t)N_;
        std::vector<float> U;
        const float* u = unaryEnergyMatrix(U);
        std::vector<float> Q(N * M_);
        if (map_out) map_out->resize(N);
        int8_t* mp = map_out ? map_out->data() : nullptr;
        bool plain = true;
        for (const auto& t : terms_) plain = plain && t.bare && t.normalization == RVSEG_NORMALIZE_SYMMETRIC && t.kp.empty();
        if (plain) {
            std::vector<const float*> fp;
            std::vector<int32_t> ds;
            std::vector<float> ws;
            for (const auto& t : terms_) { fp.push_back(t.f.data()); ds.push_back(t.d); ws.push_back(t.compat.params[0]); }
            status(rvseg_crf_infer_multi(ctx_, (int32_t)N, M_, (int32_t)fp.size(), ds.data(), fp.data(), ws.data(), u, n_iterations,
                                         Q.data(), mp, RVSEG_LABEL_ARGMAX, 0));
            return Q;
        }
        const std::vector<rvseg_crf_term> tt = termRecords();
        status(rvseg_crf_infer_terms(ctx_, (int32_t)N, M_, (int32_t)tt.size(), tt.data(), u, n_iterations, Q.data(), mp,
                                     RVSEG_LABEL_ARGMAX, 0));
        return Q;
    }
    std::vector<int8_t> map(int n_iterations) {   // densecrf.cpp:132-137
        std::vector<int8_t> m;
        inference(n_iterations, &m);
        return m;
    }
    // ---- stepwise inference, energies and KL divergence (densecrf.h:77-94) on a model the context keeps
    // (rvseg_crf_model_*): set by the first of these calls, again after any add* / set* call, and again when the context
    // keeps another model or none (modelIsLive).  Q: N x M point-major.
    std::vector<float> startInference() {   // densecrf.cpp:178-186
        std::vector<float> Q((size_t)N_ * M_);
        onModel([&] { return rvseg_crf_model_start(ctx_, Q.data()); });
        return Q;
    }
    void stepInference(std::vector<float>& Q, int n_steps = 1) {   // densecrf.cpp:187-201
        check(Q.size() == (size_t)N_ * M_);
        onModel([&] { return rvseg_crf_model_step(ctx_, Q.data(), n_steps); });
    }
    std::vector<int8_t> currentMap(const std::vector<float>& Q) {   // densecrf.cpp:202-211
        check(Q.size() == (size_t)N_ * M_);
        std::vector<int8_t> m((size_t)N_);
        status(rvseg_label_values(ctx_, Q.data(), N_, M_, RVSEG_LABEL_ARGMAX, 0, m.data()));
        return m;
    }
    std::vector<float> unaryEnergy(const std::vector<int8_t>& l) {   // densecrf.cpp:141-153
        check(l.size() == (size_t)N_);
        std::vector<float> r((size_t)N_);
        onModel([&] { return rvseg_crf_model_energy(ctx_, l.data(), -1, r.data(), nullptr); });
        return r;
    }
    std::vector<float> pairwiseEnergy(const std::vector<int8_t>& l, int term = -1) {   // densecrf.cpp:154-177
        check(l.size() == (size_t)N_);
        std::vector<float> r((size_t)N_);
        onModel([&] { return rvseg_crf_model_energy(ctx_, l.data(), term, nullptr, r.data()); });
        return r;
    }
    // densecrf.cpp:214-235; parts (optional): entropy, unary, one per term -- the value returned is their sum in that order
    double klDivergence(const std::vector<float>& Q, std::vector<double>* parts = nullptr) {
        check(Q.size() == (size_t)N_ * M_);
        std::vector<double> p(2 + terms_.size());
        onModel([&] { return rvseg_crf_model_kl(ctx_, Q.data(), p.data()); });
        double kl = 0;
        for (double v : p) kl += v;
        if (parts) *parts = p;
        return kl;
    }
    // inference(n) with the KL divergence after the start and after every iteration (kl: n + 1 values)
    std::vector<float> inferenceTrace(int n_iterations, std::vector<double>& kl, std::vector<int8_t>* map_out = nullptr) {
        std::vector<float> Q((size_t)N_ * M_);
        kl.assign((size_t)n_iterations + 1, 0.0);
        if (map_out) map_out->resize((size_t)N_);
        onModel([&] { return rvseg_crf_model_trace(ctx_, n_iterations, Q.data(), map_out ? map_out->data() : nullptr, RVSEG_LABEL_ARGMAX, 0, kl.data()); });
        return Q;
    }
    // ---- learning (densecrf.cpp:238-297) on the kept model; rvseg::minimizeLBFGS below minimises an EnergyFunction over it
    std::vector<float> applyTranspose(int term, const std::vector<float>& in) {   // pairwise.cpp:179-183
        check(in.size() == (size_t)N_ * M_);
        std::vector<float> out((size_t)N_ * M_);
        onModel([&] { return rvseg_crf_model_apply_transpose(ctx_, term, in.data(), out.data()); });
        return out;
    }
    // PairwisePotential::kernelGradient(b, Q) (pairwise.cpp:202-207): kernel_->gradient(b, compatibility(Q)), the layout of
    // the term's kernel parameters, rounded to fp32 from the library's doubles
    std::vector<float> kernelGradient(int term, const std::vector<float>& b, const std::vector<float>& Q) {
        check(term >= 0 && term < (int)terms_.size() && b.size() == (size_t)N_ * M_ && Q.size() == b.size());
        std::vector<float> lbl_Q(Q.size());
        std::vector<double> g(kernelParams(terms_[(size_t)term]).size() + 1);
        onModel([&] {
            const rvseg_status st = rvseg_crf_model_compat_apply(ctx_, term, Q.data(), lbl_Q.data());
            return st != RVSEG_OK ? st : rvseg_crf_model_kernel_gradient(ctx_, term, b.data(), lbl_Q.data(), g.data(), nullptr);
        });
        return std::vector<float>(g.begin(), g.end() - 1);
    }
    // DenseCRF::gradient: the objective's value; unary_grad (optional) the gradient of unaryParameters() (empty without a
    // logistic unary), lbl_cmp_grad (optional) that of labelCompatibilityParameters(), both rounded to fp32 from the
    // library's doubles; unary_energy_grad (optional): d value / d U, N x M; kernel_grad (optional): the gradient of
    // kernelParameters(), rounded to fp32 from the library's doubles
    double gradient(int n_iterations, const ObjectiveFunction& objective, std::vector<float>* unary_grad, std::vector<float>* lbl_cmp_grad,
                    std::vector<float>* unary_energy_grad = nullptr, std::vector<float>* kernel_grad = nullptr) {
        check(objective.gt.size() == (size_t)N_ && (objective.kind != RVSEG_OBJECTIVE_HAMMING || objective.class_weight.size() == (size_t)M_));
        const rvseg_crf_objective rec = objective.record();
        double value = 0;
        std::vector<float> ug((size_t)N_ * M_);
        std::vector<double> cg(labelCompatibilityParameters().size() + 1), kg(kernelParameters().size() + 1), lg((size_t)M_ * K_);
        double* const cgp = lbl_cmp_grad ? cg.data() : nullptr;
        double* const kgp = kernel_grad ? kg.data() : nullptr;
        const bool logistic = unary_grad && !logistic_f_.empty();
        const bool params = logistic && !unary_energy_grad;   // the parameters' doubles alone come back
        const bool want_ug = unary_grad || unary_energy_grad;
        onModel([&] {
            return params ? rvseg_crf_model_gradient_params(ctx_, n_iterations, &rec, &value, lg.data(), cgp, kgp)
                          : rvseg_crf_model_gradient_kernel(ctx_, n_iterations, &rec, &value, want_ug ? ug.data() : nullptr, cgp, kgp, nullptr);
        });
        if (logistic && !params) status(rvseg_crf_logistic_gradient(ctx_, N_, M_, K_, ug.data(), logistic_f_.data(), lg.data()));
        if (unary_grad) unary_grad->assign(lg.begin(), logistic ? lg.end() : lg.begin());
        if (lbl_cmp_grad) lbl_cmp_grad->assign(cg.begin(), cg.end() - 1);
        if (kernel_grad) kernel_grad->assign(kg.begin(), kg.end() - 1);
        if (unary_energy_grad) *unary_energy_grad = std::move(ug);
        return value;
    }
protected:
    struct Term {
        std::vector<float> f;
        int d = 0, kernel_type = RVSEG_DIAG_KERNEL, normalization = RVSEG_NORMALIZE_SYMMETRIC;
        LabelCompatibility compat;
        bool bare = false;        // added as a bare Potts weight
        std::vector<float> kp;    // kernel parameters set by setKernelParameters (empty: the features as added)
    };
    void addTerm(const float* features, int d, const LabelCompatibility& c, int kernel_type, int normalization, bool bare) {
        // the library reads 1, M or M x M compatibility values: a compatibility built for another class count is refused here
        const size_t want = c.kind == RVSEG_COMPAT_POTTS ? 1 : c.kind == RVSEG_COMPAT_DIAGONAL ? (size_t)M_ : (size_t)M_ * M_;
        if (c.params.size() != want || (c.kind == RVSEG_COMPAT_MATRIX && c.M != M_))
            throw std::runtime_error("label compatibility does not match the class count");
        model_serial_ = 0;
        Term t;
        t.f.assign(features, features + (size_t)N_ * d);
        t.d = d; t.compat = c; t.kernel_type = kernel_type; t.normalization = normalization; t.bare = bare;
        terms_.push_back(std::move(t));
    }
    static std::vector<float> kernelParams(const Term& t) {
        if (t.kernel_type == RVSEG_CONST_KERNEL) return {};
        if (!t.kp.empty()) return t.kp;
        std::vector<float> p(t.kernel_type == RVSEG_DIAG_KERNEL ? t.d : t.d * t.d, t.kernel_type == RVSEG_DIAG_KERNEL ? 1.f : 0.f);
        if (t.kernel_type == RVSEG_FULL_KERNEL) for (int i = 0; i < t.d; i++) p[(size_t)i * t.d + i] = 1.f;
        return p;
    }
    static void check(bool ok) { if (!ok) throw std::runtime_error("bad parameter vector"); }
    // the parameters of this object alone (no model call); assignKernel returns the terms whose values changed
    void assignUnary(const float* v, size_t n) {
        check(n == logistic_L_.size());
        for (int k = 0; k < K_; k++)
            for (int m = 0; m < M_; m++) logistic_L_[(size_t)m * K_ + k] = v[(size_t)k * M_ + m];
    }
    void assignCompat(const float* v, size_t n_all) {
        size_t i = 0;
        for (auto& t : terms_) {
            const size_t n = t.compat.parameters().size();
            check(i + n <= n_all);
            t.compat.setParameters(v + i);
            t.bare = false;
            i += n;
        }
        check(i == n_all);
    }
    std::vector<int> assignKernel(const float* v, size_t n_all) {
        std::vector<int> changed;
        size_t i = 0;
        for (size_t k = 0; k < terms_.size(); k++) {
            Term& t = terms_[k];
            const size_t n = kernelParams(t).size();
            check(i + n <= n_all);
            if (t.kernel_type != RVSEG_CONST_KERNEL) {
                if (t.kp.size() != n || std::memcmp(t.kp.data(), v + i, n * sizeof(float)) != 0) changed.push_back((int)k);
                t.kp.assign(v + i, v + i + n);
            }
            i += n;
        }
        check(i == n_all);
        return changed;
    }
    // Whether the context's live model is the one this object set.  The context has one model and no handle for it, so
    // objects that share a context take turns, and anybody may set a model on it directly: the library's serial tells.
    // Check-then-call needs no lock of its own: a context is not safe for concurrent calls in the first place.
    bool modelIsLive() const {
        struct rvseg_crf_model_info info;
        return model_serial_ != 0 && rvseg_crf_model_info(ctx_, &info) == RVSEG_OK && info.serial == model_serial_;
    }
    // a parameter change on the live model of this object; without one the next onModel sets the model
    template <class F>
    void inPlace(F&& update) {
        if (!modelIsLive()) { model_serial_ = 0; return; }
        const rvseg_status st = update();
        if (st != RVSEG_OK) model_serial_ = 0;
        status(st);
    }
    // the unary energy as N x M values: the constant one, the logistic one computed on the GPU into U, or zeros in U
    const float* unaryEnergyMatrix(std::vector<float>& U) {
        const size_t N = (size_t)N_;
        if (!logistic_f_.empty()) {
            U.resize(N * M_);
            status(rvseg_crf_logistic_unary(ctx_, N_, M_, K_, logistic_L_.data(), logistic_f_.data(), U.data()));
        } else if (unary_.empty()) {
            U.assign(N * M_, 0.f);
        }
        return unary_.empty() ? U.data() : unary_.data();
    }
    std::vector<rvseg_crf_term> termRecords() const {
        std::vector<rvseg_crf_term> tt;
        for (const auto& t : terms_) {
            rvseg_crf_term r{};
            r.d = t.d; r.compat = t.compat.kind; r.kernel_type = t.kernel_type; r.normalization = t.normalization;
            r.features = t.f.data(); r.compat_params = t.compat.params.data();
            r.kernel_params = t.kp.empty() ? nullptr : t.kp.data();
            tt.push_back(r);
        }
        return tt;
    }
    // runs a model call, (re)setting the context's model first when this object changed or the context keeps another model
    template <class F>
    void onModel(F&& call) {
        if (!modelIsLive()) {
            model_serial_ = 0;   // (a failure below leaves no model of this object)
            std::vector<float> U;
            const std::vector<rvseg_crf_term> tt = termRecords();
            if (!logistic_f_.empty()) U.assign((size_t)N_ * M_, 0.f);   // the model computes L f itself and keeps f
            status(rvseg_crf_model_set(ctx_, N_, M_, (int32_t)tt.size(), tt.data(), logistic_f_.empty() ? unaryEnergyMatrix(U) : U.data(), 1));
            if (!logistic_f_.empty()) status(rvseg_crf_model_set_logistic(ctx_, K_, logistic_L_.data(), logistic_f_.data()));
            struct rvseg_crf_model_info info;
            status(rvseg_crf_model_info(ctx_, &info));
            model_serial_ = info.serial;
        }
        status(call());
    }
    uint64_t model_serial_ = 0;   // the serial of the model this object set (rvseg_crf_model_info); 0: none, or changed since
    void status(rvseg_status st) {
        if (st != RVSEG_OK) throw std::runtime_error(std::string(rvseg_status_string(st)) + ": " + rvseg_last_error(ctx_));
    }
    rvseg_ctx* ctx_;
    int N_, M_, K_ = 0;
    std::vector<float> unary_, logistic_L_, logistic_f_;
    std::vector<Term> terms_;
};

// DenseCRF2D as examples/dense_inference.cpp:83-107 and examples/dense_learning.cpp:128-182 drive it: the two image kernels
// (features by rvseg_crf_features_*), then map().
class DenseCRF2D : public DenseCRF {
public:
    DenseCRF2D(rvseg_ctx* ctx, int W, int H, int M) : DenseCRF(ctx, W * H, M), W_(W), H_(H) {}
    void addPairwiseGaussian(float sx, float sy, float potts_w) {                                   // densecrf.cpp:61-69
        const auto f = gaussian(sx, sy);
        addPairwiseEnergy(f.data(), 2, potts_w);
    }
    void addPairwiseGaussian(float sx, float sy, const LabelCompatibility& function, int kernel_type = RVSEG_DIAG_KERNEL,
                             int normalization = RVSEG_NORMALIZE_SYMMETRIC) {
        const auto f = gaussian(sx, sy);
        addPairwiseEnergy(f.data(), 2, function, kernel_type, normalization);
    }
    void addPairwiseBilateral(float sx, float sy, float sr, float sg, float sb, const unsigned char* im, float potts_w) {   // :70-81
        const auto f = bilateral(sx, sy, sr, sg, sb, im);
        addPairwiseEnergy(f.data(), 5, potts_w);
    }
    void addPairwiseBilateral(float sx, float sy, float sr, float sg, float sb, const unsigned char* im, const LabelCompatibility& function,
                              int kernel_type = RVSEG_DIAG_KERNEL, int normalization = RVSEG_NORMALIZE_SYMMETRIC) {
        const auto f = bilateral(sx, sy, sr, sg, sb, im);
        addPairwiseEnergy(f.data(), 5, function, kernel_type, normalization);
    }
private:
    std::vector<float> gaussian(float sx, float sy) const {
        std::vector<float> f((size_t)W_ * H_ * 2);
        if (rvseg_crf_features_gaussian(W_, H_, sx, sy, f.data()) != RVSEG_OK) throw std::runtime_error("bad arguments");
        return f;
    }
    std::vector<float> bilateral(float sx, float sy, float sr, float sg, float sb, const unsigned char* im) const {
        std::vector<float> f((size_t)W_ * H_ * 5);
        if (rvseg_crf_features_bilateral(W_, H_, sx, sy, sr, sg, sb, im, f.data()) != RVSEG_OK) throw std::runtime_error("bad arguments");
        return f;
    }
    int W_, H_;
};

// ---- scoring: RgbLabelConversion (include/rgb_label_conversion.h) and the score block of src/test.cpp:182-228 --------
// One entry of config.json color_codings[l].coding, negative labels included (LabelClass above keeps only classes >= 0).
struct ColorCodingEntry {
    std::string name;
    std::array<uint8_t, 3> color;   // r, g, b
    int label;                      // stored as label_type = char (include/defines.h)
};

// Binds one layer's coding to a context (rvseg_color_coding_set; a later rvseg_forest_load discards it).  Images are
// the context's H x W in R, G, B byte order; conversions run on the GPU (host buffers, staged by the library).
class RgbLabelConversion {
public:
    RgbLabelConversion(rvseg_ctx* ctx, const std::vector<ColorCodingEntry>& coding, int layer = 0, int8_t missing_label = 0)
        : ctx_(ctx), layer_(layer) {
        std::vector<uint8_t> rgb;
        std::vector<int8_t> labels;
        for (const ColorCodingEntry& e : coding) {   // std::map assignments in entry order (:29-38)
            const int8_t l = (int8_t)e.label;
            rgb.insert(rgb.end(), e.color.begin(), e.color.end());
            labels.push_back(l);
            name_to_label_[e.name] = l;
            label_to_name_[l] = e.name;
        }
        check(rvseg_color_coding_set(ctx_, layer_, (int32_t)labels.size(), rgb.data(), labels.data(), missing_label));
    }
    void rgbToLabel(const uint8_t* rgb, int8_t* labels, int n_images = 1) { check(rvseg_labels_from_rgb(ctx_, layer_, n_images, rgb, labels)); }   // :59-78
    void labelToRgb(const int8_t* labels, uint8_t* rgb, int n_images = 1) { check(rvseg_labels_to_rgb(ctx_, layer_, n_images, labels, rgb)); }     // :42-57
    std::string getLabelName(int8_t label) const {                  // :91-93
        auto it = label_to_name_.find(label);
        return it == label_to_name_.end() ? std::string() : it->second;
    }
    int8_t getLabelNumber(const std::string& name) const {          // :95-97
        auto it = name_to_label_.find(name);
        return it == name_to_label_.end() ? 0 : it->second;
    }
    int getValidLabelCount() const {                                // :103-110
        int n = 0;
        for (const auto& kv : label_to_name_) n += kv.first >= 0;
        return n;
    }
private:
    void check(rvseg_status st) const {
        if (st != RVSEG_OK) throw std::runtime_error(std::string(rvseg_status_string(st)) + ": " + rvseg_last_error(ctx_));
    }
    rvseg_ctx* ctx_;
    int layer_;
    std::map<std::string, int8_t> name_to_label_;
    std::map<int8_t, std::string> label_to_name_;
};

// The confusion matrices of every label layer of a context, accumulated on the GPU (uint64), and the reference's scores.
struct EvalScores {
    double global_acc;      // NaN before anything was counted, as the reference prints it
    float class_avg_acc;
    float iou;
    std::vector<double> row_pct;   // C x C, the printed table
};

class Evaluator {
public:
    // codings: one per label layer of the loaded model; an empty coding leaves that layer to int8 ground truth
    Evaluator(rvseg_ctx* ctx, const std::vector<std::vector<ColorCodingEntry>>& codings, int8_t missing_label = 0) : ctx_(ctx) {
        int32_t n_layers = 0, cc[RVSEG_MAX_LAYERS];
        check(rvseg_forest_info(ctx_, nullptr, nullptr, nullptr, &n_layers, cc));
        if ((size_t)n_layers != codings.size()) throw std::runtime_error("one colour coding per label layer");
        class_counts_.assign(cc, cc + n_layers);
        for (int l = 0; l < n_layers; l++)
            conv_.emplace_back(codings[l].empty() ? nullptr : new RgbLabelConversion(ctx_, codings[l], l, missing_label));
        reset();
    }
    void reset() { check(rvseg_eval_reset(ctx_)); }
    // pred: n x L x H x W int8 (labels_out); gt: the same int8 layout (RVSEG_GT_LABELS) or x 3 bytes (RVSEG_GT_RGB)
    void add(int n_frames, const int8_t* pred, const void* gt, int gt_format = RVSEG_GT_LABELS) {
        check(rvseg_eval_accumulate(ctx_, n_frames, pred, gt, gt_format));
    }
    void addDevice(int n_frames, const int8_t* d_pred, const void* d_gt, int gt_format, void* hip_stream) {
        check(rvseg_eval_accumulate_device(ctx_, n_frames, d_pred, d_gt, gt_format, hip_stream));
    }
    std::vector<uint64_t> confusion(int layer, uint64_t* out_of_range = nullptr) {
        std::vector<uint64_t> c((size_t)class_counts_.at(layer) * class_counts_.at(layer));
        check(rvseg_eval_confusion(ctx_, layer, c.data(), out_of_range));
        return c;
    }
    EvalScores scores(int layer) {
        const std::vector<uint64_t> c = confusion(layer);
        const int C = class_counts_.at(layer);
        EvalScores s;
        s.row_pct.resize((size_t)C * C);
        check(rvseg_eval_scores_from_counts(c.data(), C, &s.global_acc, &s.class_avg_acc, &s.iou, s.row_pct.data()));
        return s;
    }
    // the text test.cpp:206-228 prints
    std::string report(int layer) {
        const std::vector<uint64_t> c = confusion(layer);
        const EvalScores s = scores(layer);
        const int C = class_counts_.at(layer);
        std::string out = "confusion:\n";
        char buf[64];
        for (int i = 0; i < C; i++) {
            std::string n = conv_[layer] ? conv_[layer]->getLabelName((int8_t)i) : std::string();
            for (int p = (int)n.length(); p < 15; p++) n += " ";
            out += n;
            uint64_t row = 0;
            for (int j = 0; j < C; j++) {
                std::snprintf(buf, sizeof(buf), " %6.2f", s.row_pct[(size_t)i * C + j]);
                out += buf;
                row += c[(size_t)i * C + j];
            }
            out += "   out of " + std::to_string(row) + " pixels\n";
        }
        std::snprintf(buf, sizeof(buf), "Global accuracy:         %6.2f \n", s.global_acc);
        out += buf;
        std::snprintf(buf, sizeof(buf), "Class averge accuracy:   %6.2f \n", s.class_avg_acc);
        out += buf;
        std::snprintf(buf, sizeof(buf), "Intersection over union: %6.2f \n", s.iou);
        out += buf;
        return out;
    }
    RgbLabelConversion* conversion(int layer) { return conv_.at(layer).get(); }
private:
    void check(rvseg_status st) const {
        if (st != RVSEG_OK) throw std::runtime_error(std::string(rvseg_status_string(st)) + ": " + rvseg_last_error(ctx_));
    }
    rvseg_ctx* ctx_;
    std::vector<int> class_counts_;
    std::vector<std::unique_ptr<RgbLabelConversion>> conv_;
};

// EnergyFunction / minimizeLBFGS of optimization.h / optimization.cpp:68-103 over rvseg_minimize_lbfgs: epsilon = 1e-6, at
// most 50 iterations per run, up to restart + 1 runs, ending after the first whose value is not below the lowest before it.
// x crosses to the energy as float (the reference's VectorXf).  An energy that is not finite, or whose gradient has another
// size than x, ends the loop with std::runtime_error.
class EnergyFunction {
public:
    virtual ~EnergyFunction() {}
    virtual std::vector<float> initialValue() = 0;
    virtual double gradient(const std::vector<float>& x, std::vector<float>& dx) = 0;
};

inline std::vector<float> minimizeLBFGS(EnergyFunction& efun, int restart = 0, bool verbose = false, const rvseg_lbfgs_params* params = nullptr) {
    std::vector<float> x0 = efun.initialValue();
    const int32_t n = (int32_t)x0.size();
    if (n == 0) return x0;
    std::vector<double> x(x0.begin(), x0.end());
    const rvseg_energy_fn evaluate = [](void* user, const double* xd, double* g, int32_t m) -> double {
        std::vector<float> vx(xd, xd + m), vg;
        const double r = static_cast<EnergyFunction*>(user)->gradient(vx, vg);
        if ((int32_t)vg.size() != m) return std::numeric_limits<double>::quiet_NaN();   // ends the run: RVSEG_LBFGS_NOT_FINITE
        for (int32_t i = 0; i < m; i++) g[i] = (double)vg[i];
        return r;
    };
    const rvseg_progress_fn progress = [](void*, const double*, const double*, double fx, double xnorm, double gnorm, double step, int32_t,
                                          int32_t k, int32_t) -> int32_t {
        std::printf("Iteration %d:\n  fx = %f, xnorm = %f, gnorm = %f, step = %f\n\n", k, fx, xnorm, gnorm, step);
        return 0;
    };
    rvseg_lbfgs_params param;
    rvseg_lbfgs_params_default(&param);
    param.epsilon = 1e-6;
    param.max_iterations = 50;
    if (params) param = *params;   // (the caller's instead of the reference's two settings)
    rvseg_lbfgs_report rep{};
    double last_f = 1e100;
    for (int i = 0; i <= restart; i++) {
        double fx = 0.0;
        if (rvseg_minimize_lbfgs(n, x.data(), &fx, evaluate, verbose ? progress : nullptr, &efun, &param, &rep) != RVSEG_OK)
            throw std::runtime_error("minimizeLBFGS: the energy returned a value or a gradient that is not finite, or a gradient of another "
                                     "size than x (rvseg_lbfgs_status " + std::to_string(rep.status) + ")");
        if (last_f > fx) last_f = fx;
        else break;
    }
    if (verbose) std::printf("L-BFGS optimization terminated with status code = %d\n", rep.status);
    for (int32_t i = 0; i < n; i++) x0[i] = (float)x[i];
    return x0;
}

// The EnergyFunction of examples/dense_learning.cpp:38-85 over a DenseCRF: the learned groups of x are the unary, the label
// compatibility and the kernel parameters; one evaluation is one DenseCRF::energyGradient.
class CRFEnergy : public EnergyFunction {
public:
    CRFEnergy(DenseCRF& crf, const ObjectiveFunction& objective, int NIT, bool unary = true, bool pairwise = true, bool kernel = true)
        : crf_(crf), objective_(objective), NIT_(NIT), unary_(unary), pairwise_(pairwise), kernel_(kernel),
          initial_u_param_(crf.unaryParameters()), initial_lbl_param_(crf.labelCompatibilityParameters()),
          initial_knl_param_(crf.kernelParameters()) {}
    void setL2Norm(float norm) { l2_norm_ = norm; }
    std::vector<float> initialValue() override {
        std::vector<float> p;
        if (unary_) p.insert(p.end(), initial_u_param_.begin(), initial_u_param_.end());
        if (pairwise_) p.insert(p.end(), initial_lbl_param_.begin(), initial_lbl_param_.end());
        if (kernel_) p.insert(p.end(), initial_knl_param_.begin(), initial_knl_param_.end());
        return p;
    }
    double gradient(const std::vector<float>& x, std::vector<float>& dx) override {
        return crf_.energyGradient(NIT_, objective_, unary_, pairwise_, kernel_, l2_norm_, x, dx);
    }
protected:
    DenseCRF& crf_;
    const ObjectiveFunction& objective_;
    int NIT_;
    bool unary_, pairwise_, kernel_;
    float l2_norm_ = 0.f;
    std::vector<float> initial_u_param_, initial_lbl_param_, initial_knl_param_;
};

// libf::BoostedRandomForest (classifiers.h:349-425) over a context with multi_layer = 0: T trees and a weight per tree.
// The stream's order is named by the caller (rvseg_boosted_order): the reference's write puts the weight before the tree,
// its read expects it after.
class BoostedRandomForest {
public:
    explicit BoostedRandomForest(rvseg_ctx* ctx) : ctx_(ctx) {}
    void read(const std::string& path, rvseg_boosted_order order = RVSEG_BOOSTED_WEIGHT_FIRST) { check(rvseg_boosted_load(ctx_, path.c_str(), order)); }   // classifier.cpp:264
    void read(const void* buf, size_t size, rvseg_boosted_order order = RVSEG_BOOSTED_WEIGHT_FIRST) { check(rvseg_boosted_load_mem(ctx_, buf, size, order)); }
    void write(const std::string& path, rvseg_boosted_order order = RVSEG_BOOSTED_AS_LOADED) const { check(rvseg_boosted_write(ctx_, path.c_str(), order)); }   // :250
    std::vector<uint8_t> write(rvseg_boosted_order order = RVSEG_BOOSTED_AS_LOADED) const {
        size_t size = 0;
        check(rvseg_boosted_write_mem(ctx_, order, nullptr, 0, &size));
        std::vector<uint8_t> out(size);
        check(rvseg_boosted_write_mem(ctx_, order, out.data(), out.size(), &size));
        return out;
    }
    int getSize() const {
        int32_t n = 0;
        check(rvseg_boosted_weights(ctx_, nullptr, 0, &n, nullptr));
        return n;
    }
    std::vector<float> getWeights() const {
        std::vector<float> w((size_t)getSize());
        int32_t n = 0;
        check(rvseg_boosted_weights(ctx_, w.data(), (int32_t)w.size(), &n, nullptr));
        return w;
    }
    // the weighted votes per class of P points (X: P x D), P x C (:283-302)
    std::vector<float> classLogPosterior(const float* X, int P, int D) const {
        int32_t n_layers = 0, cc[RVSEG_MAX_LAYERS];
        check(rvseg_forest_info(ctx_, nullptr, nullptr, nullptr, &n_layers, cc));
        std::vector<float> out((size_t)P * cc[0]);
        check(rvseg_forest_eval(ctx_, X, P, D, out.data()));
        return out;
    }
    // Classifier::classify (:29-51): the first class with the strictly greatest vote sum
    std::vector<int> classify(const float* X, int P, int D) const {
        const std::vector<float> post = classLogPosterior(X, P, D);
        const size_t C = P ? post.size() / (size_t)P : 0;
        std::vector<int> label((size_t)P, 0);
        for (int p = 0; p < P; p++) {
            float prob = post[(size_t)p * C];
            for (size_t c = 1; c < C; c++)
                if (post[(size_t)p * C + c] > prob) { label[(size_t)p] = (int)c; prob = post[(size_t)p * C + c]; }
        }
        return label;
    }
private:
    void check(rvseg_status st) const {
        if (st != RVSEG_OK) throw std::runtime_error(std::string(rvseg_status_string(st)) + ": " + rvseg_last_error(ctx_));
    }
    rvseg_ctx* ctx_;
};

// libforest tools.h on the model a context has loaded (RandomForest or BoostedRandomForest): X is P x D, labels P class
// indices of `layer` (rvseg.h, "forest tools").  The counts come from one pass on the device, the floats from the
// reference's arithmetic on them.
namespace tools_detail {
inline void check(rvseg_ctx* ctx, rvseg_status st) {
    if (st != RVSEG_OK) throw std::runtime_error(std::string(rvseg_status_string(st)) + ": " + rvseg_last_error(ctx));
}
inline int class_count(rvseg_ctx* ctx, int layer, int* n_trees = nullptr) {
    int32_t T = 0, n_layers = 0, cc[RVSEG_MAX_LAYERS];
    check(ctx, rvseg_forest_info(ctx, &T, nullptr, nullptr, &n_layers, cc));
    if (n_trees) *n_trees = T;
    if (layer < 0 || layer >= n_layers) throw std::runtime_error("layer outside the layers of the context's active mode");
    return cc[layer];
}
inline std::vector<std::vector<float>> rows_of(const std::vector<float>& flat, int n) {
    std::vector<std::vector<float>> out((size_t)n);
    for (int r = 0; r < n; r++) out[(size_t)r].assign(flat.begin() + (size_t)r * n, flat.begin() + (size_t)(r + 1) * n);
    return out;
}
}  // namespace tools_detail

class AccuracyTool {   // tools.cpp:61-89
public:
    float measure(rvseg_ctx* classifier, const float* X, int P, int D, const int32_t* labels, int layer = 0) const {
        const int C = tools_detail::class_count(classifier, layer);
        std::vector<uint64_t> conf((size_t)C * C);
        tools_detail::check(classifier, rvseg_forest_measure(classifier, X, P, D, labels, layer, nullptr, conf.data(), nullptr));
        float accuracy = 0.f;
        tools_detail::check(classifier, rvseg_forest_tools_scores(conf.data(), C, &accuracy, nullptr));
        return accuracy;
    }
    void print(float accuracy) const { std::printf("Accuracy: %2.2f%% (Error: %2.2f%%)\n", accuracy * 100, (1 - accuracy) * 100); }
};

class ConfusionMatrixTool {   // tools.cpp:95-186; rows are true classes, a class without examples is a NaN row
public:
    std::vector<std::vector<float>> measure(rvseg_ctx* classifier, const float* X, int P, int D, const int32_t* labels, int layer = 0) const {
        const int C = tools_detail::class_count(classifier, layer);
        std::vector<uint64_t> conf((size_t)C * C);
        tools_detail::check(classifier, rvseg_forest_measure(classifier, X, P, D, labels, layer, nullptr, conf.data(), nullptr));
        std::vector<float> norm((size_t)C * C);
        tools_detail::check(classifier, rvseg_forest_tools_scores(conf.data(), C, nullptr, norm.data()));
        return tools_detail::rows_of(norm, C);
    }
    void print(const std::vector<std::vector<float>>& result) const {   // without the colour codes
        const int C = (int)result.size();
        std::printf("        |");
        for (int c = 0; c < C; c++) std::printf(" %6d |", c);
        std::printf("\n");
        for (int c = 0; c < C + 1; c++) std::printf("--------|");
        std::printf("\n");
        for (int c = 0; c < C; c++) {
            std::printf(" %6d |", c);
            for (int cc = 0; cc < C; cc++) std::printf(" %5.2f%% |", result[(size_t)c][(size_t)cc] * 100);
            std::printf("\n");
            for (int k = 0; k < C + 1; k++) std::printf("--------|");
            std::printf("\n");
        }
    }
};

class CorrelationTool {   // tools.cpp:192-263
public:
    std::vector<std::vector<float>> measure(rvseg_ctx* forest, const float* X, int P, int D, int layer = 0) const {
        int T = 0;
        tools_detail::class_count(forest, layer, &T);
        std::vector<uint64_t> agree((size_t)T * T);
        tools_detail::check(forest, rvseg_forest_measure(forest, X, P, D, nullptr, layer, nullptr, nullptr, agree.data()));
        std::vector<float> corr((size_t)T * T);
        tools_detail::check(forest, rvseg_forest_tools_correlation(agree.data(), T, (uint64_t)P, corr.data()));
        return tools_detail::rows_of(corr, T);
    }
    void print(const std::vector<std::vector<float>>& result) const {
        const int C = (int)result.size();
        std::printf("         |");
        for (int c = 0; c < C; c++) std::printf(" %7d |", c);
        std::printf("\n");
        for (int c = 0; c < C + 1; c++) std::printf("---------|");
        std::printf("\n");
        for (int c = 0; c < C; c++) {
            std::printf(" %7d |", c);
            for (int cc = 0; cc < C; cc++) std::printf(" %6.2f%% |", result[(size_t)c][(size_t)cc] * 100);
            std::printf("\n");
            for (int k = 0; k < C + 1; k++) std::printf("---------|");
            std::printf("\n");
        }
    }
};

// DecisionTreeLearner::updateHistograms / updateMultiHistograms (learning.cpp:918-1012) on the loaded RandomForest: the
// forest.dat image of the same trees with their leaves re-estimated from (X, labels: P x class_counts.size()).
inline std::vector<uint8_t> refit(rvseg_ctx* forest, const float* X, int P, int D, const int32_t* labels, const std::vector<int32_t>& class_counts,
                                  float smoothing = 1.0f) {
    size_t size = 0;
    tools_detail::check(forest, rvseg_forest_refit(forest, X, P, D, labels, (int32_t)class_counts.size(), class_counts.data(), smoothing, nullptr, 0,
                                                   &size, nullptr));
    std::vector<uint8_t> out(size);
    tools_detail::check(forest, rvseg_forest_refit(forest, X, P, D, labels, (int32_t)class_counts.size(), class_counts.data(), smoothing, out.data(),
                                                   out.size(), &size, nullptr));
    return out;
}

// libf::RandomForestPrune (todos.txt:12-18, 310-350) on the RandomForest a context has loaded: simulated annealing
// (mcmc.h:147-240) over lists of its trees.  `params` holds the reference's settings (the 100 -> 1e-5 schedule at alpha
// 0.95 with 250 inner loops, the exchange move, the error energy) until changed.
class RandomForestPrune {
public:
    rvseg_prune_params params;
    std::vector<rvseg_prune_trace_row> trace;   // the last run's rows: what PruneCallback printed (todos.txt:34-44)
    RandomForestPrune() { rvseg_prune_params_default(&params); }
    // the best state found from `state` (empty: trees 0 .. min(15, T) - 1, todos.txt:336-340); the model is left as it is
    std::vector<int32_t> optimize(rvseg_ctx* forest, const float* X, int P, int D, const int32_t* labels, int layer = 0,
                                  std::vector<int32_t> state = {}, float* best_energy = nullptr) {
        int T = 0;
        tools_detail::class_count(forest, layer, &T);
        if (state.empty())
            for (int i = 0; i < 15 && i < T; i++) state.push_back(i);
        int32_t n = (int32_t)state.size(), iterations = 0, n_trace = 0;
        if (n > RVSEG_PRUNE_MAX_STATE) throw std::runtime_error("state longer than 64 entries");
        state.resize(RVSEG_PRUNE_MAX_STATE);
        if (rvseg_prune_schedule(&params, &iterations, nullptr) != RVSEG_OK) iterations = 0;   // rvseg_forest_prune says why
        trace.assign((size_t)iterations, rvseg_prune_trace_row());
        tools_detail::check(forest, rvseg_forest_prune(forest, X, P, D, labels, layer, &params, state.data(), &n, best_energy, trace.data(), iterations,
                                                       &n_trace, nullptr));
        state.resize((size_t)n);
        return state;
    }
    // RandomForestPrune::prune: optimize, then the context's model becomes the forest of the best state's trees
    // (todos.txt:343-349).  Returns that state.
    std::vector<int32_t> prune(rvseg_ctx* forest, const float* X, int P, int D, const int32_t* labels, int layer = 0, std::vector<int32_t> state = {}) {
        const std::vector<int32_t> best = optimize(forest, X, P, D, labels, layer, std::move(state));
        tools_detail::check(forest, rvseg_forest_prune_apply(forest, best.data(), (int32_t)best.size()));
        return best;
    }
    void print() const {   // PruneCallback::callback per row
        for (const rvseg_prune_trace_row& r : trace)
            std::printf("iteration: %d energy: %g best: %g temp: %g state: %d\n", r.iteration, r.energy, r.best_energy, r.temperature, r.state_size);
    }
};

}  // namespace rvseg
#endif
