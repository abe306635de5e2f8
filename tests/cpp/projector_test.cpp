// The poses path of the C++ Segmenter facade (include/rvseg_segmenter.hpp: setCameraMatrices, LocalMapNode::pose,
// projectCloud, processMapFromQueue; src/segmenter.cpp:234-240, 576-578): a queued local map whose nodes carry poses and
// no index images must store the same labels as the same map queued with the index images projectCloud returns, and a
// node with neither must throw.  The index images, the cloud and the matrices are written out for the Python side,
// which compares them with the restatement of the projector's definition.
// usage: projector_test <forest.dat> <rgb.u8> <depth.u16> <out.bin>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rvseg_segmenter.hpp"

static std::vector<uint8_t> slurp(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    std::fseek(f, 0, SEEK_END);
    long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> b((size_t)n);
    if (std::fread(b.data(), 1, b.size(), f) != b.size()) throw std::runtime_error("short read");
    std::fclose(f);
    return b;
}

#define REQUIRE(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage\n"); return 2; }
    try {
        rvseg::Config conf;
        conf.width = 160; conf.height = 120;
        conf.forest_file_name = argv[1];
        conf.max_batch = 8;
        const char* names[2] = {"material", "object"};
        const int counts[2] = {8, 9};
        for (int l = 0; l < 2; l++) {
            rvseg::Layer layer;
            layer.name = names[l];
            for (int c = 0; c < counts[l]; c++) layer.classes.push_back({"class" + std::to_string(c), {(uint8_t)c, (uint8_t)(2 * c), (uint8_t)(3 * c)}});
            layer.unknown_label = counts[l] - 1;
            conf.layers.push_back(layer);
        }
        const int W = conf.width, H = conf.height;
        const size_t N = (size_t)W * H;
        std::vector<uint8_t> rgb0 = slurp(argv[2]);
        std::vector<uint8_t> draw = slurp(argv[3]);
        REQUIRE(rgb0.size() == N * 3 && draw.size() == N * 2);
        const uint16_t* depth0 = reinterpret_cast<const uint16_t*>(draw.data());
        // two cameras (camera z forward = base x, base z up), the second one beside and above the first
        const int n_cam = 2;
        const float fx = 128.f;
        float calib[2 * 21] = {1 / fx, 0, -(W / 2.f) / fx, 0, 1 / fx, -(H / 2.f) / fx, 0, 0, 1, 0, 0, 1, -1, 0, 0, 0, -1, 0, 0, 0, 0.6f};
        std::memcpy(calib + 21, calib, 21 * sizeof(float));
        calib[21 + 19] = 0.25f; calib[21 + 20] = 0.9f;
        const float K[2 * 9] = {fx, 0, W / 2.f, 0, fx, H / 2.f, 0, 0, 1, fx, 0, W / 2.f, 0, fx, H / 2.f, 0, 0, 1};
        // a cloud in front of the cameras: a wall 2 .. 4 m ahead, 3000 points, some of them behind one another
        const size_t P = 3000;
        std::vector<float> xyz(P * 3), crgb(P * 3);
        uint32_t lcg = 12345u;
        auto unit = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) / 16777216.0f; };
        for (size_t i = 0; i < P; i++) {
            xyz[i * 3] = 2.0f + 2.0f * unit();
            xyz[i * 3 + 1] = -1.5f + 3.0f * unit();
            xyz[i * 3 + 2] = -0.2f + 2.0f * unit();
            for (int k = 0; k < 3; k++) crgb[i * 3 + k] = unit();
        }
        const float poses[2][12] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, {1, 0, 0, 0.05f, 0, 1, 0, -0.02f, 0, 0, 1, 0.01f}};

        rvseg::Segmenter seg(conf);
        seg.setCameras(n_cam, calib);
        seg.setCameraMatrices(K);
        // three rounds of the same four key frames (two nodes x two cameras) under different sequence numbers, one round per map
        auto seq_of = [&](int round, int cam, int node) { return 1000 * round + 100 * (cam + 1) + node; };
        for (int round = 0; round < 3; round++)
            for (int node = 0; node < 2; node++)
                for (int cam = 0; cam < n_cam; cam++) {
                    const int k = node * n_cam + cam;
                    std::vector<uint8_t> c(N * 3);
                    std::vector<uint16_t> d(N);
                    for (size_t i = 0; i < N; i++) {
                        const size_t j = (i + (size_t)k * 37) % N;
                        for (int ch = 0; ch < 3; ch++) c[i * 3 + ch] = (uint8_t)(rgb0[j * 3 + ch] + 5 * k);
                        d[i] = depth0[j] ? (uint16_t)(depth0[j] + 13 * k) : 0;
                    }
                    seg.enqueueFrame(cam, seq_of(round, cam, node), c.data(), d.data());
                }
        int total = 0, done;
        while ((done = seg.processFramesFromQueueInternalRF()) > 0) total += done;
        REQUIRE(total == 12);

        // the index images of the four sub-images through projectCloud, with their z-buffers
        std::vector<float> Ps;
        for (int node = 0; node < 2; node++)
            for (int cam = 0; cam < n_cam; cam++) {
                float Pm[12];
                REQUIRE(rvseg_projection_matrix(K + cam * 9, calib + cam * 21 + 9, poses[node], Pm) == RVSEG_OK);
                Ps.insert(Ps.end(), Pm, Pm + 12);
            }
        std::vector<float> zbuf;
        const std::vector<int32_t> idx = seg.projectCloud(4, Ps.data(), P, xyz.data(), &zbuf);
        REQUIRE(idx.size() == 4 * N && zbuf.size() == 4 * N);
        size_t hits = 0;
        for (size_t i = 0; i < idx.size(); i++) {
            REQUIRE(idx[i] >= -1 && idx[i] < (int32_t)P);
            hits += idx[i] >= 0;
        }
        REQUIRE(hits > 4 * 500);

        rvseg::LocalMap with_poses;
        with_poses.id = 21; with_poses.cloud_size = P; with_poses.cloud_xyz = xyz; with_poses.cloud_rgb = crgb;
        with_poses.nodes.resize(2);
        rvseg::LocalMap with_images = with_poses;
        with_images.id = 22;
        rvseg::LocalMap with_neither = with_poses;
        with_neither.id = 23;
        for (int node = 0; node < 2; node++) {
            with_poses.nodes[(size_t)node].subimage_seqs = {seq_of(0, 0, node), seq_of(0, 1, node)};
            with_poses.nodes[(size_t)node].pose.assign(poses[node], poses[node] + 12);
            with_images.nodes[(size_t)node].subimage_seqs = {seq_of(1, 0, node), seq_of(1, 1, node)};
            with_images.nodes[(size_t)node].index_image.assign(idx.begin() + (std::ptrdiff_t)((size_t)node * 2 * N),
                                                               idx.begin() + (std::ptrdiff_t)((size_t)(node + 1) * 2 * N));   // cameras stacked row-wise
            with_neither.nodes[(size_t)node].subimage_seqs = {seq_of(2, 0, node), seq_of(2, 1, node)};
        }
        seg.onNewLocalMap(with_poses);
        seg.onNewLocalMap(with_images);
        seg.onNewLocalMap(with_neither);
        REQUIRE(seg.processMapFromQueue());
        REQUIRE(seg.processMapFromQueue());
        bool threw = false;
        try { seg.processMapFromQueue(); } catch (const std::runtime_error&) { threw = true; }
        REQUIRE(threw);
        rvseg::IdsSrvResponse ids;
        REQUIRE(seg.srvStoredSemanticsIds(ids) && ids.local_map_ids == (std::vector<int32_t>{21, 22}));
        rvseg::LocalMapSegmentationRequest req;
        rvseg::LocalMapSegmentationResponse a, b;
        req.segmentation_layers = {"material", "object"};
        req.local_map_id = 21;
        REQUIRE(seg.srvGetLocalMapSegmentation(req, a) && a.point_labels.size() == 2 * P);
        req.local_map_id = 22;
        REQUIRE(seg.srvGetLocalMapSegmentation(req, b) && b.point_labels.size() == 2 * P);
        REQUIRE(a.point_labels == b.point_labels);
        size_t known = 0;
        for (size_t i = 0; i < P; i++) known += a.point_labels[i] != 7;
        REQUIRE(known > 0);     // the fusion reached the cloud: seen points carry a class, not "Unknown"

        FILE* f = std::fopen(argv[4], "wb");
        REQUIRE(f != nullptr);
        std::fwrite(Ps.data(), 4, Ps.size(), f);
        std::fwrite(xyz.data(), 4, xyz.size(), f);
        std::fwrite(idx.data(), 4, idx.size(), f);
        std::fwrite(zbuf.data(), 4, zbuf.size(), f);
        std::fclose(f);
        std::printf("projector ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
