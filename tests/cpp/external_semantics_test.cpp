// Exercises the external-semantics calls of the C++ Segmenter facade (include/rvseg_segmenter.hpp) the way
// Segmenter::processFramesFromQueueExternal drives the service (src/segmenter.cpp:445-514): construct without a forest,
// build the request (RGB8 + rectified 32FC3 xyz), hand a provider's label_distribution to the frame CRF.  Writes the
// request's depth image, the marginals and the labels; the Python test compares them with the C ABI's own output.
// usage: external_semantics_test <rgb.u8> <depth.u16> <dist.f32> <out.bin>
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

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage\n"); return 2; }
    try {
        rvseg::Config conf;
        conf.width = 160; conf.height = 120;
        conf.external_semantics = true;      // no forest_file_name: nothing is loaded
        conf.per_frame_crf = true;
        conf.label_mode = RVSEG_LABEL_CRF;
        conf.dcrf_iterations = 3;
        const char* names[2] = {"structure", "object"};
        const int counts[2] = {3, 5};
        for (int l = 0; l < 2; l++) {
            rvseg::Layer layer;
            layer.name = names[l];
            for (int c = 0; c < counts[l]; c++) layer.classes.push_back({"class" + std::to_string(c), {(uint8_t)c, (uint8_t)(2 * c), (uint8_t)(3 * c)}});
            layer.unknown_label = counts[l] - 1;
            conf.layers.push_back(layer);
        }
        rvseg::Segmenter seg(conf);
        if (seg.totalLabels() != 8) return 1;
        int32_t n_layers = 0;
        if (rvseg_forest_info(seg.context(), nullptr, nullptr, nullptr, &n_layers, nullptr) != RVSEG_ERR_NO_FOREST) return 1;

        const size_t N = (size_t)conf.width * conf.height, S = 8;
        std::vector<uint8_t> rgb = slurp(argv[1]), draw = slurp(argv[2]), fraw = slurp(argv[3]);
        if (rgb.size() != N * 3 || draw.size() != N * 2 || fraw.size() != N * S * 4) { std::fprintf(stderr, "bad input sizes\n"); return 1; }
        const uint16_t* depth = reinterpret_cast<const uint16_t*>(draw.data());
        const float fx = 525.f * conf.width / 640.f;
        const float calib[21] = {1 / fx, 0, -(conf.width / 2.f) / fx, 0, 1 / fx, -(conf.height / 2.f) / fx, 0, 0, 1,
                                 0, 0, 1, -1, 0, 0, 0, -1, 0, 0.1f, -0.2f, 0.6f};
        // the request of :490-502
        rvseg::SingleFrameSegmentationRequest req = seg.externalRequest(42, rgb.data(), depth, calib);
        if (req.rgb.encoding != "rgb8" || req.depth.encoding != "32FC3" || req.rgb.seq != 42 || req.depth.seq != 42) return 1;
        if (req.rgb.height != 120 || req.rgb.width != 160 || req.rgb.step != 480 || req.depth.step != 1920) return 1;
        if (req.rgb.data != rgb || req.depth.data.size() != N * 12) return 1;
        // the response: what a provider returned
        rvseg::SingleFrameSegmentationResponse resp;
        resp.label_distribution.resize(N * S);
        std::memcpy(resp.label_distribution.data(), fraw.data(), fraw.size());

        std::vector<float> marg(N * S);
        std::vector<int8_t> labels(N * 2);
        seg.processFramesExternal(1, rgb.data(), depth, calib, resp.label_distribution.data(), 1, marg.data(), labels.data());
        // a stride the context does not have must throw, and leave the object usable
        bool threw = false;
        try {
            seg.processFramesExternal(1, rgb.data(), depth, calib, resp.label_distribution.data(), 3, marg.data(), labels.data());
        } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::fprintf(stderr, "bad dist_stride did not throw\n"); return 1; }
        // the forest path of an external-semantics object has no model
        threw = false;
        try { seg.processFrames(1, rgb.data(), depth, calib); } catch (const std::runtime_error&) { threw = true; }
        if (!threw) { std::fprintf(stderr, "processFrames without a forest did not throw\n"); return 1; }
        std::vector<int8_t> again(N * 2);
        seg.setExternalLayers({3, 5});
        seg.processFramesExternal(1, rgb.data(), depth, calib, resp.label_distribution.data(), 1, nullptr, again.data());
        if (again != labels) return 1;

        FILE* out = std::fopen(argv[4], "wb");
        std::fwrite(req.depth.data.data(), 1, req.depth.data.size(), out);
        std::fwrite(marg.data(), 4, marg.size(), out);
        std::fwrite(labels.data(), 1, labels.size(), out);
        std::fclose(out);
        std::printf("external ok\n");
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "exception: %s\n", e.what());
        return 1;
    }
}
