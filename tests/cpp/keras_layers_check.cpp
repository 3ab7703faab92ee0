// Test helper: the Keras detector's three layers of the C++ class surface (ElasticFusion::KerasProposals, PyramidRoiAlign, KerasDetections) and
// ifx_pyramid_level_thresholds, built with plain g++ and no HIP header.
//   keras_layers_check <in.bin>
// in.bin: twelve int32 (n, pre_nms_limit, proposal_count, image_h, image_w, R, C, max_instances, feature channels, pool, boxes, layout), three f32 (the proposal
// layer's threshold, min_confidence, the detection layer's threshold), the window (four f32); then as f32 probs [n][2], bbox [n][4], anchors [n][4], rois [R][4],
// class probs [R][C], deltas [R][C][4], the four maps of 16^2, 8^2, 4^2 and 2^2 texels (one image, in the given layout) and boxes [boxes][4].  The std-dev vector
// is the reference's (0.1, 0.1, 0.2, 0.2).  Without a GPU the map cannot be created ("refused: <message>"); with one, the three calls on the null stream, and one
// line per output with the FNV-1a checksum of its bytes: "proposals <hex> index <hex> count <c>", "pooled <hex> levels <hex>", "detections <hex> norm <hex> index
// <hex> count <c>", then "thresholds <T0> <T1> <T2>" as f32 bit patterns, and a refused call's message ("refused count: <message>").
// The three runtime calls the helper needs for its own buffers are looked up in the HIP runtime libifx.so has loaded.
#include <dlfcn.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "ifx_host.hpp"

static unsigned long long fnv(const std::vector<char>& v)
{
    unsigned long long h = 1469598103934665603ull;
    for (char c : v) { h ^= (unsigned char)c; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    Resolution::getInstance(160, 120);
    Intrinsics::getInstance(132.f, 132.f, 80.f, 60.f);
    int32_t d[12];
    float f[3], win[4];
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)d, sizeof(d));
    in.read((char*)f, sizeof(f));
    in.read((char*)win, sizeof(win));
    const size_t n = (size_t)d[0], count = (size_t)d[2], R = (size_t)d[5], C = (size_t)d[6], M = (size_t)d[7], Cf = (size_t)d[8], pool = (size_t)d[9], nb = (size_t)d[10];
    const int32_t sizes_hw[4] = {16, 8, 4, 2};
    std::vector<std::vector<float>> host = {std::vector<float>(n * 2), std::vector<float>(n * 4), std::vector<float>(n * 4), std::vector<float>(R * 4),
                                            std::vector<float>(R * C), std::vector<float>(R * C * 4)};
    for (int s : sizes_hw) host.emplace_back((size_t)s * s * Cf);
    host.emplace_back(nb * 4);
    for (auto& v : host) in.read((char*)v.data(), (std::streamsize)(v.size() * 4));
    if (!in) { std::printf("short input file\n"); return 1; }
    std::unique_ptr<ElasticFusion> map;
    try {
        map.reset(new ElasticFusion(200, 35000, 5e-05f, 1e-05f, false, false, false, 115, 10, 12, 10, false, 0.3095f, true, false, "", 100000));
    } catch (const std::exception& e) {
        std::printf("refused: %s\n", e.what());
        return 0;
    }
    typedef int (*malloc_fn)(void**, size_t);
    typedef int (*memcpy_fn)(void*, const void*, size_t, int);
    typedef int (*free_fn)(void*);
    malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    memcpy_fn dev_memcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    if (!dev_malloc || !dev_memcpy || !dev_free) { std::printf("no HIP runtime in the process\n"); return 1; }
    std::vector<void*> dev;
    auto alloc = [&](size_t bytes) -> void* {
        void* p = nullptr;
        if (dev_malloc(&p, bytes ? bytes : 4) != 0) { std::printf("hipMalloc failed\n"); std::exit(1); }
        dev.push_back(p);
        return p;
    };
    std::vector<float*> up;
    for (auto& v : host) {
        up.push_back((float*)alloc(v.size() * 4));
        if (dev_memcpy(up.back(), v.data(), v.size() * 4, 1 /* host to device */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
    }
    auto sum = [&](void* p, size_t bytes) {
        std::vector<char> v(bytes);
        if (dev_memcpy(v.data(), p, bytes, 2 /* device to host */) != 0) { std::printf("hipMemcpy failed\n"); std::exit(1); }
        return fnv(v);
    };
    auto count_of = [&](void* p) {
        int32_t c = 0;
        if (dev_memcpy(&c, p, 4, 2) != 0) { std::printf("hipMemcpy failed\n"); std::exit(1); }
        return (int)c;
    };
    try {
        // the null stream is the map's main stream: the copies above and below are ordered with it on the device
        ifx_keras_proposal_params pp = {};
        pp.pre_nms_limit = d[1]; pp.proposal_count = d[2]; pp.nms_threshold = f[0];
        pp.std_dev[0] = 0.1f; pp.std_dev[1] = 0.1f; pp.std_dev[2] = 0.2f; pp.std_dev[3] = 0.2f;
        pp.image_h = d[3]; pp.image_w = d[4];
        float* prop = (float*)alloc(count * 16);
        int64_t* pidx = (int64_t*)alloc(count * 8);
        int32_t* pcnt = (int32_t*)alloc(4);
        map->KerasProposals(up[0], up[1], up[2], d[0], pp, prop, pidx, pcnt, nullptr);
        std::printf("proposals %016llx index %016llx count %d\n", sum(prop, count * 16), sum(pidx, count * 8), count_of(pcnt));

        const float* feats[4] = {up[6], up[7], up[8], up[9]};
        const size_t out_floats = nb * Cf * pool * pool;
        float* pooled = (float*)alloc(out_floats * 4);
        int32_t* levels = (int32_t*)alloc(nb * 4);
        map->PyramidRoiAlign(feats, sizes_hw, sizes_hw, 1, d[8], d[11], up[10], d[10], d[3], d[4], d[9], d[9], pooled, levels, nullptr);
        std::printf("pooled %016llx levels %016llx\n", sum(pooled, out_floats * 4), sum(levels, nb * 4));

        ifx_keras_detection_params dp = {};
        dp.std_dev[0] = 0.1f; dp.std_dev[1] = 0.1f; dp.std_dev[2] = 0.2f; dp.std_dev[3] = 0.2f;
        dp.min_confidence = f[1]; dp.nms_threshold = f[2]; dp.max_instances = d[7]; dp.image_h = d[3]; dp.image_w = d[4];
        for (int i = 0; i < 4; i++) dp.window[i] = win[i];
        float* det = (float*)alloc(M * 24);
        float* norm = (float*)alloc(M * 16);
        int64_t* didx = (int64_t*)alloc(M * 8);
        int32_t* dcnt = (int32_t*)alloc(4);
        map->KerasDetections(up[3], up[4], up[5], d[5], d[6], dp, det, norm, didx, dcnt, nullptr);
        std::printf("detections %016llx norm %016llx index %016llx count %d\n", sum(det, M * 24), sum(norm, M * 16), sum(didx, M * 8), count_of(dcnt));

        float t[3];
        if (ifx_pyramid_level_thresholds(d[3], d[4], t) != 0) { std::printf("thresholds refused\n"); return 1; }
        uint32_t u[3];
        std::memcpy(u, t, sizeof u);
        std::printf("thresholds %08x %08x %08x\n", u[0], u[1], u[2]);
        try {
            pp.proposal_count = 8193;
            map->KerasProposals(up[0], up[1], up[2], d[0], pp, prop, nullptr, pcnt, nullptr);
            std::printf("accepted count\n");
        } catch (const std::exception& e) {
            std::printf("refused count: %s\n", e.what());
        }
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    for (void* p : dev) dev_free(p);
    return 0;
}
