// Test helper: the proposal stage over the levels of an FPN of the C++ class surface (ElasticFusion::RpnProposalsFpn), built with plain g++ and no HIP header.
//   rpn_fpn_check <in.bin> <out.bin>
// in.bin: six int32 (levels L, pre_nms_top_n, post_nms_top_n, fpn_post_nms_top_n F, image_w, image_h), two f32 (nms_thresh, min_size), L x three int32 (A, H, W),
// then per level objectness [A][H][W], regression [4A][H][W] and anchors [H W A][4] as f32.  Without a GPU the map cannot be created ("refused: <message>"); with
// one, one call on the null stream: out.bin receives boxes (F x 4 f32), logits (F f32), levels (F int32), indices (F int64), the count (int32) and the levels'
// counts (L int32) ("wrote <count>"), and n_levels = 9 is refused with the library's message ("refused levels: <message>").
// The three runtime calls the helper needs for its own buffers are looked up in the HIP runtime libifx.so has loaded.
#include <dlfcn.h>

#include <cstdio>
#include <fstream>

#include "ifx_host.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    Resolution::getInstance(160, 120);
    Intrinsics::getInstance(132.f, 132.f, 80.f, 60.f);
    int32_t d[6], shape[8][3];
    float f[2];
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)d, sizeof(d));
    in.read((char*)f, sizeof(f));
    const int L = d[0];
    if (!in || L < 1 || L > 8) { std::printf("bad input file\n"); return 1; }
    in.read((char*)shape, (std::streamsize)(L * 12));
    std::vector<std::vector<float>> host;
    for (int l = 0; l < L; l++) {
        const size_t n = (size_t)shape[l][0] * shape[l][1] * shape[l][2];
        for (size_t count : {n, 4 * n, 4 * n}) {
            host.emplace_back(count);
            in.read((char*)host.back().data(), (std::streamsize)(count * 4));
        }
    }
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
    for (const std::vector<float>& v : host) {
        void* p = nullptr;
        if (dev_malloc(&p, v.size() * 4 + 16) != 0 || dev_memcpy(p, v.data(), v.size() * 4, 1 /* host to device */) != 0) { std::printf("upload failed\n"); return 1; }
        dev.push_back(p);
    }
    ifx_rpn_level levels[9] = {};
    for (int l = 0; l < L; l++) {
        levels[l].objectness = (const float*)dev[3 * l]; levels[l].regression = (const float*)dev[3 * l + 1]; levels[l].anchors = (const float*)dev[3 * l + 2];
        levels[l].A = shape[l][0]; levels[l].H = shape[l][1]; levels[l].W = shape[l][2];
    }
    const size_t F = (size_t)d[3];
    // outputs: boxes, logits, levels, indices, count, the levels' counts
    const size_t sizes[6] = {F * 16, F * 4, F * 4, F * 8, 4, (size_t)L * 4};
    void* o[6] = {};
    for (int i = 0; i < 6; i++)
        if (dev_malloc(&o[i], sizes[i]) != 0) { std::printf("hipMalloc failed\n"); return 1; }
    ifx_rpn_params p = {};
    p.pre_nms_top_n = d[1]; p.post_nms_top_n = d[2]; p.nms_thresh = f[0]; p.min_size = f[1];
    p.weights[0] = p.weights[1] = p.weights[2] = p.weights[3] = 1.f;
    p.xform_clip = 0.f; p.image_w = d[4]; p.image_h = d[5];
    std::vector<char> out;
    for (size_t s : sizes) out.insert(out.end(), s, 0);
    try {
        // the null stream: the copies below are ordered behind the kernels on the device
        map->RpnProposalsFpn(levels, L, p, d[3], (float*)o[0], (float*)o[1], (int32_t*)o[2], (int64_t*)o[3], (int32_t*)o[4], (int32_t*)o[5], nullptr);
        size_t at = 0;
        for (int i = 0; i < 6; i++) {
            if (dev_memcpy(out.data() + at, o[i], sizes[i], 2 /* device to host */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
            at += sizes[i];
        }
        std::ofstream of(argv[2], std::ios::binary);
        of.write(out.data(), (std::streamsize)out.size());
        int32_t count;
        std::memcpy(&count, out.data() + sizes[0] + sizes[1] + sizes[2] + sizes[3], 4);
        std::printf("wrote %d\n", (int)count);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    try {
        map->RpnProposalsFpn(levels, 9, p, d[3], (float*)o[0], nullptr, nullptr, nullptr, (int32_t*)o[4], nullptr, nullptr);
        std::printf("accepted levels\n");
    } catch (const std::exception& e) {
        std::printf("refused levels: %s\n", e.what());
    }
    for (void* p2 : dev) dev_free(p2);
    for (void* p2 : o) dev_free(p2);
    return 0;
}
