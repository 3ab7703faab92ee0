// Test helper: the proposal stage and the box decoding of the C++ class surface (ElasticFusion::RpnProposals / BoxDecode), built with plain g++ and no HIP header.
//   rpn_proposals_check <in.bin> <out.bin>
// in.bin: nine int32 (A, H, W, pre_nms_top_n, post_nms_top_n, image_w, image_h, decode rows, decode k), two f32 (nms_thresh, min_size), four f32 (the decode's
// weights), then objectness [A][H][W], regression [4A][H][W], anchors [H W A][4], codes [rows][4k] and boxes [rows][4] as f32.  Without a GPU the map cannot be
// created ("refused: <message>"); with one, one call of each on the null stream: out.bin receives the proposals' boxes (post x 4 f32), logits (post f32), indices
// (post int64), the count (int32) and the decoded boxes (rows x 4k f32) ("wrote <count>"), and pre_nms_top_n = 8193 is refused with the library's message
// ("refused pre: <message>").
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
    int32_t d[9];
    float f[2], w[4];
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)d, sizeof(d));
    in.read((char*)f, sizeof(f));
    in.read((char*)w, sizeof(w));
    const size_t n = (size_t)d[0] * d[1] * d[2], post = (size_t)d[4], n_codes = (size_t)d[7] * 4 * d[8];
    std::vector<float> obj(n), reg(4 * n), anc(4 * n), codes(n_codes), boxes((size_t)d[7] * 4);
    for (std::vector<float>* v : {&obj, &reg, &anc, &codes, &boxes}) in.read((char*)v->data(), (std::streamsize)(v->size() * 4));
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
    // inputs 0 .. 4, outputs 5 .. 9: boxes, logits, indices, count, decoded
    const size_t sizes[10] = {n * 4, n * 16, n * 16, n_codes * 4, boxes.size() * 4, post * 16, post * 4, post * 8, 4, n_codes * 4};
    const void* up[5] = {obj.data(), reg.data(), anc.data(), codes.data(), boxes.data()};
    void* dev[10] = {};
    for (int i = 0; i < 10; i++)
        if (dev_malloc(&dev[i], sizes[i]) != 0) { std::printf("hipMalloc failed\n"); return 1; }
    for (int i = 0; i < 5; i++)
        if (dev_memcpy(dev[i], up[i], sizes[i], 1 /* host to device */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
    ifx_rpn_params p = {};
    p.pre_nms_top_n = d[3]; p.post_nms_top_n = d[4]; p.nms_thresh = f[0]; p.min_size = f[1];
    p.weights[0] = p.weights[1] = p.weights[2] = p.weights[3] = 1.f;
    p.xform_clip = 0.f; p.image_w = d[5]; p.image_h = d[6];
    std::vector<char> out;
    for (int i = 5; i < 10; i++) out.insert(out.end(), sizes[i], 0);
    try {
        // the null stream: the copies below are ordered behind the kernels on the device
        map->RpnProposals((const float*)dev[0], (const float*)dev[1], (const float*)dev[2], d[0], d[1], d[2], p, (float*)dev[5], (float*)dev[6], (int64_t*)dev[7],
                          (int32_t*)dev[8], nullptr);
        map->BoxDecode((const float*)dev[3], (const float*)dev[4], d[7], d[8], w, 0.f, 0, 0, (float*)dev[9], nullptr);
        size_t at = 0;
        for (int i = 5; i < 10; i++) {
            if (dev_memcpy(out.data() + at, dev[i], sizes[i], 2 /* device to host */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
            at += sizes[i];
        }
        std::ofstream o(argv[2], std::ios::binary);
        o.write(out.data(), (std::streamsize)out.size());
        int32_t count;
        std::memcpy(&count, out.data() + sizes[5] + sizes[6] + sizes[7], 4);
        std::printf("wrote %d\n", (int)count);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    try {
        p.pre_nms_top_n = 8193;
        map->RpnProposals((const float*)dev[0], (const float*)dev[1], (const float*)dev[2], d[0], d[1], d[2], p, (float*)dev[5], nullptr, nullptr, (int32_t*)dev[8], nullptr);
        std::printf("accepted pre\n");
    } catch (const std::exception& e) {
        std::printf("refused pre: %s\n", e.what());
    }
    for (int i = 0; i < 10; i++) dev_free(dev[i]);
    return 0;
}
