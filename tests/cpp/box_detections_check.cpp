// Test helper: the box head's post-processing of the C++ class surface (ElasticFusion::BoxDetections), built with plain g++ and no HIP header.
//   box_detections_check <in.bin> <out.bin>
// in.bin: seven int32 (R, C, Creg, detections_per_img, max_out, image_w, image_h), two f32 (score_thresh, nms), four f32 (the weights), then logits [R][C],
// regression [R][4 Creg] and proposals [R][4] as f32.  Without a GPU the map cannot be created ("refused: <message>"); with one, one call on the null stream:
// out.bin receives the boxes (max_out x 4 f32), scores (max_out f32), labels and indices (max_out int64 each), the count (int32) and the stats (two int32)
// ("wrote <count>"), and max_out = 8193 is refused with the library's message ("refused max_out: <message>").
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
    int32_t d[7];
    float f[2], w[4];
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)d, sizeof(d));
    in.read((char*)f, sizeof(f));
    in.read((char*)w, sizeof(w));
    const size_t R = (size_t)d[0], C = (size_t)d[1], Creg = (size_t)d[2], rows = (size_t)d[4];
    std::vector<float> logits(R * C), reg(R * 4 * Creg), prop(R * 4);
    for (std::vector<float>* v : {&logits, &reg, &prop}) in.read((char*)v->data(), (std::streamsize)(v->size() * 4));
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
    // inputs 0 .. 2, outputs 3 .. 8: boxes, scores, labels, indices, count, stats
    const size_t sizes[9] = {logits.size() * 4, reg.size() * 4, prop.size() * 4, rows * 16, rows * 4, rows * 8, rows * 8, 4, 8};
    const void* up[3] = {logits.data(), reg.data(), prop.data()};
    void* dev[9] = {};
    for (int i = 0; i < 9; i++)
        if (dev_malloc(&dev[i], sizes[i]) != 0) { std::printf("hipMalloc failed\n"); return 1; }
    for (int i = 0; i < 3; i++)
        if (dev_memcpy(dev[i], up[i], sizes[i], 1 /* host to device */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
    ifx_box_det_params p = {};
    p.score_thresh = f[0]; p.nms = f[1]; p.detections_per_img = d[3]; p.max_out = d[4];
    for (int i = 0; i < 4; i++) p.weights[i] = w[i];
    p.xform_clip = 0.f; p.image_w = d[5]; p.image_h = d[6];
    std::vector<char> out;
    for (int i = 3; i < 9; i++) out.insert(out.end(), sizes[i], 0);
    try {
        // the null stream: the copies below are ordered behind the kernels on the device
        map->BoxDetections((const float*)dev[0], (const float*)dev[1], (const float*)dev[2], d[0], d[1], d[2], p, (float*)dev[3], (float*)dev[4], (int64_t*)dev[5],
                           (int64_t*)dev[6], (int32_t*)dev[7], (int32_t*)dev[8], nullptr);
        size_t at = 0;
        for (int i = 3; i < 9; i++) {
            if (dev_memcpy(out.data() + at, dev[i], sizes[i], 2 /* device to host */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
            at += sizes[i];
        }
        std::ofstream o(argv[2], std::ios::binary);
        o.write(out.data(), (std::streamsize)out.size());
        int32_t count;
        std::memcpy(&count, out.data() + sizes[3] + sizes[4] + sizes[5] + sizes[6], 4);
        std::printf("wrote %d\n", (int)count);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    try {
        p.max_out = 8193;
        map->BoxDetections((const float*)dev[0], (const float*)dev[1], (const float*)dev[2], d[0], d[1], d[2], p, (float*)dev[3], nullptr, nullptr, nullptr, (int32_t*)dev[7],
                           nullptr, nullptr);
        std::printf("accepted max_out\n");
    } catch (const std::exception& e) {
        std::printf("refused max_out: %s\n", e.what());
    }
    for (int i = 0; i < 9; i++) dev_free(dev[i]);
    return 0;
}
