// Test helper: multi-level ROI pooling of the C++ class surface (ElasticFusion::FpnRoiAlign), built with plain g++ and no HIP header.
//   fpn_pooler_check <in.bin> <out.bin>
// in.bin: seven int32 (levels, batch, channels, rois, pooled_h, pooled_w, sampling_ratio), then per level two int32 (height, width) and one f32 (scale), then the
// maps level by level and the rois (x 5) as f32.  Without a GPU the map cannot be created ("refused: <message>"); with one, one call on the null stream: out.bin
// receives the pooled output (f32) and the levels (rois x int32) ("wrote <outputs>"), and scales that are no ladder are refused with the library's message
// ("refused scales: <message>").
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
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)d, sizeof(d));
    const int levels = d[0];
    if (!in || levels < 1 || levels > 8) { std::printf("bad input file\n"); return 1; }
    int32_t heights[8], widths[8];
    float scales[8];
    for (int l = 0; l < levels; l++) {
        in.read((char*)&heights[l], 4);
        in.read((char*)&widths[l], 4);
        in.read((char*)&scales[l], 4);
    }
    std::vector<std::vector<float>> maps((size_t)levels);
    for (int l = 0; l < levels; l++) {
        maps[l].resize((size_t)d[1] * d[2] * heights[l] * widths[l]);
        in.read((char*)maps[l].data(), (std::streamsize)(maps[l].size() * 4));
    }
    std::vector<float> rois((size_t)d[3] * 5);
    in.read((char*)rois.data(), (std::streamsize)(rois.size() * 4));
    if (!in) { std::printf("short input file\n"); return 1; }
    const size_t n_out = (size_t)d[3] * d[2] * d[4] * d[5];
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
    void* dev[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // the maps, then rois, out, levels
    size_t sizes[11];
    const void* up[11];
    for (int l = 0; l < levels; l++) { sizes[l] = maps[l].size() * 4; up[l] = maps[l].data(); }
    sizes[levels] = rois.size() * 4; up[levels] = rois.data();
    sizes[levels + 1] = n_out * 4; up[levels + 1] = nullptr;
    sizes[levels + 2] = (size_t)d[3] * 4; up[levels + 2] = nullptr;
    for (int i = 0; i < levels + 3; i++) {
        if (dev_malloc(&dev[i], sizes[i]) != 0) { std::printf("hipMalloc failed\n"); return 1; }
        if (up[i] && dev_memcpy(dev[i], up[i], sizes[i], 1 /* host to device */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
    }
    const float* features[8];
    for (int l = 0; l < levels; l++) features[l] = (const float*)dev[l];
    std::vector<float> out(n_out, -1.f);
    std::vector<int32_t> lev((size_t)d[3], -2);
    try {
        // the null stream: the copies below are ordered behind the kernel on the device
        map->FpnRoiAlign(features, heights, widths, scales, levels, d[1], d[2], (const float*)dev[levels], d[3], d[4], d[5], d[6], (float*)dev[levels + 1],
                         (int32_t*)dev[levels + 2], nullptr);
        if (dev_memcpy(out.data(), dev[levels + 1], sizes[levels + 1], 2 /* device to host */) != 0 || dev_memcpy(lev.data(), dev[levels + 2], sizes[levels + 2], 2) != 0) {
            std::printf("hipMemcpy failed\n");
            return 1;
        }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)out.data(), (std::streamsize)sizes[levels + 1]);
        o.write((const char*)lev.data(), (std::streamsize)sizes[levels + 2]);
        std::printf("wrote %lld\n", (long long)n_out);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    try {
        scales[0] *= 1.5f;
        map->FpnRoiAlign(features, heights, widths, scales, levels, d[1], d[2], (const float*)dev[levels], d[3], d[4], d[5], d[6], (float*)dev[levels + 1], nullptr, nullptr);
        std::printf("accepted scales\n");
    } catch (const std::exception& e) {
        std::printf("refused scales: %s\n", e.what());
    }
    for (int i = 0; i < levels + 3; i++) dev_free(dev[i]);
    return 0;
}
