// Test helper: the detector operators of the C++ class surface (ElasticFusion::RoiAlignForward / Nms), built with plain g++ and no HIP header.
//   detector_ops_check <in.bin> <out.bin>
// in.bin: nine int32 (batch, channels, height, width, rois, pooled_h, pooled_w, sampling_ratio, boxes), two f32 (spatial_scale, threshold), then the input tensor,
// the rois (x 5), the boxes (x 4) and the scores as f32.  Without a GPU the map cannot be created ("refused: <message>"); with one, one call of each operator on
// the null stream: out.bin receives the ROIAlign output (f32), the padded keep list (boxes x int64) and the count (int32) ("wrote <outputs> <count>"), and a
// ninth thousand box is refused with the library's message ("refused n: <message>").
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
    float f[2];
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)d, sizeof(d));
    in.read((char*)f, sizeof(f));
    const size_t n_in = (size_t)d[0] * d[1] * d[2] * d[3], n_out = (size_t)d[4] * d[1] * d[5] * d[6];
    std::vector<float> input(n_in), rois((size_t)d[4] * 5), boxes((size_t)d[8] * 4), scores((size_t)d[8]);
    in.read((char*)input.data(), (std::streamsize)(input.size() * 4));
    in.read((char*)rois.data(), (std::streamsize)(rois.size() * 4));
    in.read((char*)boxes.data(), (std::streamsize)(boxes.size() * 4));
    in.read((char*)scores.data(), (std::streamsize)(scores.size() * 4));
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
    const size_t sizes[7] = {n_in * 4, rois.size() * 4, n_out * 4, boxes.size() * 4, scores.size() * 4, (size_t)d[8] * 8, 4};
    void* dev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < 7; i++)
        if (dev_malloc(&dev[i], sizes[i]) != 0) { std::printf("hipMalloc failed\n"); return 1; }
    const void* up[7] = {input.data(), rois.data(), nullptr, boxes.data(), scores.data(), nullptr, nullptr};
    for (int i = 0; i < 7; i++)
        if (up[i] && dev_memcpy(dev[i], up[i], sizes[i], 1 /* host to device */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
    std::vector<float> out(n_out, -1.f);
    std::vector<int64_t> keep((size_t)d[8], -2);
    int32_t count = -2;
    try {
        // the null stream: the copies below are ordered behind the kernels on the device
        map->RoiAlignForward((const float*)dev[0], d[0], d[1], d[2], d[3], (const float*)dev[1], d[4], f[0], d[5], d[6], d[7], (float*)dev[2], nullptr);
        map->Nms((const float*)dev[3], (const float*)dev[4], nullptr, d[8], f[1], (int64_t*)dev[5], (int32_t*)dev[6], nullptr);
        if (dev_memcpy(out.data(), dev[2], sizes[2], 2 /* device to host */) != 0 || dev_memcpy(keep.data(), dev[5], sizes[5], 2) != 0 || dev_memcpy(&count, dev[6], 4, 2) != 0) {
            std::printf("hipMemcpy failed\n");
            return 1;
        }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)out.data(), (std::streamsize)sizes[2]);
        o.write((const char*)keep.data(), (std::streamsize)sizes[5]);
        o.write((const char*)&count, 4);
        std::printf("wrote %lld %d\n", (long long)n_out, (int)count);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    try {
        map->Nms((const float*)dev[3], (const float*)dev[4], nullptr, 8193, f[1], (int64_t*)dev[5], (int32_t*)dev[6], nullptr);
        std::printf("accepted n\n");
    } catch (const std::exception& e) {
        std::printf("refused n: %s\n", e.what());
    }
    for (int i = 0; i < 7; i++) dev_free(dev[i]);
    return 0;
}
