// Test helper: the mask head's stage and the detections entry of the C++ class surface (ElasticFusion::MaskHeadSelect, InstanceFusion::
// ProcessSegmentationDetections), built with plain g++ and no HIP header.
//   mask_head_check <in.bin> <out.bin>
// in.bin: nine int32 (R, C, M, in_w, in_h, out_w, out_h, sort_by_score, use_class_map), one f32 (score_thresh), then logits [R][C][M][M] f32, boxes [R][4] f32,
// scores [R] f32, labels [R] int64, class map [C] int32.  Without a GPU the map cannot be created ("refused: <message>"); with one, one MaskHeadSelect on the null
// stream: out.bin receives the ROI masks (R x M x M f32), boxes (R x 4 f32), class ids and rows (R int32 each) and kept (int32) ("wrote <kept>"); then
// ProcessSegmentationDetections on the same inputs against the 160 x 120 map, which holds no surfel yet: the stage and the read of kept run, nothing is applied
// ("detections kept <kept>"); M = 65 is refused with the library's message ("refused 65: <message>").
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
    float thresh;
    std::ifstream in(argv[1], std::ios::binary);
    in.read((char*)d, sizeof(d));
    in.read((char*)&thresh, 4);
    const size_t R = (size_t)d[0], C = (size_t)d[1], M = (size_t)d[2];
    std::vector<float> logits(R * C * M * M), boxes(R * 4), scores(R);
    std::vector<int64_t> labels(R);
    std::vector<int32_t> cmap(C);
    in.read((char*)logits.data(), (std::streamsize)(logits.size() * 4));
    in.read((char*)boxes.data(), (std::streamsize)(boxes.size() * 4));
    in.read((char*)scores.data(), (std::streamsize)(scores.size() * 4));
    in.read((char*)labels.data(), (std::streamsize)(labels.size() * 8));
    in.read((char*)cmap.data(), (std::streamsize)(cmap.size() * 4));
    if (!in) { std::printf("short input file\n"); return 1; }
    std::unique_ptr<ElasticFusionInterface> map(new ElasticFusionInterface());
    const bool up = map->Init(std::vector<ClassColour>(), 100000, 0, "./ResultModel", false);
    std::fprintf(stderr, "map initialised: %d\n", up ? 1 : 0);
    InstanceFusion inst(IFX_NUM_INSTANCES, 160, 120);
    ifx_mask_head_params p = {};
    p.score_thresh = thresh; p.in_w = d[3]; p.in_h = d[4]; p.out_w = d[5]; p.out_h = d[6]; p.sort_by_score = d[7];
    if (!up) {
        try {
            inst.ProcessSegmentationDetections(map, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, (int)C, (int)M, p, 0.5f, 0, false, nullptr);
            std::printf("accepted\n");
        } catch (const std::exception& e) {
            std::printf("refused: %s\n", e.what());
        }
        return 0;
    }
    typedef int (*malloc_fn)(void**, size_t);
    typedef int (*memcpy_fn)(void*, const void*, size_t, int);
    typedef int (*free_fn)(void*);
    malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    memcpy_fn dev_memcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    if (!dev_malloc || !dev_memcpy || !dev_free) { std::printf("no HIP runtime in the process\n"); return 1; }
    // inputs 0 .. 4, outputs 5 .. 9: ROI masks, boxes, class ids, rows, kept
    const size_t sizes[10] = {logits.size() * 4, boxes.size() * 4, scores.size() * 4, labels.size() * 8, cmap.size() * 4, R * M * M * 4, R * 16, R * 4, R * 4, 4};
    const void* src[5] = {logits.data(), boxes.data(), scores.data(), labels.data(), cmap.data()};
    void* dev[10] = {};
    for (int i = 0; i < 10; i++)
        if (dev_malloc(&dev[i], sizes[i]) != 0) { std::printf("hipMalloc failed\n"); return 1; }
    for (int i = 0; i < 5; i++)
        if (dev_memcpy(dev[i], src[i], sizes[i], 1 /* host to device */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
    const int32_t* d_map = d[8] ? (const int32_t*)dev[4] : nullptr;
    try {
        // the null stream: the copies below are ordered behind the kernels on the device
        map->elasticFusion().MaskHeadSelect((const float*)dev[0], (const float*)dev[1], (const float*)dev[2], (const int64_t*)dev[3], nullptr, d_map, d[0], d[1], d[2], p,
                                            (float*)dev[5], (float*)dev[6], (int32_t*)dev[7], (int32_t*)dev[8], (int32_t*)dev[9], nullptr);
        std::vector<char> out;
        for (int i = 5; i < 10; i++) out.insert(out.end(), sizes[i], 0);
        size_t at = 0;
        for (int i = 5; i < 10; i++) {
            if (dev_memcpy(out.data() + at, dev[i], sizes[i], 2 /* device to host */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
            at += sizes[i];
        }
        std::ofstream o(argv[2], std::ios::binary);
        o.write(out.data(), (std::streamsize)out.size());
        int32_t kept;
        std::memcpy(&kept, out.data() + out.size() - 4, 4);
        std::printf("wrote %d\n", (int)kept);
        const int k = inst.ProcessSegmentationDetections(map, (const float*)dev[0], (const float*)dev[1], (const float*)dev[2], (const int64_t*)dev[3], nullptr, d_map, d[0],
                                                         d[1], d[2], p, 0.5f, 100, false, nullptr);
        std::printf("detections kept %d\n", k);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    try {
        inst.ProcessSegmentationDetections(map, (const float*)dev[0], (const float*)dev[1], (const float*)dev[2], (const int64_t*)dev[3], nullptr, d_map, d[0], d[1], 65, p,
                                           0.5f, 100, false, nullptr);
        std::printf("accepted 65\n");
    } catch (const std::exception& e) {
        std::printf("refused 65: %s\n", e.what());
    }
    for (int i = 0; i < 10; i++) dev_free(dev[i]);
    return 0;
}
