// Test helper: the ROI form of a segmentation call on a sharded map at a world of one (n_ranks = -1, root = 0), driven through the C ABI the way a host with its own
// transport drives it -- ifx_owner_segmentation_begin_rois, the exchange list of ifx_owner_exchange(h, 200, ...), ifx_owner_segmentation_resume -- built with plain
// g++ and no HIP header (ifx_host.hpp is included so that its owner forms compile with it).
//   owner_seg_device_check                      -> "refused: <message>" where there is no GPU, "created" otherwise
//   owner_seg_device_check <in.bin> <out.bin>
// in.bin: int32 nf, w, h, n, M, upload_at, n_surfels, tick; f32 fx, fy, cx, cy; pose f32[16]; the map to upload in front of frame upload_at (pc, nr f32[ns][4], col, tm
// f32[ns][2], ic f32[ns][4], votes f32[ns][48]); nf frames (rgb u8[P][3], depth u16[P]); ROI masks f32[n][M][M], boxes f32[n][4], class ids int32[n].
// The frames go through ifx_owner_frame_phase (a world of one: every exchange is the identity), then one call with the superpixel refinement on the last frame.
// Prints "record <bytes> op <op>" for the call's first exchange point and "exchanges <count>"; out.bin receives the labels (int32 per live surfel).
// The runtime calls the helper needs for its own buffers are looked up in the HIP runtime libifx.so has loaded.
#include <dlfcn.h>

#include <cstdio>
#include <fstream>

#include "ifx_host.hpp"

static int fail(ifx_t* h, const char* what)
{
    std::printf("%s failed: %s\n", what, h ? ifx_last_error(h) : "");
    return 1;
}

int main(int argc, char** argv)
{
    int32_t d[8] = {0, 64, 48, 0, 1, -1, 0, 0};
    float k[4] = {50.f, 50.f, 32.f, 24.f}, pose[16] = {};
    std::ifstream in;
    if (argc == 3) {
        in.open(argv[1], std::ios::binary);
        in.read((char*)d, sizeof(d));
        in.read((char*)k, sizeof(k));
        in.read((char*)pose, sizeof(pose));
        if (!in) { std::printf("short input file\n"); return 1; }
    } else if (argc != 1) return 2;
    ifx_config cfg = {};
    cfg.width = d[1]; cfg.height = d[2];
    cfg.fx = k[0]; cfg.fy = k[1]; cfg.cx = k[2]; cfg.cy = k[3];
    cfg.time_delta = 200; cfg.confidence = 10.f; cfg.depth_cut = 12.f; cfg.max_depth_processed = 20.f; cfg.icp_weight = 10.f;
    cfg.pyramid = 1; cfg.fast_odom = 0; cfg.so3 = 1; cfg.max_surfels = 400000; cfg.device = 0; cfg.n_ranks = -1; cfg.rank = 0;
    ifx_t* h = nullptr;
    if (ifx_create(&cfg, &h) != IFX_OK || !h) { std::printf("refused: no handle without a GPU\n"); return 0; }
    if (argc == 1) { std::printf("created\n"); ifx_destroy(h); return 0; }
    const size_t nf = (size_t)d[0], P = (size_t)d[1] * d[2], n = (size_t)d[3], M = (size_t)d[4], ns = (size_t)d[6];
    std::vector<float> pc(ns * 4), nr(ns * 4), col(ns * 2), tm(ns * 2), ic(ns * 4), votes(ns * 48), rois(n * M * M), boxes(n * 4);
    std::vector<uint8_t> rgb(nf * P * 3);
    std::vector<uint16_t> depth(nf * P);
    std::vector<int32_t> cls(n);
    for (std::vector<float>* v : {&pc, &nr, &col, &tm, &ic, &votes}) in.read((char*)v->data(), (std::streamsize)(v->size() * 4));
    for (size_t f = 0; f < nf; f++) {
        in.read((char*)&rgb[f * P * 3], (std::streamsize)(P * 3));
        in.read((char*)&depth[f * P], (std::streamsize)(P * 2));
    }
    in.read((char*)rois.data(), (std::streamsize)(rois.size() * 4));
    in.read((char*)boxes.data(), (std::streamsize)(boxes.size() * 4));
    in.read((char*)cls.data(), (std::streamsize)(cls.size() * 4));
    if (!in) { std::printf("short input file\n"); return 1; }
    typedef int (*malloc_fn)(void**, size_t);
    typedef int (*memcpy_fn)(void*, const void*, size_t, int);
    typedef int (*free_fn)(void*);
    malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    memcpy_fn dev_memcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    if (!dev_malloc || !dev_memcpy || !dev_free) { std::printf("no HIP runtime in the process\n"); return 1; }
    // every frame in device memory of its own (a frame's phases are enqueue-only), then the ROI tensors
    const size_t sizes[5] = {rgb.size(), depth.size() * 2, rois.size() * 4, boxes.size() * 4, cls.size() * 4};
    const void* src[5] = {rgb.data(), depth.data(), rois.data(), boxes.data(), cls.data()};
    void* dev[5] = {};
    for (int i = 0; i < 5; i++) {
        if (dev_malloc(&dev[i], sizes[i]) != 0) { std::printf("hipMalloc failed\n"); return 1; }
        if (dev_memcpy(dev[i], src[i], sizes[i], 1 /* host to device */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
    }
    void* ptrs[8]; int64_t bytes[8]; int32_t ops[8];
    const int phases[11] = {310, 300, 301, 0, 1, 2, 3, 4, 5, 6, 7};
    for (size_t f = 0; f < nf; f++) {
        if ((int)f == d[5]) {   // the stable map of the Python run, the pose it belongs to, and the prediction from it (steps 0 and 1 are followed by exchanges 4 and 5)
            if (ifx_map_upload(h, (int)ns, pc.data(), nr.data(), col.data(), tm.data(), ic.data(), votes.data()) < 0) return fail(h, "ifx_map_upload");
            if (ifx_set_pose(h, pose, d[7]) < 0) return fail(h, "ifx_set_pose");
            for (int step = 0; step < 3; step++)
                if (ifx_owner_predict_phase(h, step) < 0) return fail(h, "ifx_owner_predict_phase");
        }
        for (int phase : phases) {
            if (ifx_owner_frame_phase(h, phase, (const uint8_t*)dev[0] + f * P * 3, (const uint16_t*)dev[1] + f * P) < 0) return fail(h, "ifx_owner_frame_phase");
            if (ifx_owner_exchange(h, phase, ptrs, bytes, ops, 8) < 0) return fail(h, "ifx_owner_exchange");   // (one rank: every reduction is the identity)
        }
    }
    int r = ifx_owner_segmentation_begin_rois(h, 0, 16, &rgb[(nf - 1) * P * 3], &depth[(nf - 1) * P], (const float*)dev[2], (int)M, (const float*)dev[3], 0.5f, (const int32_t*)dev[4],
                                              (int)n, 100, 2, nullptr);
    if (r < 0) return fail(h, "ifx_owner_segmentation_begin_rois");
    int exchanges = 0;
    while (r == 1) {
        const int nb = ifx_owner_exchange(h, 200, ptrs, bytes, ops, 8);
        if (nb < 0) return fail(h, "ifx_owner_exchange");
        if (exchanges == 0) {
            if (nb != 1) { std::printf("the first exchange point lists %d buffers\n", nb); return 1; }
            std::printf("record %lld op %d\n", (long long)bytes[0], (int)ops[0]);
        }
        exchanges++;
        r = ifx_owner_segmentation_resume(h);   // (a broadcast from the one rank to itself: nothing to move)
        if (r < 0) return fail(h, "ifx_owner_segmentation_resume");
    }
    std::printf("exchanges %d\n", exchanges);
    const int count = ifx_map_count(h);
    if (count < 0) return fail(h, "ifx_map_count");
    std::vector<int32_t> labels((size_t)std::max(count, 1));
    const int m = ifx_labels(h, labels.data(), count);
    if (m < 0) return fail(h, "ifx_labels");
    std::ofstream o(argv[2], std::ios::binary);
    o.write((const char*)labels.data(), (std::streamsize)((size_t)m * 4));
    std::printf("labels %d\n", m);
    for (int i = 0; i < 5; i++) dev_free(dev[i]);
    ifx_destroy(h);
    return 0;
}
