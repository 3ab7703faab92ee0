// Test helper: the detector-input entries of the C++ class surface (InstanceFusion::DetectorInputSize / DetectorInput), built with plain g++ and no HIP header.
//   detector_input_check <frames.bin> <out.bin>
// frames.bin: two 160 x 120 frames, each rgb (u8 x 3) then depth (u16).  Prints "size <ow> <oh> <W'> <H'>" (host only: works anywhere); without a GPU the map
// cannot be created and DetectorInput must refuse loudly ("refused: <message>"); with one, both frames are processed, DetectorInput(ticket -1) writes into a
// device buffer, out.bin receives its 3 * H' * W' floats ("wrote <n>") and a zero std is refused with the library's message ("refused std: <message>").
// The three runtime calls the helper needs for its own buffer are looked up in the HIP runtime libifx.so has loaded.
#include <dlfcn.h>

#include <cstdio>
#include <fstream>

#include "ifx_host.hpp"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    const int W = 160, H = 120;
    Resolution::getInstance(W, H);
    Intrinsics::getInstance(132.f, 132.f, 80.f, 60.f);
    ifx_detector_prep prep = InstanceFusion::DetectorPrep(100, 0, 32, true, true);
    int32_t sz[4];
    InstanceFusion::DetectorInputSize(W, H, prep, sz);
    std::printf("size %d %d %d %d\n", sz[0], sz[1], sz[2], sz[3]);
    std::unique_ptr<ElasticFusionInterface> map(new ElasticFusionInterface());
    const bool up = map->Init(std::vector<ClassColour>(), 200000, 0, "./ResultModel", false);
    std::fprintf(stderr, "map initialised: %d\n", up ? 1 : 0);
    InstanceFusion inst(IFX_NUM_INSTANCES, W, H);
    const int64_t n = (int64_t)3 * sz[2] * sz[3];
    if (!up) {
        try {
            inst.DetectorInput(map, -1, prep, nullptr, n, nullptr);
            std::printf("accepted\n");
        } catch (const std::exception& e) {
            std::printf("refused: %s\n", e.what());
        }
        return 0;
    }
    std::vector<unsigned char> rgb((size_t)W * H * 3);
    std::vector<unsigned short> depth((size_t)W * H);
    std::ifstream f(argv[1], std::ios::binary);
    for (int i = 0; i < 2; i++) {
        f.read((char*)rgb.data(), (std::streamsize)rgb.size());
        f.read((char*)depth.data(), (std::streamsize)(depth.size() * 2));
        if (!f) { std::printf("short frame file\n"); return 1; }
        map->ProcessFrame(rgb.data(), depth.data(), i, nullptr, nullptr);
    }
    typedef int (*malloc_fn)(void**, size_t);
    typedef int (*memcpy_fn)(void*, const void*, size_t, int);
    typedef int (*free_fn)(void*);
    malloc_fn dev_malloc = (malloc_fn)dlsym(RTLD_DEFAULT, "hipMalloc");
    memcpy_fn dev_memcpy = (memcpy_fn)dlsym(RTLD_DEFAULT, "hipMemcpy");
    free_fn dev_free = (free_fn)dlsym(RTLD_DEFAULT, "hipFree");
    if (!dev_malloc || !dev_memcpy || !dev_free) { std::printf("no HIP runtime in the process\n"); return 1; }
    float* d_out = nullptr;
    if (dev_malloc((void**)&d_out, (size_t)n * 4) != 0) { std::printf("hipMalloc failed\n"); return 1; }
    std::vector<float> out((size_t)n, -1.f);
    try {
        inst.DetectorInput(map, -1, prep, d_out, n, nullptr);   // the null stream is the consumer: the copy below is ordered behind the kernel on the device
        if (dev_memcpy(out.data(), d_out, (size_t)n * 4, 2 /* device to host */) != 0) { std::printf("hipMemcpy failed\n"); return 1; }
        std::ofstream o(argv[2], std::ios::binary);
        o.write((const char*)out.data(), (std::streamsize)((size_t)n * 4));
        std::printf("wrote %lld\n", (long long)n);
    } catch (const std::exception& e) {
        std::printf("failed: %s\n", e.what());
        return 1;
    }
    try {
        prep.std[1] = 0.f;
        inst.DetectorInput(map, -1, prep, d_out, n, nullptr);
        std::printf("accepted std\n");
    } catch (const std::exception& e) {
        std::printf("refused std: %s\n", e.what());
    }
    dev_free(d_out);
    return 0;
}
