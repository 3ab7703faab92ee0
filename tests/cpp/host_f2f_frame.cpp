// The reference's constructor arguments `reloc` and `frameToFrameRGB` through the C++ host class (instancefusion_amd/host/ifx_host.hpp): a translation unit that
// constructs ElasticFusion with frameToFrameRGB = true -- it used to throw -- and runs frames.  usage: host_f2f_frame W H reloc(0|1)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ifx_host.hpp"

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int w = std::atoi(argv[1]), h = std::atoi(argv[2]);
    const bool reloc = std::atoi(argv[3]) != 0;
    try {
        Resolution::getInstance(w, h);
        Intrinsics::getInstance(0.825f * w, 0.825f * w, 0.5f * w, 0.5f * h);
        ElasticFusion ef(200, 35000, 5e-05f, 1e-05f, true, false, reloc, 115, 10, 12, 10, false, 0.3095f, true, /* frameToFrameRGB */ true, "", 200000);
        std::vector<unsigned char> rgb((size_t)w * h * 3);
        std::vector<unsigned short> depth((size_t)w * h);
        for (int f = 0; f < 3; f++) {   // a tilted, textured plane that shifts by a pixel per frame
            for (int y = 0; y < h; y++)
                for (int x = 0; x < w; x++) {
                    const size_t k = (size_t)y * w + x;
                    depth[k] = (unsigned short)(1500 + 2 * x + y);
                    const int u = x + f;
                    rgb[k * 3] = (unsigned char)(40 + ((u / 8 + y / 8) % 2) * 120 + (u * 3) % 40);
                    rgb[k * 3 + 1] = (unsigned char)(60 + (y * 5) % 150);
                    rgb[k * 3 + 2] = (unsigned char)(30 + (u * 7 + y * 3) % 200);
                }
            ef.processFrame(rgb.data(), depth.data(), (int64_t)f * 33333, nullptr);
        }
        ef.setFrameToFrameRGB(false);
        ef.processFrame(rgb.data(), depth.data(), (int64_t)3 * 33333, nullptr);
        float rs[12];
        if (ifx_reloc_state(ef.handle(), rs) != IFX_OK) return 3;
        std::printf("frames 4 surfels %d lost %d fused %d\n", ifx_map_count(ef.handle()), (int)ef.getLost(), (int)rs[11]);
        return 0;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
