// Stand-alone check of ifx_pyramid_level_thresholds' host arithmetic (instancefusion_amd/host/ifx_detector_prep.hpp), meant to be built with
// -fsanitize=address,undefined: the three thresholds of a list of image sizes in an exactly-sized heap buffer, their order, and the refusals.  Prints one line per
// size -- "thr <image_h> <image_w> <T0> <T1> <T2>" as f32 bit patterns in hex -- and "ok", or "FAIL ..." and a non-zero status.
//   keras_levels_check
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ifx_detector_prep.hpp"

static int fails = 0;
#define CHECK(c, ...)                                             \
    do {                                                          \
        if (!(c)) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); fails++; } \
    } while (0)

int main()
{
    const int sizes[8][2] = {{1024, 1024}, {64, 64}, {512, 640}, {1, 1}, {800, 1333}, {46340, 46340}, {2147483647, 2147483647}, {1, 2147483647}};
    for (const auto& s : sizes) {
        float* t = (float*)std::malloc(3 * sizeof(float));
        const char* bad = ifx_detprep::pyramid_level_thresholds(s[0], s[1], t);
        CHECK(!bad, "%d x %d refused: %s", s[0], s[1], bad ? bad : "");
        CHECK(t[0] > 0.f && t[0] < t[1] && t[1] < t[2], "%d x %d: the thresholds do not ascend", s[0], s[1]);
        uint32_t u[3];
        std::memcpy(u, t, sizeof u);
        std::printf("thr %d %d %08x %08x %08x\n", s[0], s[1], u[0], u[1], u[2]);
        std::free(t);
    }
    float t[3];
    CHECK(ifx_detprep::pyramid_level_thresholds(0, 64, t) != nullptr, "image_h 0 accepted");
    CHECK(ifx_detprep::pyramid_level_thresholds(64, -3, t) != nullptr, "image_w -3 accepted");
    CHECK(ifx_detprep::pyramid_level_thresholds(64, 64, nullptr) != nullptr, "NULL output accepted");
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
