// Stand-alone check of instancefusion_amd/host/ifx_detector_prep.hpp (the host arithmetic of ifx_detector_input_size / ifx_detector_resize_taps), meant to be built
// with -fsanitize=address,undefined: the tap tables at their extremes in exactly-sized heap buffers, so that a write past count, past ksize or past out_size is
// caught.  Prints one line per table -- "taps <in> <out> <ksize> <max count> <min first> <max last>" -- and "ok", or "FAIL ..." and a non-zero status.
//   detector_prep_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ifx_detector_prep.hpp"

static int fails = 0;
#define CHECK(c, ...)                                             \
    do {                                                          \
        if (!(c)) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); fails++; } \
    } while (0)

static void table(int in, int out)
{
    const int ks = ifx_detprep::resize_ksize(in, out);
    // exactly-sized heap blocks: the sanitizer sees the first byte past each
    int32_t* first = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)out);
    int32_t* count = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)out);
    int32_t* coeff = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)out * (size_t)ks);
    const int got = ifx_detprep::resize_taps(in, out, first, count, coeff, ks);
    CHECK(got == ks, "ksize %d != %d (%d -> %d)", got, ks, in, out);
    int max_n = 0, min_f = in, max_l = 0;
    for (int i = 0; got == ks && i < out; i++) {
        CHECK(first[i] >= 0 && count[i] >= 1 && count[i] <= ks && first[i] + count[i] <= in, "taps of %d leave the input (%d -> %d): first %d count %d", i, in, out, first[i], count[i]);
        CHECK(i == 0 || (first[i] >= first[i - 1] && first[i] + count[i] >= first[i - 1] + count[i - 1]), "taps of %d go backwards (%d -> %d)", i, in, out);
        long long sum = 0;
        for (int k = 0; k < ks; k++) {
            const int32_t c = coeff[(size_t)i * ks + k];
            CHECK(c >= 0 && (k < count[i] || c == 0), "coefficient %d of %d (%d -> %d) is %d", k, i, in, out, (int)c);
            sum += c;
        }
        // rounded to the nearest unit each: the sum is 2^22 give or take half a unit per tap (what keeps the kernel's 32-bit sums exact)
        CHECK(sum >= (1 << 22) - (ks + 1) / 2 && sum <= (1 << 22) + (ks + 1) / 2, "coefficients of %d (%d -> %d) add up to %lld", i, in, out, sum);
        if (count[i] > max_n) max_n = count[i];
        if (first[i] < min_f) min_f = first[i];
        if (first[i] + count[i] > max_l) max_l = first[i] + count[i];
    }
    std::printf("taps %d %d %d %d %d %d\n", in, out, ks, max_n, min_f, max_l);
    // one tap too few for the caller's buffers: refused, nothing written (the blocks are too small for a write to go unnoticed)
    CHECK(ifx_detprep::resize_taps(in, out, first, count, coeff, ks - 1) == -1, "max_ksize %d accepted (%d -> %d)", ks - 1, in, out);
    std::free(first); std::free(count); std::free(coeff);
}

int main()
{
    table(1, 1);        // in = 1, out = 1
    table(1, 16);       // scale 1/16 out of a single sample
    table(10, 160);     // scale 1/16
    table(640, 1);      // out = 1
    table(17, 1);
    table(160, 20);     // scale 8: 17 taps
    table(161, 20);     // just above: 19
    table(120, 16);     // 7.5
    table(640, 682);
    table(480, 800);
    table(7, 7);        // an identity pass: (2^22, 0)
    CHECK(ifx_detprep::resize_taps(0, 4, nullptr, nullptr, nullptr, 17) == -1, "in = 0 accepted");
    CHECK(ifx_detprep::resize_taps(4, 0, nullptr, nullptr, nullptr, 17) == -1, "out = 0 accepted");
    // the size rule at its corners
    ifx_detector_prep p = {512, 0, 32, 0, {0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}};
    int32_t o[4];
    CHECK(!ifx_detprep::input_size(640, 480, &p, o) && o[0] == 682 && o[1] == 512 && o[2] == 704 && o[3] == 512, "640x480 min 512: %d %d %d %d", o[0], o[1], o[2], o[3]);
    p.min_size = 800;
    CHECK(!ifx_detprep::input_size(640, 480, &p, o) && o[0] == 1066 && o[1] == 800 && o[2] == 1088 && o[3] == 800, "640x480 min 800: %d %d %d %d", o[0], o[1], o[2], o[3]);
    p.min_size = 100; p.max_size = 120; p.size_divisible = 0;
    CHECK(!ifx_detprep::input_size(160, 120, &p, o) && o[0] == 120 && o[1] == 90 && o[2] == 120 && o[3] == 90, "160x120 min 100 max 120: %d %d", o[0], o[1]);
    p.max_size = 90;    // 67.5 -> 68, half to even
    CHECK(!ifx_detprep::input_size(160, 120, &p, o) && o[1] == 68, "max 90: %d", o[1]);
    p.max_size = 94;    // 70.5 -> 70
    CHECK(!ifx_detprep::input_size(160, 120, &p, o) && o[1] == 70, "max 94: %d", o[1]);
    p.min_size = 2147483647; p.max_size = 0; p.size_divisible = 2147483647;   // no 32-bit product on the way
    CHECK(ifx_detprep::input_size(2147483647, 3, &p, o) != nullptr, "an output beyond 2^31 accepted");
    p.min_size = 1; p.max_size = 1; p.size_divisible = 0;
    CHECK(ifx_detprep::input_size(4000, 3, &p, o) != nullptr, "an empty output accepted");
    p.min_size = 0;
    CHECK(ifx_detprep::input_size(64, 48, &p, o) != nullptr, "min_size 0 accepted");
    CHECK(ifx_detprep::input_size(64, 48, nullptr, o) != nullptr, "NULL parameters accepted");
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
