// Stand-alone check of what ifx_unmold_detections and ifx_molded_input_size take from instancefusion_amd/host/ifx_detector_prep.hpp, meant to be built with
// -fsanitize=address,undefined: the tap tables of M -> 1 .. 160 for the mask sizes the tests use, in exactly-sized heap buffers, with the property the paste
// kernel's LDS rows rely on (never more than M taps reach a sample, whatever ksize is), and the molded size rule at its corners.  Prints one line per table --
// "taps <in> <out> <max count> <sum of 3 first + count> <coefficients weighted by position, mod 1000003>" -- and "ok", or "FAIL ..." and a non-zero status.
//   molded_prep_check
#include <cstdio>
#include <cstdlib>

#include "ifx_detector_prep.hpp"

static int fails = 0;
#define CHECK(c, ...)                                             \
    do {                                                          \
        if (!(c)) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); fails++; } \
    } while (0)

static void table(int in, int out)
{
    const int ks = ifx_detprep::resize_ksize(in, out);
    int32_t* first = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)out);
    int32_t* count = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)out);
    int32_t* coeff = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)out * (size_t)ks);
    const int got = ifx_detprep::resize_taps(in, out, first, count, coeff, ks);
    CHECK(got == ks && ks <= 2 * in + 1, "ksize %d != %d (%d -> %d)", got, ks, in, out);
    long long max_n = 0, pos = 0, weighted = 0;
    for (int i = 0; got == ks && i < out; i++) {
        CHECK(first[i] >= 0 && count[i] >= 1 && count[i] <= in && first[i] + count[i] <= in, "taps of %d leave the mask (%d -> %d): first %d count %d", i, in, out, first[i], count[i]);
        long long sum = 0;
        for (int k = 0; k < ks; k++) {
            const int32_t c = coeff[(size_t)i * ks + k];
            CHECK(c >= 0 && (k < count[i] || c == 0), "coefficient %d of %d (%d -> %d) is %d", k, i, in, out, (int)c);
            sum += c;
            weighted += (long long)c * (k + 1);
        }
        // 2^21 + 255 * sum < 2^31: the 32-bit accumulators of the two passes are exact
        CHECK(sum <= (1 << 22) + (count[i] + 1) / 2 && (1ll << 21) + 255 * sum < (1ll << 31), "coefficients of %d (%d -> %d) add up to %lld", i, in, out, sum);
        if (count[i] > max_n) max_n = count[i];
        pos += 3ll * first[i] + count[i];
    }
    std::printf("taps %d %d %lld %lld %lld\n", in, out, max_n, pos, weighted % 1000003);
    std::free(first); std::free(count); std::free(coeff);
}

static void size(int w, int h, int mn, int mx, int nw, int nh, int top, int left)
{
    int32_t o[8];
    const char* bad = ifx_detprep::molded_input_size(w, h, mn, mx, o);
    CHECK(!bad && o[0] == nw && o[1] == nh && o[2] == mx && o[3] == mx && o[4] == top && o[5] == left && o[6] == top + nh && o[7] == left + nw,
          "%d x %d (%d, %d): %s %d %d %d %d", w, h, mn, mx, bad ? bad : "", o[0], o[1], o[4], o[5]);
}

int main()
{
    const int sizes[5] = {1, 2, 27, 28, 64};
    for (int m : sizes)
        for (int out = 1; out <= 160; out++) table(m, out);
    size(640, 480, 512, 512, 512, 384, 64, 0);
    size(640, 480, 800, 1024, 1024, 768, 128, 0);
    size(480, 640, 800, 1024, 768, 1024, 0, 128);
    size(160, 120, 0, 160, 160, 120, 20, 0);       // no resize
    size(160, 120, 90, 94, 94, 70, 12, 0);         // 70.5 -> 70, half to even
    size(100, 76, 128, 129, 129, 98, 15, 0);       // 98.04 -> 98; (129 - 98) / 2 = 15, floor
    size(1, 1, 800, 1024, 800, 800, 112, 112);
    int32_t o[8];
    CHECK(ifx_detprep::molded_input_size(160, 120, 128, 0, o) != nullptr, "max_dim 0 accepted");
    CHECK(ifx_detprep::molded_input_size(160, 120, 0, 19, o) != nullptr, "a resize scale above 8 accepted");
    CHECK(ifx_detprep::molded_input_size(0, 120, 128, 128, o) != nullptr, "width 0 accepted");
    CHECK(ifx_detprep::molded_input_size(160, 120, 128, 128, nullptr) != nullptr, "NULL output accepted");
    CHECK(ifx_detprep::molded_input_size(2147483647, 2147483647, 2147483647, 2147483647, o) == nullptr && o[0] == 2147483647 && o[4] == 0, "the largest sizes");
    if (fails) return 1;
    std::printf("ok\n");
    return 0;
}
