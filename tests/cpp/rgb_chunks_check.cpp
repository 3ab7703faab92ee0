// Chunk arithmetic of the fused photometric step (instancefusion_amd/csrc/ifx_rgb_chunks.h) on the CPU, under AddressSanitizer + UBSan (tests/test_rgb_chunks_cpu.py):
// for a list of capacity `cap` and a device count `cand_n`, walking the chunks the way a claiming block does touches every index of [0, n) exactly once, n =
// min(cand_n, cap), and none at or beyond n -- including the claims past the last chunk, which every block draws once to learn that nothing is left.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ifx_rgb_chunks.h"

static int check(unsigned int cand_n, int cap, int extra_claims)
{
    const int n = rgb_chunk_n(cand_n, cap);
    if (n < 0 || n > cap || (cand_n <= (unsigned int)cap && n != (int)cand_n)) { std::printf("n: cand_n %u cap %d -> %d\n", cand_n, cap, n); return 1; }
    std::vector<unsigned char> hit((size_t)n, 0);   // (exactly n bytes: an index >= n is a heap overflow the sanitizer reports)
    const int chunks = rgb_chunk_count(n);
    for (unsigned int c = 0; c < (unsigned int)(chunks + extra_claims); c++) {
        const RgbChunk r = rgb_chunk_range(c, n);
        if (r.first < 0 || r.end < r.first || r.end > n || r.end - r.first > RGB_CHUNK) { std::printf("range: n %d chunk %u -> [%d, %d)\n", n, c, r.first, r.end); return 1; }
        if ((int)c < chunks && r.end == r.first) { std::printf("empty chunk %u of %d, n %d\n", c, chunks, n); return 1; }
        if ((int)c >= chunks && r.end != r.first) { std::printf("chunk %u past the list is not empty, n %d\n", c, n); return 1; }
        for (int t = 0; t < RGB_CHUNK_THREADS; t++)
            for (int u = 0; u < RGB_CHUNK_IT; u++) {
                const int k = r.first + t + u * RGB_CHUNK_THREADS;   // the thread's record, as in the kernel
                if (k < r.end) hit[(size_t)k]++;
            }
    }
    for (int k = 0; k < n; k++)
        if (hit[(size_t)k] != 1) { std::printf("index %d of %d covered %d times\n", k, n, (int)hit[(size_t)k]); return 1; }
    return 0;
}

int main()
{
    int bad = 0, cases = 0;
    const int caps[] = {40 * 30, 80 * 60, 160 * 120, 320 * 240, 640 * 480, 1, RGB_CHUNK, RGB_CHUNK + 1};
    for (int cap : caps) {
        const long long ns[] = {0, 1, 255, 256, 257, RGB_CHUNK - 1, RGB_CHUNK, RGB_CHUNK + 1, cap - 1, cap, (long long)cap + 1, 2LL * cap + 7, 0x7FFFFFFFLL, 0x80000000LL, 0xFFFFFFFFLL};
        for (long long n : ns) {
            if (n < 0) continue;
            bad += check((unsigned int)n, cap, 70);   // (more claims past the end than any grid has photometric blocks)
            cases++;
        }
    }
    bad += check(5u, 0, 3); cases++;   // a list without capacity
    // the claim counter itself can pass any value: far past the list, still empty and in range
    for (unsigned int c : {1u << 20, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu}) {
        const RgbChunk r = rgb_chunk_range(c, 640 * 480);
        if (r.first != r.end || r.end > 640 * 480) { std::printf("claim %u: [%d, %d)\n", c, r.first, r.end); bad++; }
        cases++;
    }
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
