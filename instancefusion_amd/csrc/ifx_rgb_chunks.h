// Chunks of the fused photometric step (ifx_track.hip, k_icp_residual<.., FUSE>): the records [0, n) of a level's candidate list are stepped in chunks of
// RGB_CHUNK records, which the photometric blocks claim from an atomic counter.  Thread t of the claiming block takes the records first + t + u * threads,
// u = 0 .. RGB_CHUNK_IT - 1, that lie below `end`.  Plain integer arithmetic, shared with the host check (tests/cpp/rgb_chunks_check.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IFX_HD __host__ __device__
#else
#define IFX_HD
#endif

#define RGB_CHUNK_THREADS 256   // = RED_THREADS
#define RGB_CHUNK_IT 2          // records per thread and chunk (four, the two-launch step's number, does not fit the fused kernel's 128 VGPRs beside the 29 f64 sums)
#define RGB_CHUNK (RGB_CHUNK_THREADS * RGB_CHUNK_IT)

struct RgbChunk { int first, end; };   // records [first, end), end - first <= RGB_CHUNK; empty past the list

// the number of records a run steps: the device's count clamped to the list's capacity (a slot that is being rewritten under a dropped run may show any count)
IFX_HD inline int rgb_chunk_n(unsigned int cand_n, int capacity)
{
    const unsigned int cap = capacity > 0 ? (unsigned int)capacity : 0u;
    return (int)(cand_n < cap ? cand_n : cap);
}
IFX_HD inline int rgb_chunk_count(int n) { return n <= 0 ? 0 : (n - 1) / RGB_CHUNK + 1; }
IFX_HD inline RgbChunk rgb_chunk_range(unsigned int chunk, int n)
{
    RgbChunk r;
    const unsigned int count = (unsigned int)rgb_chunk_count(n);
    if (chunk >= count) { r.first = n > 0 ? n : 0; r.end = r.first; return r; }   // (the claim that tells a block that nothing is left)
    r.first = (int)chunk * RGB_CHUNK;                                             // chunk < count <= 2^31 / RGB_CHUNK: no overflow
    r.end = n - r.first < RGB_CHUNK ? n : r.first + RGB_CHUNK;
    return r;
}
