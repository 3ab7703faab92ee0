// Shares of the own-records form of the fused photometric step (ifx_track.hip, k_icp_residual<.., FUSE, OWN>, option rgb_own): the records [0, n) of a level's
// candidate list are stepped by the G photometric blocks that wrote them.  Thread `tid` of block `b` has the records first + k * G * threads below n, k = 0 ..
// rounds - 1: round 0 is the record the thread computed in its residual pass and still holds in registers, the later rounds are read back from memory.  The
// assignment is static: a block that stopped waiting at the meeting hands its whole share to the last arriver through two mask words, a bit per block, hence the
// cap on G.  Plain integer arithmetic, shared with the host check (tests/cpp/rgb_own_check.cpp).
#pragma once

#include "ifx_rgb_chunks.h"   // IFX_HD, RGB_CHUNK_THREADS, rgb_chunk_n (the clamp of the device's count to the list's capacity)

#define RGB_OWN_MAX_G 64   // photometric blocks of an own-records launch: one bit each in a 64-bit orphan mask and a 64-bit taken mask (a launch with more runs the chunk form)
#define RGB_OWN_IT 2       // read-back records in flight per thread (= RGB_CHUNK_IT: the fused kernel's register budget)

// the first record of thread `tid` of block `b` (b < G <= 2^22: no overflow)
IFX_HD inline int rgb_own_first(int b, int tid) { return b * RGB_CHUNK_THREADS + tid; }
// the records a thread with first record `first` has below n: first + k * g * threads < n (written so that nothing can overflow for any n, first >= 0 and g <= 2^22)
IFX_HD inline int rgb_own_rounds(int n, int g, int first)
{
    if (g <= 0 || first < 0 || first >= n) return 0;
    return (n - 1 - first) / (g * RGB_CHUNK_THREADS) + 1;
}
// ... and record k of them, k < rgb_own_rounds: below n, so no overflow
IFX_HD inline int rgb_own_record(int g, int first, int k) { return first + k * (g * RGB_CHUNK_THREADS); }
// the rounds block `b` runs: its thread 0 has the most (0: the block has no record at all -- it still arrives at the meeting)
IFX_HD inline int rgb_own_block_rounds(int n, int g, int b) { return rgb_own_rounds(n, g, rgb_own_first(b, 0)); }
