// Index arithmetic of k_raster_view's flattened pixel loop (ifx_map.hip), kept free of intrinsics so that a host program runs the same text
// (tests/test_walk_owner_cpu.py).
//
// A wave prepares 64 surfels; lane j's pixel box has area[j] >= 0 candidates, incl[] / excl[] are the inclusive / exclusive prefix sums and total = incl[63].
// The wave walks the concatenation of all boxes 64 candidates a step: lane l of the step that starts at g0 tests candidate g = g0 + l, which belongs to surfel
//     owner(g) = #{ j : incl[j] <= g }        (for g < total: the one j with excl[j] <= g < incl[j]; that j has area[j] > 0)
//              = max{ j : area[j] > 0 and excl[j] <= g }.
// The second form is computed without a loop over j or a branch on data.  A box is named by ONE word, its mark (excl[j] << 6) | j: among the boxes of positive area
// excl[] and j grow together, so the largest mark is the mark of the largest j, and it hands the lane the box's first candidate together with its number.
//   1. scatter   every lane j whose box STARTS inside the step (area[j] > 0, g0 <= excl[j] < g0 + 64) writes its mark to slot excl[j] - g0 of a 64-entry table of the
//                wave.  Boxes of positive area start at distinct candidates, so the slots are distinct; every other slot holds 0.
//   2. gather    lane l takes slot l and puts 0 back (the table is clear again for the next step).
//   3. max-scan  an inclusive maximum over lanes 0..l: the last box that starts at or before candidate g0 + l INSIDE this step (0 if none: 0 is the identity of the
//                maximum over marks, and the one real mark 0 -- lane 0's box at candidate 0 -- is the smallest there is).
//   4. carry     the maximum with the mark of the previous step's last candidate, which covers a box that started before g0.  Marks never decrease along g, so the
//                carry is a lower bound of every mark of this step and the maximum is the owner's.  The first step's carry is 0.
// The carry that leaves a step is lane 63's mark.  In the last step the lanes with g >= total hold the last box's mark; they test nothing.
// Range: an area is at most 512 x 512 (IFX_MAX_SPRITE squared), so excl <= 63 * 2^18 < 2^24 and a mark is below 2^30.
#ifndef IFX_WALK_OWNER_H
#define IFX_WALK_OWNER_H

#if defined(__HIPCC__)
#define IFX_WO_FN __host__ __device__ __forceinline__
#else
#define IFX_WO_FN static inline
#endif

#define IFX_WO_LANES 64
#define IFX_WO_IDENTITY 0

// What lane j keeps for the scatter: its box's mark, or -1 for an empty box (never inside a step: g0 >= 0).
IFX_WO_FN int wo_mark(int excl, int area, int j) { return area > 0 ? (excl << 6) | j : -1; }
// A mark's two halves: the record to read, and the box's first candidate (what g is counted from).
IFX_WO_FN int wo_lane(int mark) { return mark & 63; }
IFX_WO_FN int wo_first(int mark) { return mark >> 6; }
// Slot of the table a lane writes its mark to in the step starting at g0, or -1: no write.  (As unsigned: a start before g0, the -1 of an empty box included, wraps above 63.)
IFX_WO_FN int wo_slot(int mark, int g0) { const unsigned int d = (unsigned int)(mark >> 6) - (unsigned int)g0; return d < (unsigned int)IFX_WO_LANES ? (int)d : -1; }
// The scan's operator.
IFX_WO_FN int wo_join(int a, int b) { return a > b ? a : b; }
// Step 4: the candidate's mark from the scanned slot and the carry.
IFX_WO_FN int wo_owner(int scanned, int carry) { return wo_join(scanned, carry); }

// The six steps of the scan as the kernel issues them (gfx9 DPP: row_shr 1, 2, 4, 8 inside rows of 16 lanes, then row_bcast15 into rows 1 and 3 and row_bcast31 into
// rows 2 and 3): the lane whose value lane `lane` joins to its own in step `step`, or -1 for none (it joins the identity).
#define IFX_WO_SCAN_STEPS 6
IFX_WO_FN int wo_scan_src(int step, int lane)
{
    if (step < 4) { const int s = 1 << step; return (lane & 15) >= s ? lane - s : -1; }
    if (step == 4) return (lane & 16) ? (lane & ~15) - 1 : -1;   // lanes 16..31 take lane 15, lanes 48..63 lane 47
    return lane >= 32 ? 31 : -1;
}

// ---- lattice membership: x % d == 0 for 0 <= x < 2^16 and 2 <= d <= 2^14, without a division.
// m = ceil(2^32 / d) = (2^32 + e) / d with 0 <= e < d.  Write x = q d + r, 0 <= r < d.  Then x m = q 2^32 + q e + r m, and
//   q e <= x < 2^16;   r m <= (d - 1)(2^32 + e) / d = 2^32 + e - m;   so q e + r m < 2^32 + (2^16 + d) - m <= 2^32, as m >= 2^18 > 2^16 + d for d <= 2^14.
// The low 32 bits of x m are therefore q e + r m exactly: below 2^16 < m when r = 0, at least m when r >= 1.  Hence x % d == 0  <=>  (uint32)(x m) < m.
// d <= 1: every x is a multiple; the magic is 0 and says so.
IFX_WO_FN unsigned int wo_lattice_magic(int d) { return d > 1 ? 0xFFFFFFFFu / (unsigned int)d + 1u : 0u; }
IFX_WO_FN bool wo_on_lattice(int x, unsigned int m) { return m == 0u || (unsigned int)x * m < m; }

#endif
