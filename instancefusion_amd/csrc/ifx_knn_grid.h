// Grid arithmetic of the kNN search (ifx_knn.hip): how many cells the bounding box's longest side is cut into, and which cells of a row of the shell at Chebyshev
// distance r around the query's cell are new.  The search is exact for any cell size (a query walks shells until its 10th candidate is closer than the inner border
// of the next one), so the side shows in the cost only: a grid far finer than the cloud makes a query that finds nothing nearby walk empty cells, sum (2r+1)^3 of them.
// Plain integer arithmetic (a double cube root as the first guess only), shared with the host check (tests/cpp/knn_grid_check.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IFX_HD __host__ __device__
#else
#define IFX_HD
#endif

#define KNN_GRID_MAX 256     // cells along the longest side at most: the buffers of a call are sized for KNN_GRID_MAX^3 cells, a smaller grid uses a prefix
#define KNN_GRID_FACTOR 8    // cells per point the grid may have at most: side^3 <= KNN_GRID_FACTOR * count (the k_knn_* row)

// cells along the longest side for `count` points (an upper bound of the live ones does): the largest side in [2, KNN_GRID_MAX] with side^3 <= max(8, FACTOR * count).
// Never 1: the cell size is extent / (side - 1).  Monotone in count; KNN_GRID_MAX from count = KNN_GRID_MAX^3 / KNN_GRID_FACTOR (2^21) on.
IFX_HD inline int knn_grid_side(int count)
{
    const long long room = (long long)KNN_GRID_FACTOR * (count > 0 ? count : 0);
    if (room >= (long long)KNN_GRID_MAX * KNN_GRID_MAX * KNN_GRID_MAX) return KNN_GRID_MAX;
    long long side = (long long)cbrt((double)room);   // within one of the integer cube root, whatever the library's last bit: the two loops settle it
    while ((side + 1) * (side + 1) * (side + 1) <= room) side++;
    while (side * side * side > room) side--;
    return side < 2 ? 2 : (int)side;
}

// the cells x of a row of the shell r around the cell c (0 <= c < dim, r >= 0): on a face of the shell (|y - cy| == r or |z - cz| == r) the whole run
// [max(c - r, 0), min(c + r, dim - 1)] is new, off a face only the cells with |x - c| == r are -- c - r and c + r, each if it is inside the grid.
//     for (int x = knn_row_first(c, r, face); x <= knn_row_last(c, r, dim); x += knn_row_step(r, face)) ...
IFX_HD inline int knn_row_first(int c, int r, bool face) { return c - r >= 0 ? c - r : (face ? 0 : c + r); }
IFX_HD inline int knn_row_last(int c, int r, int dim) { return c + r < dim - 1 ? c + r : dim - 1; }
IFX_HD inline int knn_row_step(int r, bool face) { return face || r == 0 ? 1 : 2 * r; }
