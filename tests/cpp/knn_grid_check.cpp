// Grid arithmetic of the kNN search (instancefusion_amd/csrc/ifx_knn_grid.h) on the CPU, under AddressSanitizer + UBSan (tests/test_knn_grid_cpu.py):
//  - knn_grid_side: monotone in the count, within [2, 256], side^3 <= max(8, 8 * count), 256 from 2^21 points on;
//  - the cells of a shell row: the loop the vote kernels run yields exactly the cells of the run [max(c - r, 0), min(c + r, dim - 1)] that are new in shell r -- all of
//    them on a face of the shell, the ones with |x - c| == r off a face -- each once; and walking the shells r = 0, 1, ... as the kernels do visits every cell of a
//    grid exactly once, in the shell of its Chebyshev distance from the query's cell.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ifx_knn_grid.h"

static int bad = 0, cases = 0;

static void check_side(int count, int prev_side)
{
    const int s = knn_grid_side(count);
    const long long room = count > 0 ? 8LL * count : 0, cap = room > 8 ? room : 8;
    cases++;
    if (s < 2 || s > 256) { std::printf("side(%d) = %d outside [2, 256]\n", count, s); bad++; return; }
    if ((long long)s * s * s > cap) { std::printf("side(%d) = %d: %lld cells > %lld\n", count, s, (long long)s * s * s, cap); bad++; }
    if (s < prev_side) { std::printf("side(%d) = %d below the side of a smaller count, %d\n", count, s, prev_side); bad++; }
    if (count >= (1 << 21) && s != 256) { std::printf("side(%d) = %d, not 256\n", count, s); bad++; }
}

static void check_row(int c, int r, int dim, bool face)
{
    std::vector<unsigned char> hit((size_t)dim, 0);   // (exactly dim bytes: a cell outside the grid is a heap overflow the sanitizer reports)
    int trips = 0;
    const int last = knn_row_last(c, r, dim), step = knn_row_step(r, face);
    if (step < 1) { std::printf("row c %d r %d dim %d face %d: step %d\n", c, r, dim, (int)face, step); bad++; return; }
    for (int x = knn_row_first(c, r, face); x <= last; x += step) {
        if (x < 0 || x >= dim) { std::printf("row c %d r %d dim %d face %d: cell %d outside the grid\n", c, r, dim, (int)face, x); bad++; return; }
        hit[(size_t)x]++;
        if (++trips > dim) break;
    }
    for (int x = 0; x < dim; x++) {
        const bool in_run = x >= c - r && x <= c + r;
        const int want = in_run && (face || std::abs(x - c) == r) ? 1 : 0;
        if (hit[(size_t)x] != want) { std::printf("row c %d r %d dim %d face %d: cell %d visited %d times, expected %d\n", c, r, dim, (int)face, x, (int)hit[(size_t)x], want); bad++; }
    }
    cases++;
}

// the shell walk of k_knn_vote / k_knnx_vote around the cell (cx, cy, cz) of a dx x dy x dz grid, without its early exit
static void check_walk(int cx, int cy, int cz, int dx, int dy, int dz)
{
    std::vector<int> shell((size_t)dx * dy * dz, -1);
    const int c[3] = {cx, cy, cz};
    const int rmax = dx > dy ? (dx > dz ? dx : dz) : (dy > dz ? dy : dz);
    for (int r = 0; r <= rmax; r++)
        for (int z = (c[2] - r > 0 ? c[2] - r : 0); z <= (c[2] + r < dz - 1 ? c[2] + r : dz - 1); z++)
            for (int y = (c[1] - r > 0 ? c[1] - r : 0); y <= (c[1] + r < dy - 1 ? c[1] + r : dy - 1); y++) {
                const bool face = std::abs(z - c[2]) == r || std::abs(y - c[1]) == r;
                const int x1 = knn_row_last(c[0], r, dx), xs = knn_row_step(r, face);
                for (int x = knn_row_first(c[0], r, face); x <= x1; x += xs) {
                    int& s = shell[(size_t)((z * dy + y) * dx + x)];
                    if (s != -1) { std::printf("walk (%d %d %d) in %d x %d x %d: cell (%d %d %d) again in shell %d after %d\n", cx, cy, cz, dx, dy, dz, x, y, z, r, s); bad++; return; }
                    s = r;
                }
            }
    for (int z = 0; z < dz; z++)
        for (int y = 0; y < dy; y++)
            for (int x = 0; x < dx; x++) {
                const int ax = std::abs(x - cx), ay = std::abs(y - cy), az = std::abs(z - cz), want = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
                if (shell[(size_t)((z * dy + y) * dx + x)] != want) {
                    std::printf("walk (%d %d %d) in %d x %d x %d: cell (%d %d %d) in shell %d, expected %d\n", cx, cy, cz, dx, dy, dz, x, y, z, shell[(size_t)((z * dy + y) * dx + x)], want);
                    bad++; return;
                }
            }
    cases++;
}

int main()
{
    const int counts[] = {0, 1, 2, 9, 10, 11, 4096, (1 << 21) - 1, 1 << 21, INT_MAX};
    int prev = 0;
    for (int n : counts) { check_side(n, prev); prev = knn_grid_side(n); }
    check_side(-1, 0); check_side(INT_MIN, 0);      // (a count is never negative; the function still answers 2)
    if (knn_grid_side(0) != 2 || knn_grid_side(1) != 2 || knn_grid_side(4096) != 32 || knn_grid_side((1 << 21) - 1) != 255) {
        std::printf("side: %d %d %d %d for 0, 1, 4096, 2^21 - 1; expected 2 2 32 255\n", knn_grid_side(0), knn_grid_side(1), knn_grid_side(4096), knn_grid_side((1 << 21) - 1));
        bad++;
    }
    prev = 0;
    for (int n = 0; n <= (1 << 21) + 4096; n += (n < 70000 ? 1 : 997)) { check_side(n, prev); prev = knn_grid_side(n); }   // monotone over every small count, sampled above
    for (int dim = 1; dim <= 12; dim++)
        for (int c = 0; c < dim; c++)
            for (int r = 0; r <= dim + 2; r++) {
                check_row(c, r, dim, true);
                if (r > 0) check_row(c, r, dim, false);   // (in shell 0 the one row is on a face)
            }
    for (int dim : {255, 256})
        for (int c : {0, 1, 127, dim - 2, dim - 1})
            for (int r : {1, 2, 127, 128, dim - 1, dim}) { check_row(c, r, dim, true); check_row(c, r, dim, false); }
    const int dims[][3] = {{1, 1, 1}, {2, 1, 1}, {1, 2, 1}, {1, 1, 3}, {5, 1, 1}, {4, 3, 1}, {1, 4, 3}, {5, 4, 3}, {3, 4, 5}, {6, 6, 6}, {7, 2, 5}};
    for (const auto& d : dims)
        for (int z = 0; z < d[2]; z++)
            for (int y = 0; y < d[1]; y++)
                for (int x = 0; x < d[0]; x++) check_walk(x, y, z, d[0], d[1], d[2]);
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
