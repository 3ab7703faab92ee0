// Host check of instancefusion_amd/csrc/ifx_walk_owner.h (tests/test_walk_owner_cpu.py; g++ -fsanitize=address,undefined, no GPU).
//   walk_owner_check          every case below; prints "<cases> vectors, <candidates> candidates, <lattice tests> lattice tests, <n> bad"
//   walk_owner_check carry    the same with a deliberately WRONG carry (the first lane's owner leaves a step, not the last lane's): lists the cases that catch it
// The new lookup is run as the kernel runs it -- table, scatter of the marks, gather + clear, the six scan steps through wo_scan_src, carry -- and compared for every
// candidate g in [0, total) with a literal transcription of the two loops it replaces (the record) and with excl[] (the box's first candidate, which the mark brings).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ifx_walk_owner.h"

static const int L = IFX_WO_LANES;
static bool g_wrong_carry = false;

// the search k_raster_view had: two data-dependent scalar loops over readlane(incl, j) / readlane(excl, j); mine[] for every lane of the step at g0
struct OldWalk {
    int jlo = 0;
    void step(const int* incl, const int* excl, int g0, int* mine)
    {
        while (jlo < 63 && incl[jlo] <= g0) jlo++;
        for (int lane = 0; lane < L; lane++) mine[lane] = jlo;
        for (int j = jlo + 1; j < 64; j++) {
            const int ej = excl[j];
            if (ej >= g0 + 64) break;
            for (int lane = 0; lane < L; lane++)
                if (g0 + lane >= ej) mine[lane] = j;
        }
    }
};

// the new lookup, lane by lane as the wave does it
struct NewWalk {
    int tab[L];
    int carry = IFX_WO_IDENTITY;
    NewWalk() { for (int l = 0; l < L; l++) tab[l] = IFX_WO_IDENTITY; }
    bool step(const int* mark, int g0, int* mine)
    {
        bool ok = true;
        for (int lane = 0; lane < L; lane++) {   // scatter
            const int sl = wo_slot(mark[lane], g0);
            if (sl >= 0) {
                if (tab[sl] != IFX_WO_IDENTITY) ok = false;   // two boxes at one slot
                tab[sl] = mark[lane];
            }
        }
        int v[L], w[L];
        for (int lane = 0; lane < L; lane++) { v[lane] = tab[lane]; tab[lane] = IFX_WO_IDENTITY; }   // gather + clear
        for (int s = 0; s < IFX_WO_SCAN_STEPS; s++) {
            for (int lane = 0; lane < L; lane++) {
                const int src = wo_scan_src(s, lane);
                w[lane] = wo_join(v[lane], src >= 0 ? v[src] : IFX_WO_IDENTITY);
            }
            memcpy(v, w, sizeof(v));
        }
        for (int lane = 0; lane < L; lane++) mine[lane] = wo_owner(v[lane], carry);
        carry = g_wrong_carry ? mine[0] : mine[L - 1];
        return ok;
    }
};

static long long n_vec = 0, n_cand = 0, n_bad = 0;
static std::vector<std::string> caught;

static void check(const char* name, const std::vector<int>& area)
{
    int incl[L], excl[L], mark[L];
    long long run = 0;
    for (int j = 0; j < L; j++) { excl[j] = (int)run; run += area[j]; incl[j] = (int)run; mark[j] = wo_mark(excl[j], area[j], j); }
    const int total = incl[L - 1];
    OldWalk o;
    NewWalk w;
    long long bad = 0;
    int cnt = 0;
    for (int g0 = 0; g0 < total; g0 += 64) {
        int mo[L], mn[L];
        o.step(incl, excl, g0, mo);
        if (!w.step(mark, g0, mn)) bad++;
        for (int lane = 0; lane < L && g0 + lane < total; lane++) {
            const int g = g0 + lane;
            while (cnt < L && incl[cnt] <= g) cnt++;   // the definition, #{ j : incl[j] <= g }: incl[] does not decrease and g only grows
            const bool fine = cnt < L && wo_lane(mn[lane]) == mo[lane] && wo_lane(mn[lane]) == cnt && wo_first(mn[lane]) == excl[cnt] && area[cnt] > 0 && excl[cnt] <= g && g < incl[cnt];
            if (!fine) {
                if (bad < 3 && !g_wrong_carry) printf("  %s: g %d new %d (first %d) old %d count %d\n", name, g, wo_lane(mn[lane]), wo_first(mn[lane]), mo[lane], cnt);
                bad++;
            }
            n_cand++;
        }
    }
    for (int l = 0; l < L; l++)
        if (w.tab[l] != IFX_WO_IDENTITY) bad++;   // the table is left clear
    n_vec++;
    if (bad) {
        n_bad++;
        if (caught.empty() || caught.back() != name) caught.push_back(name);
    }
}

static std::vector<int> zeros() { return std::vector<int>(L, 0); }

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

int main(int argc, char** argv)
{
    g_wrong_carry = argc > 1 && std::string(argv[1]) == "carry";
    {   // all zero: no step at all
        check("all zero", zeros());
    }
    for (int pos : {0, 63})   // a single non-zero lane at 0 or at 63
        for (int a : {1, 5, 64, 200}) {
            auto v = zeros(); v[pos] = a;
            check(pos == 0 ? "single lane 0" : "single lane 63", v);
        }
    check("all ones", std::vector<int>(L, 1));   // 64 box starts in one step
    for (int a : {1, 63, 64, 65, 4096, 512 * 512})   // one area of each size, alone and among ones, at several lanes
        for (int pos : {0, 1, 31, 62, 63}) {
            if (a == 512 * 512 && (pos == 1 || pos == 62)) continue;
            auto v = zeros(); v[pos] = a;
            check("one area alone", v);
            auto u = std::vector<int>(L, 1); u[pos] = a;
            check("one area among ones", u);
        }
    {   // the largest first candidate there is: 63 boxes of IFX_MAX_SPRITE squared in front of a small one (62 of them stepped through by their size alone)
        auto v = std::vector<int>(L, 512 * 512); v[L - 1] = 3;
        long long run = 0; int m = 0;
        for (int j = 0; j < L; j++) { m = wo_mark((int)run, v[j], j); run += v[j]; }
        if (wo_lane(m) != 63 || wo_first(m) != 63 * 512 * 512 || m < 0) { printf("  the largest mark does not fit\n"); n_bad++; }
        for (int j = 2; j < L - 2; j++) v[j] = 0;
        check("large boxes", v);
    }
    for (int sum : {63, 64, 65, 127, 128, 129})   // sums landing exactly on a step boundary, and one short of / past it
        for (int parts : {1, 2, 3, 7, 64}) {
            if (parts > sum) continue;
            auto v = zeros();
            int left = sum;
            for (int k = 0; k < parts; k++) { const int a = k == parts - 1 ? left : sum / parts; v[(k * 9) % L] += a; left -= a; }
            check("sum on a step boundary", v);
            auto u = zeros();   // the same amounts in the LAST lanes
            for (int k = 0; k < L; k++) u[L - 1 - k] = v[k];
            check("sum on a step boundary", u);
        }
    for (int run : {1, 2, 31, 61})   // runs of empty boxes straddling a step boundary: a box ends exactly at, one before and one behind the boundary, then the run
        for (int first : {62, 63, 64, 65, 66, 127, 128, 129}) {
            auto v = zeros();
            v[0] = first;
            v[1 + run] = 3; v[2 + run] = 64; if (3 + run < L) v[3 + run] = 1;
            check("empty run across a boundary", v);
            auto u = zeros();
            u[1] = first; u[2 + run] = 70;
            check("empty run across a boundary", u);
        }
    for (int it = 0; it < 6000; it++) {   // seeded random vectors mixing 0, 1, 2 and large
        std::vector<int> v(L);
        const int kind = it % 6;
        for (int j = 0; j < L; j++) {
            const uint32_t r = rnd() % 100;
            int a;
            if (kind == 0) a = r < 40 ? 0 : (r < 70 ? 1 : 2);
            else if (kind == 1) a = r < 80 ? 0 : 1 + (int)(rnd() % 300);
            else if (kind == 2) a = r < 30 ? 0 : (r < 60 ? 1 : (r < 80 ? 2 : 1 + (int)(rnd() % 100)));
            else if (kind == 3) a = r < 10 ? 0 : 1 + (int)(rnd() % 40);
            else if (kind == 4) a = r < 50 ? 0 : (r < 97 ? 1 + (int)(rnd() % 3) : 1 + (int)(rnd() % 5000));
            else a = r < 90 ? (int)(rnd() % 3) : (r < 99 ? 64 * (1 + (int)(rnd() % 3)) - (int)(rnd() % 2) : (it % 60 == 5 ? 512 * 512 : 4096 + (int)(rnd() % 4096)));
            v[j] = a;
        }
        check("random", v);
    }
    // lattice test: every x in [0, 65535], every step in [1, 64]
    long long n_lat = 0, bad_lat = 0;
    for (int d = 1; d <= 64; d++) {
        const unsigned int m = wo_lattice_magic(d);
        for (int x = 0; x <= 65535; x++) {
            if (wo_on_lattice(x, m) != (x % d == 0)) bad_lat++;
            n_lat++;
        }
    }
    if (g_wrong_carry) {
        printf("wrong carry caught by:");
        for (auto& c : caught) printf(" [%s]", c.c_str());
        printf("\n");
    }
    printf("%lld vectors, %lld candidates, %lld lattice tests, %lld bad\n", n_vec, n_cand, n_lat, n_bad + bad_lat);
    return (n_bad + bad_lat) ? 1 : 0;
}
