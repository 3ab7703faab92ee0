// The own-records form of the fused photometric step (instancefusion_amd/csrc/ifx_rgb_own.h, option rgb_own) on the CPU, under AddressSanitizer + UBSan
// (tests/test_rgb_own_cpu.py).  Two parts.
//
// 1. The share arithmetic.  For G photometric blocks and a count n, thread tid of block b steps the records rgb_own_record(G, first, k), k < rgb_own_rounds(n, G,
//    first), first = rgb_own_first(b, tid).  Checked for every n in 0 .. 3 * G * 256 + 3 and G in {1, 2, 3, 32, 33, 64, 1024}:
//      - every n: record n - 1 has exactly one owner (thread (n - 1) mod G * 256, round (n - 1) div G * 256), that owner's round count went up by one from n - 1 and its
//        last record is n - 1; the owner's neighbours and the list's first and last thread did not move; the block's round count is its thread 0's;
//      - full walk, every thread of every block writing a hit array of exactly n bytes (an index >= n is a heap overflow the sanitizer reports), "covered exactly once":
//        at every n for G <= 3, and for the larger G at the n around every multiple of G * 256 and of 256 next to it (where a round or a block begins) and at the end.
//    Counts above the capacity and UINT_MAX go through rgb_chunk_n first, as in the kernel, with the hit array as long as the capacity.
//
// 2. The take-over protocol, as a model: G = 2 and 3 "blocks" whose memory operations -- the arrival add, a poll, the OR into the orphan mask, the re-load of the
//    arrival word, the OR into the taken mask; the last arriver's load of the orphan mask and its OR into the taken mask -- are single atomic steps on shared words,
//    run through EVERY interleaving, with a wait that may run out at any time (and the test switch rgb_fuse_poll = 0, where it has run out at once).  At the end of
//    every interleaving every share has been stepped exactly once, and the blocks that left are as many as the shares adopted.  A protocol without the re-load must
//    fail the same search: the model can see a lost share.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ifx_rgb_own.h"

static int bad = 0, cases = 0;
#define FAIL(...) do { if (bad < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } bad++; } while (0)

// every thread of every block walks its share of [0, n) over an array of exactly `size` bytes
static void full_walk(int n, int g, size_t size)
{
    std::vector<unsigned char> hit(size, 0);
    long long total = 0;
    for (int b = 0; b < g; b++) {
        const int block_rounds = rgb_own_block_rounds(n, g, b);
        for (int tid = 0; tid < RGB_CHUNK_THREADS; tid++) {
            const int first = rgb_own_first(b, tid);
            const int rounds = rgb_own_rounds(n, g, first);
            if (rounds < 0 || rounds > block_rounds) FAIL("rounds: n %d G %d block %d thread %d: %d, the block's %d", n, g, b, tid, rounds, block_rounds);
            for (int k = 0; k < rounds; k++) hit[(size_t)rgb_own_record(g, first, k)]++;
            total += rounds;
        }
    }
    if (total != n) FAIL("n %d G %d: %lld records stepped", n, g, total);
    for (int i = 0; i < n; i++)
        if (hit[(size_t)i] != 1) { FAIL("n %d G %d: record %d stepped %d times", n, g, i, (int)hit[(size_t)i]); break; }
    cases++;
}

static void shares(int g)
{
    const int stride = g * RGB_CHUNK_THREADS, n_max = 3 * stride + 3;
    std::vector<int> rounds((size_t)stride, 0);   // per thread of the launch, at the n before
    for (int t = 0; t < stride; t++)
        if (rgb_own_rounds(0, g, t) != 0) FAIL("G %d: thread %d has a record of an empty list", g, t);
    for (int n = 0; n <= n_max; n++) {
        if (n > 0) {
            const int i = n - 1, owner = i % stride, k = i / stride;
            const int r = rgb_own_rounds(n, g, owner);
            if (r != rounds[(size_t)owner] + 1 || r != k + 1) FAIL("G %d n %d: the owner %d of record %d has %d rounds, had %d", g, n, owner, i, r, rounds[(size_t)owner]);
            else if (rgb_own_record(g, owner, r - 1) != i) FAIL("G %d n %d: the owner's last record is %d", g, n, rgb_own_record(g, owner, r - 1));
            rounds[(size_t)owner] = r;
            const int others[] = {owner - 1, owner + 1, 0, stride - 1, owner - RGB_CHUNK_THREADS, owner + RGB_CHUNK_THREADS};
            for (int t : others)
                if (t >= 0 && t < stride && t != owner && rgb_own_rounds(n, g, t) != rounds[(size_t)t]) FAIL("G %d n %d: thread %d moved to %d rounds", g, n, t, rgb_own_rounds(n, g, t));
            if (rgb_own_block_rounds(n, g, owner / RGB_CHUNK_THREADS) != rounds[(size_t)(owner / RGB_CHUNK_THREADS) * RGB_CHUNK_THREADS]) FAIL("G %d n %d: block rounds", g, n);
        }
        cases++;
        const int in_round = n % stride, in_block = n % RGB_CHUNK_THREADS;
        const bool edge = g <= 3 || n == n_max || ((in_round <= RGB_CHUNK_THREADS + 1 || in_round >= stride - RGB_CHUNK_THREADS - 1) && (in_block <= 1 || in_block == RGB_CHUNK_THREADS - 1));
        if (edge) full_walk(n, g, (size_t)n);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the take-over protocol
enum Pc { ARRIVE, POLL, OR_ORPHAN, RELOAD, OR_TAKEN, LAST_LOAD, LAST_TAKE, DONE };
struct Model {
    int g;
    bool polls;        // false: rgb_fuse_poll = 0, the wait has run out before the first poll
    bool reload;       // false: the broken protocol -- a block leaves behind its OR into the orphan mask without looking at the arrival word again
    unsigned arrivals = 0, orphan = 0, taken = 0;
    int pc[3] = {ARRIVE, ARRIVE, ARRIVE};
    unsigned seen[3] = {0, 0, 0};   // the last arriver's copy of the orphan mask
    int stepped[3] = {0, 0, 0}, left = 0, adopted = 0;
};
static long long ends = 0, violations = 0;

static void at_end(const Model& m)
{
    ends++;
    bool ok = m.left == m.adopted;
    for (int b = 0; b < m.g; b++) ok = ok && m.stepped[b] == 1;
    if (!ok) violations++;
}
static void explore(const Model& m)
{
    bool any = false;
    for (int b = 0; b < m.g; b++) {
        if (m.pc[b] == DONE) continue;
        any = true;
        const unsigned bit = 1u << b;
        Model s = m;
        switch (m.pc[b]) {
        case ARRIVE:      // the returning add: the block that draws the last arrival never waits
            s.pc[b] = ++s.arrivals == (unsigned)m.g ? LAST_LOAD : (m.polls ? POLL : OR_ORPHAN);
            explore(s);
            break;
        case POLL:        // a poll that sees everybody goes on; the wait may also run out at any poll, whatever the word shows by then
            if (m.arrivals == (unsigned)m.g) { Model q = m; q.stepped[b]++; q.pc[b] = DONE; explore(q); }
            s.pc[b] = OR_ORPHAN;
            explore(s);
            break;
        case OR_ORPHAN:
            s.orphan |= bit;
            s.pc[b] = RELOAD;
            if (!m.reload) { s.left++; s.pc[b] = DONE; }
            explore(s);
            break;
        case RELOAD:      // issued after the OR's result returned
            if (m.arrivals < (unsigned)m.g) { s.left++; s.pc[b] = DONE; }   // incomplete behind its own OR: the last arriver's load of the mask comes later
            else s.pc[b] = OR_TAKEN;
            explore(s);
            break;
        case OR_TAKEN:
            if (m.taken & bit) s.left++;   // the last arriver has the share
            else s.stepped[b]++;           // goes on as a block that met
            s.taken |= bit;
            s.pc[b] = DONE;
            explore(s);
            break;
        case LAST_LOAD:   // issued after the arrival add's result returned; the block then steps its own share
            s.seen[b] = m.orphan;
            s.stepped[b]++;
            s.pc[b] = LAST_TAKE;
            explore(s);
            break;
        case LAST_TAKE: { // one OR of all the orphan bits it saw: the shares whose bits it was first to set are its own now
            const unsigned mine = m.seen[b] & ~m.taken;
            s.taken |= m.seen[b];
            for (int o = 0; o < m.g; o++)
                if (mine & (1u << o)) { s.stepped[o]++; s.adopted++; }
            s.pc[b] = DONE;
            explore(s);
            break;
        }
        default: break;
        }
    }
    if (!any) at_end(m);
}
static void protocol()
{
    for (int g = 2; g <= 3; g++)
        for (int polls = 0; polls < 2; polls++) {
            Model m; m.g = g; m.polls = polls != 0; m.reload = true;
            ends = violations = 0;
            explore(m);
            std::printf("protocol: G %d, %s: %lld interleavings, %lld with a share lost, stepped twice or miscounted\n", g, polls ? "bounded wait" : "nobody waits", ends, violations);
            if (violations || ends == 0) FAIL("take-over protocol, G %d polls %d", g, polls);
            cases++;
            m.reload = false;
            ends = violations = 0;
            explore(m);
            if (violations == 0) FAIL("the model does not see the share a block loses when it leaves without the re-load (G %d polls %d)", g, polls);
            cases++;
        }
}

int main()
{
    for (int g : {1, 2, 3, 32, 33, 64, 1024}) shares(g);
    // counts above the capacity: clamped as in the kernel, walked over an array as long as the capacity
    const int caps[] = {40 * 30, 80 * 60, 160 * 120, 320 * 240, 640 * 480, 1, 255, 256, 257};
    for (int cap : caps)
        for (unsigned int cand_n : {(unsigned int)cap, (unsigned int)cap + 1u, 2u * (unsigned int)cap + 7u, 0x7FFFFFFFu, 0x80000000u, UINT_MAX})
            for (int g : {1, 2, 32, 33, 64}) {
                const int n = rgb_chunk_n(cand_n, cap);
                if (n != cap) FAIL("clamp: cand_n %u capacity %d -> %d", cand_n, cap, n);
                full_walk(n, g, (size_t)cap);
            }
    if (rgb_chunk_n(UINT_MAX, 0) != 0 || rgb_own_rounds(0, 32, 0) != 0 || rgb_own_rounds(5, 0, 0) != 0) FAIL("empty list / no blocks");
    cases++;
    protocol();
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
