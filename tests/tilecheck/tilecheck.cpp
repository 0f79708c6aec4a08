// TEST INFRASTRUCTURE ONLY -- host check of the alpha table's tile list (nusiprop_amd/csrc/nusi_alpha_tiles.hpp):
// the partition of the entries n < m < T over (tile, thread slot), the edge counts of the tile sides, the entry
// lists of the partly filled tiles.  Plain C++ (g++), also built with -fsanitize=address,undefined
// (tests/test_alpha_tile_partition.py).  Prints one line per grid and "OK", or the first failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nusi_alpha_tiles.hpp"

using namespace nusi;

static int fails = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (fails++ < 20) {                         \
                std::printf("FAIL %s: ", #c);           \
                std::printf(__VA_ARGS__);               \
                std::printf("\n");                      \
            }                                           \
        }                                               \
    } while (0)

// distinct bin edges of bins [b0, b0 + cnt), as alpha_edge_list counts them on the device
static int side_edges(const std::vector<unsigned char>& shared, int b0, int cnt)
{
    int e = 0;
    for (int j = b0; j < b0 + cnt; ++j) e += (j > b0 && shared[j - 1]) ? 1 : 2;
    return e;
}

// (min_offdiag: over the tiles whose n bins all lie below their m bins; core / mrun / ext: both sides in the first N
// bins / n side there, m side extended / the n side reaches into the extended bins)
struct Census { int tiles = 0, npair = 0, min_entries = 1 << 30, min_offdiag = 1 << 30, core = 0, mrun = 0, ext = 0, other = 0; };

// N energy bins share their edges; the T - N redshift-extended bins above them do not
static Census check_grid(int N, int T)
{
    std::vector<unsigned char> shared(T, 0);
    for (int n = 0; n + 1 < N; ++n) shared[n] = 1;
    const AlphaTileList tl = alpha_tiles_build(T, shared.data());
    std::vector<unsigned char> own((size_t)T * T, 0);
    Census cs;
    const int cap[3][2] = {{kAlphaTile + 1, kAlphaTile + 1}, {kAlphaTile + 1, 2 * kAlphaTile}, {2 * kAlphaTile, 2 * kAlphaTile}};
    for (int c = 0; c < 3; ++c) {
        CHECK((int)tl.cls[c].size() % kTileWords == 0, "N %d T %d class %d", N, T, c);
        for (int i = 0; i < tl.count(c); ++i) {
            const int* w = tl.cls[c].data() + kTileWords * i;
            const AlphaTile t = alpha_tile_decode(w);
            int w2[kTileWords];
            alpha_tile_encode(t, w2);
            CHECK(w2[0] == w[0] && w2[1] == w[1], "N %d T %d class %d tile %d: words", N, T, c, i);
            CHECK(t.n0 >= 0 && t.m0 >= 0 && t.ncnt >= 1 && t.mcnt >= 1 && t.ncnt <= kAlphaTile && t.mcnt <= kAlphaTile &&
                      t.n0 + t.ncnt <= T && t.m0 + t.mcnt <= T,
                  "N %d T %d class %d tile %d: n %d+%d m %d+%d", N, T, c, i, t.n0, t.ncnt, t.m0, t.mcnt);
            if (fails) return cs;
            const int et = side_edges(shared, t.n0, t.ncnt), es = side_edges(shared, t.m0, t.mcnt);
            // the batched class: at most 17 distinct edges per side; every class: its launch's LDS capacity (class 0:
            // kAlphaTile + 1; the per-table classes 1 and 2 of a grid whose core / extended boundary lies inside a
            // tile: 2 kAlphaTile)
            CHECK(c > 0 || (et <= 17 && es <= 17), "N %d T %d tile %d: %d / %d edges", N, T, i, et, es);
            CHECK(et <= cap[c][0] && es <= cap[c][1], "N %d T %d class %d tile %d: %d / %d edges", N, T, c, i, et, es);
            // ownership by thread slot, and the entry list
            const int ne = alpha_tile_entries(t, T);
            int seen = 0, last = -1;
            std::vector<int> list(kTileThreads, -1);
            for (int tid = 0; tid < kTileThreads; ++tid) {
                const int r = alpha_tile_entry_rank(t, T, tid);
                CHECK((r >= 0) == alpha_tile_slot_valid(t, T, tid), "rank / valid, tile %d slot %d", i, tid);
                if (r < 0) continue;
                const int n = t.n0 + tid % kAlphaTile, m = t.m0 + tid / kAlphaTile;
                CHECK(n < m && m < T, "N %d T %d tile %d slot %d: entry (%d, %d)", N, T, i, tid, n, m);
                if (!(n < m && m < T)) return cs;
                ++own[(size_t)n * T + m];
                CHECK(r < ne, "N %d T %d tile %d slot %d: rank %d of %d", N, T, i, tid, r, ne);
                CHECK(r == last + 1, "N %d T %d tile %d slot %d: rank %d after %d (thread order)", N, T, i, tid, r, last);
                if (r >= 0 && r < kTileThreads) list[r] = tid;
                last = r;
                ++seen;
            }
            CHECK(seen == ne, "N %d T %d tile %d: %d slots, %d entries", N, T, i, seen, ne);
            for (int r = 0; r < ne; ++r) CHECK(list[r] >= 0 && list[r] < kAlphaTile * kAlphaTile, "list[%d] = %d", r, list[r]);
            if (c == 0) {
                const bool pair = i >= tl.count(0) - tl.npair;
                CHECK(pair == (ne <= kPairEntries), "N %d T %d tile %d: %d entries, paired %d", N, T, i, ne, (int)pair);
                if (pair) {
                    // the kernel's two halves: thread tid combines entry list[tid % kPairEntries] of point tid / kPairEntries
                    for (int tid = 0; tid < kTileThreads; ++tid) {
                        const int e = tid % kPairEntries;
                        if (e < ne) CHECK(list[e] >= 0 && list[e] <= 255 && alpha_tile_slot_valid(t, T, list[e]), "half slot %d", tid);
                    }
                    ++cs.npair;
                }
                ++cs.tiles;
                if (ne < cs.min_entries) cs.min_entries = ne;
                if (t.n0 + t.ncnt <= t.m0 && ne < cs.min_offdiag) cs.min_offdiag = ne;
                if (t.m0 + t.mcnt <= N) ++cs.core;
                else if (t.n0 + t.ncnt <= N && t.m0 >= N) ++cs.mrun;
                else if (t.n0 + t.ncnt > N && t.m0 >= N) ++cs.ext;
                else ++cs.other;
            }
        }
    }
    CHECK(cs.npair == tl.npair, "N %d T %d: npair %d / %d", N, T, cs.npair, tl.npair);
    long long bad = 0;
    for (int n = 0; n < T; ++n)
        for (int m = 0; m < T; ++m) bad += own[(size_t)n * T + m] != (n < m ? 1 : 0);
    CHECK(bad == 0, "N %d T %d: %lld entries not owned exactly once", N, T, bad);
    std::printf("N %d T %d: class 0 %d tiles (%d paired; %d core, %d core x extended, %d extended, %d other; min %d entries, off the diagonal %d), "
                "class 1 %d, class 2 %d\n", N, T, cs.tiles, cs.npair, cs.core, cs.mrun, cs.ext, cs.other, cs.min_entries, cs.min_offdiag,
                tl.count(1), tl.count(2));
    return cs;
}

int main()
{
    const int shapes[][2] = {{300, 346}, {45, 91}, {40, 78}, {31, 79}, {60, 106}, {1200, 1333}};
    for (const auto& s : shapes) {
        const Census c = check_grid(s[0], s[1]);
        if (s[0] == 300) {
            CHECK(c.min_entries >= 30, "C4: a workgroup of %d entries", c.min_entries);
            CHECK(c.core == 210 && c.mrun == 120 && c.ext == 21 && c.other == 0 && c.tiles == 351,
                  "C4: %d core + %d + %d (+ %d) = %d workgroups", c.core, c.mrun, c.ext, c.other, c.tiles);
        }
    }
    for (int d = 0; d <= 60; ++d) check_grid(45, 45 + d);
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("OK\n");
    return 0;
}
