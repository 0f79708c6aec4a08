// nuSIprop MI355X -- the alpha table's tile list: descriptors, their decoding, the entry list of a partly filled
// tile, and the host classification of a grid's tiles (alpha_tiles_build).  Plain C++ without HIP calls: the kernels
// include it, and so does the host program of tests/tilecheck.
#pragma once

#include <vector>

#ifndef NUSI_FN
#if defined(__HIPCC__)
#define NUSI_FN __host__ __device__ inline
#else
#define NUSI_FN inline
#endif
#endif

namespace nusi {

constexpr int kAlphaTile = 15;   // bins per alpha tile side (the edges of a core tile side are kAlphaTile + 1 <= 17)
constexpr int kTileThreads = 256;
static_assert(kAlphaTile * kAlphaTile <= kTileThreads, "one entry per work-item");
// a tile of at most kPairEntries entries n < m fits one half of a workgroup: the reference-order batch kernel runs
// two points of the batch per iteration of its point loop over it (AlphaTile::pair, k_alpha_batch)
constexpr int kPairEntries = kTileThreads / 2;

// A tile: bins [n0, n0 + ncnt) x [m0, m0 + mcnt) of the table, ncnt, mcnt <= kAlphaTile, all inside the table.  Two
// words per tile in the list: n0 | ncnt << 24, m0 | mcnt << 24 | pair << 28.  (Explicit starts and counts: the redshift-extended
// bins are cut into runs of 8 from the first extended bin, which is no multiple of a fixed half tile.)
constexpr int kTileWords = 2;
struct AlphaTile { int n0, ncnt, m0, mcnt; bool pair = false; };
NUSI_FN void alpha_tile_encode(const AlphaTile& t, int* w)
{
    w[0] = t.n0 | (t.ncnt << 24);
    w[1] = t.m0 | (t.mcnt << 24) | ((int)t.pair << 28);
}
NUSI_FN AlphaTile alpha_tile_decode(const int* w)
{
    return AlphaTile{w[0] & 0xffffff, (w[0] >> 24) & 0xf, w[1] & 0xffffff, (w[1] >> 24) & 0xf, ((w[1] >> 28) & 1) != 0};
}
// thread slot tid of a workgroup holds entry (n0 + tid % kAlphaTile, m0 + tid / kAlphaTile) of its tile
NUSI_FN bool alpha_tile_slot_valid(const AlphaTile& t, int T, int tid)
{
    const int ln = tid % kAlphaTile, lm = tid / kAlphaTile, n = t.n0 + ln, m = t.m0 + lm;
    return tid < kAlphaTile * kAlphaTile && ln < t.ncnt && lm < t.mcnt && n < m && m < T;
}
// entries n < m of the tile's row lm (m = m0 + lm): its n bins are n0 .. n0 + count - 1
NUSI_FN int alpha_tile_row_entries(const AlphaTile& t, int T, int lm)
{
    const int m = t.m0 + lm;
    if (lm >= t.mcnt || m >= T) return 0;
    const int c = m - t.n0;   // n < m
    return c < 0 ? 0 : c < t.ncnt ? c : t.ncnt;
}
NUSI_FN int alpha_tile_entries(const AlphaTile& t, int T)
{
    int c = 0;
    for (int lm = 0; lm < kAlphaTile; ++lm) c += alpha_tile_row_entries(t, T, lm);
    return c;
}
// The compact entry list of a tile, in thread-slot order: the index of slot tid's entry in it, or -1 for a slot
// without an entry.  list[alpha_tile_entry_rank(t, T, tid)] = tid over the valid slots fills list[0 .. entries).
NUSI_FN int alpha_tile_entry_rank(const AlphaTile& t, int T, int tid)
{
    if (!alpha_tile_slot_valid(t, T, tid)) return -1;
    const int ln = tid % kAlphaTile, lm = tid / kAlphaTile;
    int r = ln;   // (the row's entries are its first slots: n0 <= n < min(n0 + ncnt, m))
    for (int j = 0; j < lm; ++j) r += alpha_tile_row_entries(t, T, j);
    return r;
}

// The tiles of a grid of T bins; shared[n] = (hi[n] == lo[n + 1]) bitwise.  Three launch classes by the distinct
// bin edges of a tile's sides (bins of the first N share edges, the redshift-extended bins do not), which set the
// LDS footprint: class 0 both sides <= kAlphaTile + 1 edges, 1: t side <= kAlphaTile + 1, S' side <= 2 kAlphaTile,
// 2: both <= 2 kAlphaTile.  cls[c]: kTileWords words per tile.  Class 0 lists its tiles of more than kPairEntries
// entries first, then the npair others, flagged pair (the longer workgroups start first).
struct AlphaTileList {
    std::vector<int> cls[3];
    int npair = 0;
    int count(int c) const { return (int)cls[c].size() / kTileWords; }
};
inline AlphaTileList alpha_tiles_build(int T, const unsigned char* shared)
{
    const int nt = (T + kAlphaTile - 1) / kAlphaTile;
    // distinct edges of each tile side, exactly as alpha_edge_list counts them on the device
    std::vector<int> ne(nt, 0);
    for (int t = 0; t < nt; ++t)
        for (int j = t * kAlphaTile; j < (t + 1) * kAlphaTile && j < T; ++j)
            ne[t] += (j > t * kAlphaTile && shared[j - 1]) ? 1 : 2;
    // From the first tile t0 whose bins do not share edges (the redshift-extended bins) on, tiles of class 2
    // save no corner (4 per entry, like the per-entry path) and their 80-KB LDS footprint halves the
    // occupancy.
    const int cap_core = kAlphaTile + 1;
    int t0 = nt;
    for (int t = 0; t < nt; ++t)
        if (ne[t] > cap_core) { t0 = t; break; }
    bool tail_ext = true;   // no bin from tile t0 on shares an edge with its neighbour
    for (int n = t0 * kAlphaTile; n + 1 < T; ++n) tail_ext = tail_ext && !shared[n];
    AlphaTileList out;
    std::vector<AlphaTile> c0;
    auto put = [&](std::vector<int>& v, const AlphaTile& t) {
        int w[kTileWords];
        alpha_tile_encode(t, w);
        v.insert(v.end(), w, w + kTileWords);
    };
    auto span = [&](int b0, int cnt) { return b0 + cnt < T ? cnt : T - b0; };
    if (tail_ext && t0 < nt) {
        // A purely unshared tail: on the m side its bins from x0 = t0 kAlphaTile on are cut into runs of 8 (16 edges,
        // the core tiles' LDS footprint; the remainder is the last run), each a row of tiles of class 0, batched with
        // the core tiles.  (Cut at the halves of the fixed tiles instead -- 8, 7, 8, 7, ... -- C4's 46 extended bins
        // ended in a row of a single bin.)  The n side of a row [s, s + c): the core tiles up to bin xl = x0 - 1, then
        // the bins [xl, s + c - 1) in runs of 8 counted down from the top, so that the tile on the diagonal is
        // n in [s - 1, s + 7) against m in [s, s + 8): 36 entries -- a run against itself has 28, the last run of 6
        // bins 15 -- and the lowest run, the remainder, starts at the last core bin xl (in every row, so the core
        // tiles of these rows end there); no more tiles than with the n side cut like the m side.
        for (int tm = 0; tm < t0; ++tm)
            for (int tn = 0; tn <= tm; ++tn) c0.push_back(AlphaTile{tn * kAlphaTile, kAlphaTile, tm * kAlphaTile, kAlphaTile});
        const int x0 = t0 * kAlphaTile, xl = x0 > 0 ? x0 - 1 : 0;
        for (int rm = x0; rm < T; rm += 8) {
            const int mc = span(rm, 8);
            for (int n0 = 0; n0 < xl; n0 += kAlphaTile)
                c0.push_back(AlphaTile{n0, n0 + kAlphaTile < xl ? kAlphaTile : xl - n0, rm, mc});
            std::vector<AlphaTile> row;
            for (int e = rm + mc - 1; e > xl; e -= 8) {   // n bins [max(xl, e - 8), e)
                const int n0 = e - 8 > xl ? e - 8 : xl;
                row.push_back(AlphaTile{n0, e - n0, rm, mc});
            }
            c0.insert(c0.end(), row.rbegin(), row.rend());
        }
    } else {
        // Class-1 tiles (t side core, S' side extended: 30 S' edges) are split into their first 8 and last
        // 7 m bins (16 / 14 S' edges): the halves fit the core tiles' LDS footprint and join class 0,
        // whose launch builds batches of tables.  So cls[1] stays empty: c == 1 needs ne[tn] <= cap_core < ne[tm],
        // hence tn < tm, and every such tile is split.  The launchers keep their three-class loop.
        for (int tm = 0; tm < nt; ++tm)
            for (int tn = 0; tn <= tm; ++tn) {
                const int c = (ne[tn] <= cap_core && ne[tm] <= cap_core) ? 0 : (ne[tn] <= cap_core) ? 1 : 2;
                const int n0 = tn * kAlphaTile, m0 = tm * kAlphaTile;
                const AlphaTile t{n0, span(n0, kAlphaTile), m0, span(m0, kAlphaTile)};
                if (c == 1) {
                    c0.push_back(AlphaTile{n0, t.ncnt, m0, span(m0, 8)});
                    if (m0 + 8 < T) c0.push_back(AlphaTile{n0, t.ncnt, m0 + 8, span(m0 + 8, kAlphaTile - 8)});
                } else if (c == 0) {
                    c0.push_back(t);
                } else {
                    put(out.cls[c], t);
                }
            }
    }
    for (int pass = 0; pass < 2; ++pass)
        for (AlphaTile t : c0) {
            const bool pair = t.pair = alpha_tile_entries(t, T) <= kPairEntries;
            if (pair == (pass == 1)) put(out.cls[0], t);
            if (pair && pass == 1) ++out.npair;
        }
    return out;
}

}  // namespace nusi
