// TEST INFRASTRUCTURE ONLY: host build of nusi_libm.hpp's atan2 forms (atan2_i and atan2_w with the first-range vote,
// which on the host is each call's own predicate; atan2_full, fdlibm's branches; atan2_slow, atan2 without the
// first-range vote), for tests/test_atan2_range_vote.py, and of the alpha tile list, for
// tests/test_atan2_vote_tables_gpu.py.  Never linked into libnusi.so.
#include "nusi_alpha_tiles.hpp"
#include "nusi_libm.hpp"

extern "C" {

// the three forms on n operand pairs; pi, pw: the path atan2_i and atan2_w took -- 0 the first-range body, 1 the
// select path, 2 fdlibm's branches --, set inside the code that ran by the flagged instances atan2_vote_t<.., true>,
// plus 8 where the flagged call's bits differ from the plain call's (pw: meaningful inside atan2_w's bounds only)
void hc_atan2_n(int n, const double* y, const double* x, double* ai, double* aw, double* af, int* pi, int* pw)
{
    using namespace nusi;
    for (int i = 0; i < n; ++i) {
        ai[i] = nm::atan2_i(y[i], x[i]);
        aw[i] = nm::atan2_w(y[i], x[i]);
        af[i] = nm::atan2_full(y[i], x[i]);
        int qi = -1, qw = -1;
        const double fi = nm::atan2_vote_t<false, true>(y[i], x[i], &qi), fw = nm::atan2_vote_t<true, true>(y[i], x[i], &qw);
        pi[i] = qi + (nm::bits(fi) != nm::bits(ai[i]) ? 8 : 0);
        pw[i] = qw + (nm::bits(fw) != nm::bits(aw[i]) ? 8 : 0);
    }
}
// atan2 without the first-range vote: what a wave that fails it calls (the select path, or fdlibm's branches)
void hc_atan2_slow_n(int n, const double* y, const double* x, double* a)
{
    for (int i = 0; i < n; ++i) a[i] = nusi::nm::atan2_slow<false>(y[i], x[i]);
}

// the class-0 tiles of a grid of T bins (alpha_tiles_build; the tiles k_alpha_batch runs), four ints each: n0, ncnt,
// m0, mcnt; returns their number (at most cap are written).  For tests/test_atan2_vote_tables_gpu.py's wave layout
int hc_alpha_tiles0(int T, const unsigned char* shared, int* out, int cap)
{
    const nusi::AlphaTileList tl = nusi::alpha_tiles_build(T, shared);
    const int n = tl.count(0);
    for (int i = 0; i < n && i < cap; ++i) {
        const nusi::AlphaTile t = nusi::alpha_tile_decode(tl.cls[0].data() + nusi::kTileWords * i);
        out[4 * i] = t.n0; out[4 * i + 1] = t.ncnt; out[4 * i + 2] = t.m0; out[4 * i + 3] = t.mcnt;
    }
    return n;
}

}  // extern "C"
