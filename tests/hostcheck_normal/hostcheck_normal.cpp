// TEST INFRASTRUCTURE ONLY: host build of nusi_draw.hpp's normal0 -- the function k_normal_draw, k_nuis_inject and
// k_nuis_belt call, compiled for the CPU -- for tests/test_draw_normal.py, which compares it with
// detector.draw_normal_host under the oracle's log.  Never linked into libnusi.so.
#include "nusi_draw.hpp"

extern "C" {

int hc_normal_rounds(void) { return nusi::draw::kNormalRounds; }
unsigned hc_normal_block0(void) { return nusi::draw::kNormalBlock0; }

// out[row][p][j] as nusi_plan_draw_normals defines it; used[row][p][j] (or NULL): the blocks each draw consumed
void hc_normal(const double* center, const double* sigma, int rows, int J, int P, unsigned long long seed, unsigned stream,
               double* out, int* used)
{
    for (int row = 0; row < rows; ++row)
        for (int p = 0; p < P; ++p)
            for (int j = 0; j < J; ++j) {
                const size_t i = ((size_t)row * P + p) * J + j;
                out[i] = nusi::draw::normal0(center[(size_t)row * J + j], sigma[j],
                                             nusi::draw::ident(seed, stream, (unsigned)row, (unsigned)p, (unsigned)j),
                                             used ? used + i : nullptr);
            }
}
}
