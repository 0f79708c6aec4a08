// TEST INFRASTRUCTURE ONLY: host build of nusi_draw.hpp -- the functions k_poisson_draw calls, compiled for the CPU -- for
// tests/test_draw.py, which compares them with detector.draw_host under the oracle's exp and log.  Never linked into
// libnusi.so.
#include "nusi_draw.hpp"

extern "C" {

void hc_philox(const unsigned* ctr, const unsigned* key, unsigned* out)
{
    const nusi::draw::Block b = nusi::draw::philox4x32(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) out[i] = b.x[i];
}

double hc_loggam(double x) { return nusi::draw::loggam(x); }

// out[row][p][c] as nusi_plan_draw_counts defines it
void hc_draw(const double* mu, int rows, int C, int P, unsigned long long seed, unsigned stream, double* out)
{
    for (int row = 0; row < rows; ++row)
        for (int p = 0; p < P; ++p)
            for (int c = 0; c < C; ++c)
                out[((size_t)row * P + p) * C + c] =
                    nusi::draw::poisson(mu[(size_t)row * C + c], nusi::draw::ident(seed, stream, (unsigned)row, (unsigned)p, (unsigned)c));
}
}
