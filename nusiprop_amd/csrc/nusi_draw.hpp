// nuSIprop MI355X -- the counter-based generator of the detector layer's pseudo-experiments (include/nusi.h, "Drawing
// counts"): Philox4x32-10, two uniforms per 128-bit block, and Poisson counts by inversion below mu = 10 and Hoermann's
// PTRS from there (numpy's split and its random_loggam).  Every operation is rounded on its own (no contraction), exp
// and log are nm::exp_i and nm::log_i, so detector.draw_host gives the same bits with the same exp and log.  A draw is
// identified by (seed, stream, row, p, c) alone: it does not depend on the launch, a chunk or a slice.
// normal0 (include/nusi.h, "Drawing normals") is a truncated normal variate on the same blocks' generator, in a counter
// domain of its own; detector.draw_normal_host gives the same bits with the same log.
#pragma once

#include "nusi_libm.hpp"

namespace nusi {
namespace draw {

constexpr unsigned kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
constexpr int kInversionMax = 255, kPtrsRounds = 64;

struct Block {
    unsigned x[4];
};

// ten rounds of  c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),  the key bumped after each
NUSI_FN Block philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)kM0 * c0, p1 = (unsigned long long)kM1 * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += kW0;
        k1 += kW1;
    }
    return Block{{c0, c1, c2, c3}};
}

// 53 bits of two words as a double in [0, 1): exact
NUSI_FN double uniform(unsigned hi, unsigned lo)
{
    return (double)(((unsigned long long)(hi >> 5) << 26) + (unsigned long long)(lo >> 6)) * 0x1p-53;
}

// the draw's identity: the key is the seed, the counter (block, p 64 + c, row, stream)
struct Ident {
    unsigned k0, k1, pc, row, stream;
};
NUSI_FN Ident ident(unsigned long long seed, unsigned stream, unsigned row, unsigned p, unsigned c)
{
    return Ident{(unsigned)seed, (unsigned)(seed >> 32), p * 64u + c, row, stream};
}
NUSI_FN void uniforms(const Ident& id, unsigned block, double& u0, double& u1)
{
    const Block b = philox4x32(block, id.pc, id.row, id.stream, id.k0, id.k1);
    u0 = uniform(b.x[0], b.x[1]);
    u1 = uniform(b.x[2], b.x[3]);
}

// numpy's random_loggam: log Gamma(x), x > 0, by the shift to x0 = x + n >= 7, ten terms of Stirling's series in
// 1 / x0^2 (Horner), and the shift undone by subtracting logs; exactly 0 at 1 and 2
NUSI_FN double loggam(double x)
{
#pragma clang fp contract(off)
    constexpr double a[10] = {8.333333333333333e-02, -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04,
                              8.417508417508418e-04, -1.917526917526918e-03, 6.410256410256410e-03, -2.955065359477124e-02,
                              1.796443723688307e-01, -1.39243221690590e+00};
    constexpr double hl2pi = 0.5 * 1.8378770664093453e+00;
    if (x == 1.0 || x == 2.0) return 0.0;
    const int n = x < 7.0 ? (int)(7.0 - x) : 0;
    double x0 = x + (double)n;
    const double ix = 1.0 / x0;
    const double x2 = ix * ix;
    double gl0 = a[9];
#pragma unroll
    for (int k = 8; k >= 0; --k) {
        gl0 = gl0 * x2;
        gl0 = gl0 + a[k];
    }
    double gl = gl0 / x0;
    gl = gl + hl2pi;
    const double t = (x0 - 0.5) * nm::log_i(x0);
    gl = gl + t;
    gl = gl - x0;
    for (int k = 1; k <= n; ++k) {
        x0 = x0 - 1.0;
        gl = gl - nm::log_i(x0);
    }
    return gl;
}

// one Poisson(mu) count as a double.  mu == 0: 0, no bits drawn.  NaN for a mu that is negative, NaN or infinite
// (the host forms refuse those).
NUSI_FN double poisson(double mu, const Ident& id)
{
#pragma clang fp contract(off)
    if (mu == 0.0) return 0.0;
    if (!(mu > 0.0) || mu == 1.0 / 0.0) return (mu - mu) / (mu - mu);
    double u0, u1;
    if (mu < 10.0) {
        uniforms(id, 0u, u0, u1);
        double p = nm::exp_i(-mu), F = p, k = 0.0;
        while (!(u0 < F)) {
            k = k + 1.0;
            p = (p * mu) / k;
            const double Fn = F + p;
            if ((Fn == F && k > mu) || k == (double)kInversionMax) break;
            F = Fn;
        }
        return k;
    }
    const double slam = __builtin_sqrt(mu), loglam = nm::log_i(mu);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
    const double vr = 0.9277 - 3.6224 / (b - 2.0);
    const double lia = nm::log_i(invalpha);
    double k = 0.0;
    for (int r = 0; r < kPtrsRounds; ++r) {
        uniforms(id, (unsigned)r, u0, u1);
        const double U = u0 - 0.5, V = u1;
        const double us = 0.5 - __builtin_fabs(U);
        if (us == 0.0) continue;
        double x = (2.0 * a) / us;
        x = x + b;
        x = x * U;
        x = x + mu;
        x = x + 0.43;
        k = __builtin_floor(x);
        if (us >= 0.07 && V <= vr) return k;
        if (k < 0.0 || (us < 0.013 && V > us)) continue;
        double lhs = nm::log_i(V) + lia;
        double y = a / (us * us);
        y = y + b;
        lhs = lhs - nm::log_i(y);
        double rhs = -mu + k * loglam;
        rhs = rhs - loggam(k + 1.0);
        if (lhs <= rhs) return k;
    }
    return k > 0.0 ? k : 0.0;
}

// one normal variate around center >= 0 of width sigma, truncated to x >= 0 (include/nusi.h, "Drawing normals"):
// Marsaglia's polar method, round r on block kNormalBlock0 + r -- the counts use blocks 0 .. 63, so under one identity
// the two families share no block.  sigma == +inf (no prior): center, no bits drawn.  After kNormalRounds rejected
// rounds: center.  used: nullptr, or receives the blocks consumed.
constexpr unsigned kNormalBlock0 = 0x80000000u;
constexpr int kNormalRounds = 64;

NUSI_FN double normal0(double center, double sigma, const Ident& id, int* used = nullptr)
{
#pragma clang fp contract(off)
    if (used) *used = 0;
    if (sigma == 1.0 / 0.0) return center;
    for (int r = 0; r < kNormalRounds; ++r) {
        double u0, u1;
        uniforms(id, kNormalBlock0 + (unsigned)r, u0, u1);
        if (used) *used = r + 1;
        const double u = 2.0 * u0 - 1.0, v = 2.0 * u1 - 1.0;   // (exact)
        const double uu = u * u, vv = v * v;
        const double s = uu + vv;
        if (!(s < 1.0) || s == 0.0) continue;
        const double l2 = -2.0 * nm::log_i(s);
        const double q = l2 / s;
        const double f = __builtin_sqrt(q);
        const double z = u * f;
        const double sz = sigma * z;
        const double x = center + sz;
        if (!(x >= 0.0)) continue;
        return x;
    }
    return center;
}

}   // namespace draw
}   // namespace nusi
