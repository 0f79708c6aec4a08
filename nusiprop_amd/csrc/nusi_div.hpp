// nuSIprop MI355X -- fp64 division with one refined reciprocal per divisor.
//
// The compiler expands an fp64 a / b into 11 VALU instructions: two v_div_scale_f64 (divisor, numerator), v_rcp_f64,
// two Newton steps on the reciprocal (four fma), q = a y, r = fma(-b, q, a), v_div_fmas_f64 (fma(r, y, q), rescaled
// when v_div_scale flagged it) and v_div_fixup_f64 (zeros, infinities, NaN, subnormal quotients).  Two quotients over
// one divisor refine the same reciprocal twice, and the scale / fixup instructions do nothing when no operand is near
// the ends of the exponent range.  Here the reciprocal is refined once per divisor (5 instructions) and each
// numerator takes q = a y, r = fma(-b, q, a), fma(r, y, q) (3): the compiler's own sequence on the same start value
// (__builtin_amdgcn_rcp is v_rcp_f64), minus the instructions that pass their operand through -- the same bits, RN(a /
// b).  tests/test_div_shared_gpu.py compares it with the device's / and numpy's bit for bit.
//
// When v_div_scale_f64 (S0, divisor S1, numerator S2) scales nothing and sets no VCC: S1, S2 finite and nonzero;
// exponent(S2) - exponent(S1) < 768; S1 normal; 1 / S1 normal (|S1| <= 2^1022); S2 / S1 normal (exponent(S2) -
// exponent(S1) > -1022); |S2| >= 2^-969.  Then v_div_fmas is the plain fma and v_div_fixup returns it.  Every operand
// in [2^-380, 2^380) (div_in_window) gives all of that: exponent differences within +-759, quotients in (2^-760,
// 2^760), and the residual r either 0 or at least an ulp of a 2^-53-th of |a|, normal.  A zero numerator is outside
// the window on purpose: for a = -0 over b > 0 the short sequence returns +0 (r = +0, and +0 y + -0 rounds to +0).  A
// numerator +0 over b > 0 does come out +0 (q = +0, r = fma(-b, +0, +0) = +0, +0 y + +0 = +0): the one zero a caller
// of the *_v forms may let through (an exact difference x - x, which rounds to +0, over a positive divisor).
// tests/test_div_forced_gpu.py drives the *_v forms with the flag set on such zeros, on the call sites' operand
// ranges and on the ends of the conditions above.
//
// The fast path runs only where a whole wave can: the *_v forms take a wave-uniform flag (a vote the caller formed,
// which may cover several divisions whose operands it bounds), div_shared / div_shared2 vote on their own operands.
// A wave with any lane outside takes the plain /, and so does the host build (tests/hostcheck), where the votes
// return the one call's predicate so that the callers' branch structure is the device's.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

#ifndef NUSI_FN
#define NUSI_FN __host__ __device__ inline
#endif

namespace nusi {
namespace nm {

constexpr double kDivLo = 0x1p-380, kDivHi = 0x1p+380;
// finite, nonzero, |x| in [kDivLo, kDivHi) (NaN fails the compares)
NUSI_FN bool div_in_window(double x)
{
    const double a = fabs(x);
    return a >= kDivLo && a < kDivHi;
}
// every active lane's predicate (host: the call's)
NUSI_FN bool div_vote(bool p)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __all(p);
#else
    return p;
#endif
}

#ifdef __HIP_DEVICE_COMPILE__
// 1 / b to the precision the compiler's division refines it to: v_rcp_f64 and two Newton steps
__device__ inline double div_recip(double b)
{
    double y = __builtin_amdgcn_rcp(b);
    y = fma(y, fma(-b, y, 1.0), y);
    y = fma(y, fma(-b, y, 1.0), y);
    return y;
}
// RN(a / b) from y = div_recip(b), operands as the header comment requires
__device__ inline double div_by_recip(double a, double b, double y)
{
    const double q = a * y;
    return fma(fma(-b, q, a), y, q);
}
#endif

// RN(a / b); ok: wave-uniform, true only if every active lane's a and b satisfy the header comment's conditions
NUSI_FN double div_v(bool ok, double a, double b)
{
#ifdef __HIP_DEVICE_COMPILE__
    if (ok) return div_by_recip(a, b, div_recip(b));
#endif
    return a / b;
}
// RN(a0 / b), RN(a1 / b)
NUSI_FN void div2_v(bool ok, double a0, double a1, double b, double& q0, double& q1)
{
#ifdef __HIP_DEVICE_COMPILE__
    if (ok) {
        const double y = div_recip(b);
        q0 = div_by_recip(a0, b, y);
        q1 = div_by_recip(a1, b, y);
        return;
    }
#endif
    q0 = a0 / b;
    q1 = a1 / b;
}
// the same with the vote on the operands themselves
NUSI_FN double div_shared(double a, double b) { return div_v(div_vote(div_in_window(a) && div_in_window(b)), a, b); }
NUSI_FN void div_shared2(double a0, double a1, double b, double& q0, double& q1)
{
    div2_v(div_vote(div_in_window(a0) && div_in_window(a1) && div_in_window(b)), a0, a1, b, q0, q1);
}

}  // namespace nm
}  // namespace nusi
