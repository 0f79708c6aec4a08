// nuSIprop MI355X -- TEST ONLY: one dispatch over the special functions, shared by the device kernel
// k_debug_specfun (nusi_debug_specfun.hip, entry nusi_debug_specfun) and its host twin hc_specfun_n (tests/hostcheck).
//
// debug_specfun<FN>(a, b, c, o0, o1) is the single call expression of function FN, written as the kernels call it;
// a function of fewer arguments ignores the rest, one of a single result sets o1 = +0.  The numbers are the test's
// interface (tests/specfun_cases.py holds the same list); no product code includes this header.
#pragma once

#include "nusi_physics.hpp"

namespace nusi {

enum DebugSpecfun {
    kDsLog = 0,        // nm::log(a)
    kDsLogI,           // nm::log_i(a)
    kDsLog1p,          // nm::log1p(a)
    kDsExp,            // nm::exp(a)
    kDsAtan,           // nm::atan(a)
    kDsAtanh,          // nm::atanh(a)
    kDsLog10,          // nm::log10(a)
    kDsPow,            // nm::pow(a, b), a > 0
    kDsSqrt,           // o0 = sqrt(a); o1 = cabs(a + i b) = sqrt(a a + b b)
    kDsClog,           // clog(a + i b)
    kDsCdivReal,       // a / (b + i c): the member chain's quotient, operator/(double, cd) (Smith)
    kDsCdiv,           // (a - i c) / (b + i c): operator/(cd, cd) with a complex numerator, as alpha_member_ref_arg's
    kDsCdivV,          // cdiv_v(w, a, b + i c), w its own div_vote of alpha_member_win on a, b, c
    kDsLi2,            // li2(a)
    kDsLi3,            // li3(a), a in [-1, 1/2]
    kDsCli2,           // cli2(a, b)
    kDsGslLi2,         // gsl_li2(a)
    kDsClausen,        // gsl::clausen(a)
    kDsHypot,          // gsl::hypot<false>(a, b)
    kDsHypotW,         // gsl::hypot<true>(a, b), inside its caller's bounds
    kDsGslCli2,        // gsl_cli2(a, b)
    kDsGslCli2Inl,     // gsl_cli2_inl(a, b), inside the member window
    kDsMemberDc,       // alpha_member_ref_dc(S = a, t = b, gr = c)
    kDsMemberDcInl,    // alpha_member_ref_dc_inl(S = a, t = b, gr = c)
    kDsCount
};

template <int FN>
NUSI_FN void debug_specfun(double a, double b, double c, double& o0, double& o1)
{
    static_assert(FN >= 0 && FN < kDsCount, "debug_specfun: no such function");
    o1 = 0.0;
    if constexpr (FN == kDsLog) o0 = nm::log(a);
    else if constexpr (FN == kDsLogI) o0 = nm::log_i(a);
    else if constexpr (FN == kDsLog1p) o0 = nm::log1p(a);
    else if constexpr (FN == kDsExp) o0 = nm::exp(a);
    else if constexpr (FN == kDsAtan) o0 = nm::atan(a);
    else if constexpr (FN == kDsAtanh) o0 = nm::atanh(a);
    else if constexpr (FN == kDsLog10) o0 = nm::log10(a);
    else if constexpr (FN == kDsPow) o0 = nm::pow(a, b);
    else if constexpr (FN == kDsSqrt) {
        o0 = sqrt(a);
        o1 = cabs(C(a, b));
    } else if constexpr (FN == kDsLi2) o0 = li2(a);
    else if constexpr (FN == kDsLi3) o0 = li3(a);
    else if constexpr (FN == kDsGslLi2) o0 = gsl_li2(a);
    else if constexpr (FN == kDsClausen) o0 = gsl::clausen(a);
    else if constexpr (FN == kDsHypot) o0 = gsl::hypot<false>(a, b);
    else if constexpr (FN == kDsHypotW) o0 = gsl::hypot<true>(a, b);
    else {
        cd z;
        if constexpr (FN == kDsClog) z = clog(C(a, b));
        else if constexpr (FN == kDsCdivReal) z = a / C(b, c);
        else if constexpr (FN == kDsCdiv) z = C(a, -c) / C(b, c);
        else if constexpr (FN == kDsCdivV)
            z = cdiv_v(nm::div_vote(alpha_member_win(a) && alpha_member_win(b) && alpha_member_win(c)), C(a), C(b, c));
        else if constexpr (FN == kDsCli2) z = cli2(a, b);
        else if constexpr (FN == kDsGslCli2) z = gsl_cli2(a, b);
        else if constexpr (FN == kDsGslCli2Inl) z = gsl_cli2_inl(a, b);
        else if constexpr (FN == kDsMemberDc) z = alpha_member_ref_dc(a, b, c);
        else z = alpha_member_ref_dc_inl(a, b, c);
        o0 = z.r;
        o1 = z.i;
    }
}

}  // namespace nusi
