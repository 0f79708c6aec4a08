// One data set through steps 2 - 4 of nusi_plan_response_composition_belt (include/nusi.h): the FREE fit of the three
// signal components and the K templates (k_components_fit<3, 3 + K>'s iteration), the HELD fit at the record's
// composition -- the composed signal's scale and the templates float: k_detector_fit<1 + K>'s iteration, at K = 0
// k_detector_profile's chain --, lambda by k_interval's ratio form and the statistic.  Included by
// k_composition_belt<NCF> for the observed pass and per toy.  The iterations are the existing texts, #included here in
// blocks of their own, each with the names that text expects (NC, NS, X, S1, pr, ku) bound to this kernel's values.
// Expects: NCF, KT = NCF - 3; in, d (the lane's datum; 0 in a padding lane), XF[NCF] (s_0 .. s_2, T_1 .. T_K), S1F[NCF]
// = tree(XF), sphi, S1p = tree(sphi), b, lgC, gmask, the lambdas add, min, any; prf (m[], w[]: NCF entries, the signal
// components' zeros in front), tp (the plan's FitPrior), kuf, kuh.  Leaves: thh[NCF], muh, sth (the free fit, its mu
// and word); thc[1 + KT], mu, stc (the held fit's); stat (NaN as the rules say), nofit, nocond.
        // ---- the free fit ---------------------------------------------------------------------------------------------
        double thh[NCF], muh;
        int sth;
        {
            constexpr int NC = NCF, NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major)
            double X[NC], S1[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                X[j] = XF[j];
                S1[j] = S1F[j];
            }
            const auto& pr = prf;
            const double ku = kuf;
#define FN_NSIG 3
#include "nusi_fit_newton.inc"
#undef FN_NSIG
#pragma unroll
            for (int j = 0; j < NC; ++j) thh[j] = th[j];
            muh = m;
            sth = st;
        }

        // ---- the held fit at the record's composition ------------------------------------------------------------------
        double thc[1 + KT], mu;
        int stc;
        if constexpr (KT == 0) {
            double X[1] = {sphi}, S1[1] = {S1p};
#include "nusi_profile_chain1.inc"
            thc[0] = a[0];
            mu = m;
            stc = st;
        } else {
            constexpr int NC = 1 + KT, NS = NC + NC * (NC + 1) / 2;
            double X[NC], S1[NC];
            X[0] = sphi;
            S1[0] = S1p;
#pragma unroll
            for (int j = 1; j < NC; ++j) {
                X[j] = XF[2 + j];
                S1[j] = S1F[2 + j];
            }
            const FitPrior& pr = tp;
            const double ku = kuh;
#define FN_NSIG 1
#include "nusi_fit_newton.inc"
#undef FN_NSIG
#pragma unroll
            for (int j = 0; j < NC; ++j) thc[j] = th[j];
            mu = m;
            stc = st;
        }

        // ---- lambda from ratios against the free fit's counts (k_interval's), and the statistic -------------------------
        double lv[1];
        {
            const bool lact = in && d > 0.0 && muh > 0.0;
            const double dmu = mu - muh;
            const double ratio = mu / muh;
            const double lr = ratio > 0.0 ? nm::log_i(ratio) : -__builtin_inf();
            const double pl = d * lr;
            const double tl = dmu - pl;
            lv[0] = lact ? tl : dmu;
        }
        det_butterfly(lv, lgC, add);
        double lam = lv[0];
#pragma unroll
        for (int j = 1; j <= KT; ++j)
            if (tp.w[j] > 0.0) {
                const double dj = thc[j] - thh[2 + j];
                const double sj = (thc[j] - tp.m[j]) + (thh[2 + j] - tp.m[j]);
                const double pd = ((0.5 * tp.w[j]) * dj) * sj;
                lam = lam + pd;
            }
        double stat = lam > 0.0 ? 2.0 * lam : 0.0;
        const bool nofit = (sth & (NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR)) != 0;
        const bool nocond = (stc & (NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR)) != 0;
        if (nofit || nocond) stat = __builtin_nan("");
