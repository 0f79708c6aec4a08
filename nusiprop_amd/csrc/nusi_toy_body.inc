// One data set through the calibration calls' steps 2 - 4 (include/nusi.h nusi_plan_response_inject): the best fit, ONE
// conditional fit with the signal held at `atest` from the header's cold start, lambda by k_interval's ratio form and
// the statistic under ii.mode.  Included by k_inject<NC> (per toy) and k_belt<NC> (the observed pass and per toy).
// Expects: NC, KT, KA; in, d (the lane's datum; 0 in a padding lane), X[NC], S1h[NC] = tree(X), b, lgC, the lambdas add,
// min, any; atest, asig = atest X[0], supt, nlt; pr, ku, ii.mode.  Leaves: thh[NC], muh, sth (the best fit, its mu and
// word); th[KA], st, mu (the conditional fit's); stat, th0 (NaN as the rules say), nofit, nocond.
        // ---- the best fit --------------------------------------------------------------------------------------------
        double thh[NC], muh;
        int sth;
        if constexpr (NC == 1) {
            double S1[1] = {S1h[0]};
#include "nusi_profile_chain1.inc"
            thh[0] = a[0];
            muh = m;
            sth = st;
        } else {
            constexpr int NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major)
            double S1[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) S1[j] = S1h[j];
#define FN_NSIG 1
#include "nusi_fit_newton.inc"
#undef FN_NSIG
#pragma unroll
            for (int j = 0; j < NC; ++j) thh[j] = th[j];
            muh = m;
            sth = st;
        }

        // ---- the conditional fit at a_test, from the header's cold start ------------------------------------------------
        double th[KA];
        int st = 0;   // (the conditional fit's word; sth: the best fit's)
        if constexpr (KT > 0) {
            constexpr int NS = KT + KT * (KT + 1) / 2;
            const bool sup = b > 0.0 || (atest > 0.0 && X[0] > 0.0) || supt;
            const bool act = d > 0.0 && sup;
            double dsum[1] = {act ? d : 0.0}, dmin[1] = {act ? d : 1.0};
            det_butterfly(dsum, lgC, add);
            det_butterfly(dmin, lgC, min);
            const double D0 = dsum[0], dq = 0.0625 * (dmin[0] < 1.0 ? dmin[0] : 1.0);
            double the[KT], pp[KT];
#pragma unroll
            for (int i = 0; i < KT; ++i) {
                const double x = D0 / ((double)nlt * S1h[i + 1]);
                th[i] = S1h[i + 1] > 0.0 ? x : 0.0;
                the[i] = th[i];
                pp[i] = 0.0;
            }
            double tt = 1.0;
            int steps = 0, halv = 0, trials = 0;
            bool run = true, first = true, quad = false;
#define CF_N KT
#define CF_X(i) X[(i) + 1]
#define CF_S1(i) S1h[(i) + 1]
#define CF_LIVE(i) (S1h[(i) + 1] > 0.0)
#include "nusi_conditional_newton.inc"
#undef CF_N
#undef CF_X
#undef CF_S1
#undef CF_LIVE
            st |= steps | ((halv < NUSI_FIT_TRIALS_MASK ? halv : NUSI_FIT_TRIALS_MASK) << NUSI_FIT_TRIALS_SHIFT);
        } else {
            th[0] = 0.0;
        }
        double mu = asig;
#pragma unroll
        for (int i = 0; i < KT; ++i) mu = mu + th[i] * X[i + 1];
        mu = mu + b;
        if constexpr (KT > 0) {
#pragma unroll
            for (int i = 0; i < KT; ++i)
                if (th[i] == 0.0) st |= NUSI_FIT_ZERO << (i + 1);
            if (any(in && d > 0.0 && mu == 0.0)) st |= NUSI_FIT_INFINITE;
        }

        // ---- lambda from ratios against the best fit's counts (k_interval's), and the statistic -----------------------
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
        for (int j = 0; j < KT; ++j)
            if (pr.w[j + 1] > 0.0) {
                const double dj = th[j] - thh[(j + 1) < NC ? j + 1 : 0];
                const double sj = (th[j] - pr.m[j + 1]) + (thh[(j + 1) < NC ? j + 1 : 0] - pr.m[j + 1]);
                const double pd = ((0.5 * pr.w[j + 1]) * dj) * sj;
                lam = lam + pd;
            }
        double stat = lam > 0.0 ? 2.0 * lam : 0.0, th0 = thh[0];
        if ((ii.mode == 1 && th0 > atest) || (ii.mode == 2 && th0 < atest)) stat = 0.0;
        const bool nofit = (sth & (NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR)) != 0;
        const bool nocond = (st & (NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR)) != 0;
        if (nofit) th0 = __builtin_nan("");
        if (nofit || nocond) stat = __builtin_nan("");
