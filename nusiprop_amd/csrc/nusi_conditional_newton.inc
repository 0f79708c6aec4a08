// The rounds of k_conditional_fit's damped Newton iteration over the templates' normalisations with the signal's term
// held in den: the loop of nusi_fit_newton.inc on the components 1 .. K alone (what differs: include/nusi.h, and the
// block comment of k_conditional_fit).  nusi_detector.hip includes it in k_conditional_fit and, per toy, in k_inject.
// The cold start and the counters stay in front of it at each site: declared in the fragment, or in one order at both
// sites, they moved an instruction of k_conditional_fit<1> or of k_inject<2>.  Arrays of the free components are indexed
// i = j - 1; the two kernels keep X, tree(X) and the liveness in different places, which four token parameters
// reconcile -- the site #defines them in front of the #include and #undefs them behind it:
//   CF_N        the number of free components, K       (k_conditional_fit: NC;       k_inject: KT)
//   CF_X(i)     the lane's T_{i+1,c}                   (k_conditional_fit: X[i];     k_inject: X[(i) + 1])
//   CF_S1(i)    its sum over the bins                  (k_conditional_fit: S1[i];    k_inject: S1h[(i) + 1])
//   CF_LIVE(i)  is component i + 1 live                (k_conditional_fit: live[i];  k_inject: (S1h[(i) + 1] > 0.0))
// In scope besides: NS = CF_N + CF_N (CF_N + 1) / 2 (constexpr); asig (the held term a s_c), b, d, act, dq; th[CF_N],
// the[CF_N] (= th: the start), pp[CF_N] (0), tt (1.0), st, steps, halv, trials (0), run (true), first (true), quad
// (false); pr (FitPrior), ku; lgC and the lambdas add, any(bool).
// It leaves behind: th (the estimate), st (NOT_CONVERGED and SINGULAR added: the site adds the counts and the bits that
// need mu), steps, halv.
    // (every round ends a chain, counts a step towards NUSI_FIT_ITER_MAX or a trial towards NUSI_FIT_TRIALS_MAX)
    while (__any(run)) {
        double v[NS];
        double den = asig;
#pragma unroll
        for (int i = 0; i < CF_N; ++i) den = den + the[i] * CF_X(i);
        den = den + b;
        const double wq0 = d / den;
        const double wq = act ? wq0 : 0.0;
        const double r0 = wq / den;
        const double r = act ? r0 : 0.0;
        {
            int i = CF_N;
#pragma unroll
            for (int j = 0; j < CF_N; ++j) {
                v[j] = CF_X(j) * wq;
                const double xr = CF_X(j) * r;
#pragma unroll
                for (int k = j; k < CF_N; ++k) v[i++] = xr * CF_X(k);
            }
        }
        det_butterfly(v, lgC, add);
        const bool bad = any(act && !(den > 0.0));
        if (run) {
            double g[CF_N];
#pragma unroll
            for (int j = 0; j < CF_N; ++j) g[j] = (CF_S1(j) - v[j]) + pr.w[j + 1] * (the[j] - pr.m[j + 1]);
            bool ok, changed = true;
            if (first) {
                ok = !bad;
                if (!ok) {
                    run = false;
                    st |= NUSI_FIT_NOT_CONVERGED;
                }
            } else {
                double slope = 0.0;
#pragma unroll
                for (int j = 0; j < CF_N; ++j) slope = slope + pp[j] * g[j];
                ok = !bad && (quad || !(slope > 0.0));
                if (!ok) {
                    if (trials == NUSI_FIT_TRIALS_MAX) {
                        run = false;
                        st |= NUSI_FIT_NOT_CONVERGED;
                    } else {
                        ++trials;
                        ++halv;
                        tt = tt * 0.5;
#pragma unroll
                        for (int j = 0; j < CF_N; ++j) the[j] = th[j] + tt * pp[j];
                    }
                } else {
                    changed = false;
#pragma unroll
                    for (int j = 0; j < CF_N; ++j) changed = changed || the[j] != th[j];
                    ++steps;
                }
            }
            if (ok) {
                bool fs[CF_N], conv = true;
#pragma unroll
                for (int j = 0; j < CF_N; ++j) {
                    th[j] = the[j];
                    fs[j] = CF_LIVE(j) && (th[j] > 0.0 || g[j] < 0.0);
                    const double sc = (CF_S1(j) + v[j]) + pr.w[j + 1] * (th[j] + pr.m[j + 1]);
                    const double ag = g[j] < 0.0 ? -g[j] : g[j];
                    if (fs[j] && !(ag <= ku * sc)) conv = false;
                }
                if (conv) {
                    run = false;
                } else if ((!first && !changed) || steps == NUSI_FIT_ITER_MAX) {
                    run = false;
                    st |= NUSI_FIT_NOT_CONVERGED;
                } else {
                    first = false;
#define LS_N CF_N
#define LS_NA CF_N
#define LS_PW(j) pr.w[(j) + 1]
#include "nusi_ldlt_solve.inc"
#undef LS_N
#undef LS_NA
#undef LS_PW
                    if (sing || !(acc < 0.0)) {
                        run = false;
                        st |= NUSI_FIT_SINGULAR;
#pragma unroll
                        for (int j = 0; j < CF_N; ++j) pp[j] = 0.0;
                    } else {
                        double ratio[CF_N];
                        tt = 1.0;
#pragma unroll
                        for (int j = 0; j < CF_N; ++j) {
                            const double x = th[j] / -pp[j];
                            ratio[j] = (fs[j] && pp[j] < 0.0) ? x : 1.0;
                            if (ratio[j] < tt) tt = ratio[j];
                        }
                        const bool clipped = tt < 1.0;
                        quad = !clipped && -acc <= dq;
                        trials = 0;
#pragma unroll
                        for (int j = 0; j < CF_N; ++j) {
                            const double x = th[j] + tt * pp[j];
                            the[j] = (clipped && fs[j] && pp[j] < 0.0 && ratio[j] == tt) ? 0.0 : x;
                        }
                    }
                }
            }
        }
    }
