// k_detector_fit<NC>'s damped Newton iteration over the NC = 1 + K normalisations (include/nusi.h defines it), from the
// liveness of the components to the status word.  nusi_detector.hip includes it in k_detector_fit, in k_ensemble_fit and,
// for NC > 1, in the best fit of k_interval, k_toys_limit and k_inject: one text, so the five agree by construction (a
// call to a shared __device__ body, inlined, moved the kernels' registers: DESIGN.md sec. 4).  The Newton direction
// inside it is nusi_ldlt_solve.inc, shared with the conditional fit's and the search's text.
// k_components_fit<J, NC> includes it too, with J signal components in front of the templates (include/nusi.h,
// nusi_plan_response_fit_components): the includer #defines FN_NSIG, the number of signal components (a constant
// expression, 1 .. NC), in front of the #include and #undefs it behind; the five above define it as 1, where the loops over
// the signal components 1 .. FN_NSIG - 1 below are empty and the text is what it was.
// In scope: NC and NS = NC + NC (NC + 1) / 2 (constexpr); X[NC], S1[NC] = tree(X), b, d, in; pr (m[], w[]: NC entries at
// least, the signal components' zeros in front), ku; lgC and the lambdas add, min, any(bool).
// It leaves behind: th[NC] (the estimate), live[NC], m (the estimate's mu_c), st (the status word, complete), steps,
// halv; and, of no further use, slive, szero, sup, nl, act, D0, dq, the[NC], pp[NC] (the direction), tt, trials, run, first, quad.
    bool live[NC];
    live[0] = any(d > 0.0 && X[0] > 0.0) && S1[0] > 0.0;
    bool sup = b > 0.0;
    int nl = 0;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        if (j > 0) live[j] = j < FN_NSIG ? (any(d > 0.0 && X[j] > 0.0) && S1[j] > 0.0) : S1[j] > 0.0;
        sup = sup || (live[j] && X[j] > 0.0);
        nl += live[j] ? 1 : 0;
    }
    const bool act = d > 0.0 && sup;
    double dsum[1] = {act ? d : 0.0}, dmin[1] = {act ? d : 1.0};   // (1.0: dmin = min(1, the smallest active datum))
    det_butterfly(dsum, lgC, add);
    det_butterfly(dmin, lgC, min);
    const double D0 = dsum[0], dq = 0.0625 * (dmin[0] < 1.0 ? dmin[0] : 1.0);
    double th[NC], the[NC], pp[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const double x = D0 / ((double)nl * S1[j]);
        th[j] = live[j] ? x : 0.0;
        the[j] = th[j];
        pp[j] = 0.0;
    }
    double tt = 1.0;
    int st = 0, steps = 0, halv = 0, trials = 0;
    bool run = true, first = true, quad = false;
    // (every round ends a chain, counts a step towards NUSI_FIT_ITER_MAX or a trial towards NUSI_FIT_TRIALS_MAX)
    while (__any(run)) {
        double v[NS];
        double den = the[0] * X[0];
#pragma unroll
        for (int j = 1; j < NC; ++j) den = den + the[j] * X[j];
        den = den + b;
        const double wq0 = d / den;
        const double wq = act ? wq0 : 0.0;
        const double r0 = wq / den;
        const double r = act ? r0 : 0.0;
        {
            int i = NC;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                v[j] = X[j] * wq;
                const double xr = X[j] * r;   // (not (X_j X_k) r: ten loop-invariant products would stay in registers)
#pragma unroll
                for (int k = j; k < NC; ++k) v[i++] = xr * X[k];
            }
        }
        det_butterfly(v, lgC, add);
        const bool bad = any(act && !(den > 0.0));
        if (run) {
            double g[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) g[j] = (S1[j] - v[j]) + pr.w[j] * (the[j] - pr.m[j]);
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
                for (int j = 0; j < NC; ++j) slope = slope + pp[j] * g[j];
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
                        for (int j = 0; j < NC; ++j) the[j] = th[j] + tt * pp[j];
                    }
                } else {
                    changed = false;
#pragma unroll
                    for (int j = 0; j < NC; ++j) changed = changed || the[j] != th[j];
                    ++steps;
                }
            }
            if (ok) {
                bool fs[NC], conv = true;
#pragma unroll
                for (int j = 0; j < NC; ++j) {
                    th[j] = the[j];
                    fs[j] = live[j] && (th[j] > 0.0 || g[j] < 0.0);
                    const double scale = (S1[j] + v[j]) + pr.w[j] * (th[j] + pr.m[j]);
                    const double ag = g[j] < 0.0 ? -g[j] : g[j];
                    if (fs[j] && !(ag <= ku * scale)) conv = false;
                }
                if (conv) {
                    run = false;
                } else if ((!first && !changed) || steps == NUSI_FIT_ITER_MAX) {
                    run = false;
                    st |= NUSI_FIT_NOT_CONVERGED;
                } else {
                    first = false;
#define LS_N NC
#define LS_NA NC
#define LS_PW(j) pr.w[j]
#include "nusi_ldlt_solve.inc"
#undef LS_N
#undef LS_NA
#undef LS_PW
                    if (sing || !(acc < 0.0)) {
                        run = false;
                        st |= NUSI_FIT_SINGULAR;
#pragma unroll
                        for (int j = 0; j < NC; ++j) pp[j] = 0.0;
                    } else {
                        double ratio[NC];
                        tt = 1.0;
#pragma unroll
                        for (int j = 0; j < NC; ++j) {
                            const double x = th[j] / -pp[j];
                            ratio[j] = (fs[j] && pp[j] < 0.0) ? x : 1.0;
                            if (ratio[j] < tt) tt = ratio[j];
                        }
                        const bool clipped = tt < 1.0;
                        quad = !clipped && -acc <= dq;
                        trials = 0;
#pragma unroll
                        for (int j = 0; j < NC; ++j) {
                            const double x = th[j] + tt * pp[j];
                            the[j] = (clipped && fs[j] && pp[j] < 0.0 && ratio[j] == tt) ? 0.0 : x;
                        }
                    }
                }
            }
        }
    }
    double m = th[0] * X[0];
#pragma unroll
    for (int j = 1; j < NC; ++j) m = m + th[j] * X[j];
    m = m + b;
    bool slive = live[0], szero = th[0] == 0.0;   // some signal component is live; every one ends at zero
#pragma unroll
    for (int j = 1; j < FN_NSIG; ++j) {
        slive = slive || live[j];
        szero = szero && th[j] == 0.0;
    }
    if (!slive)
        st |= NUSI_FIT_FLAT;
    else if (szero)
        st |= NUSI_FIT_BOUNDARY;
#pragma unroll
    for (int j = 0; j < NC; ++j)
        if (th[j] == 0.0) st |= NUSI_FIT_ZERO << j;
    if (any(in && d > 0.0 && m == 0.0)) st |= NUSI_FIT_INFINITE;
    st |= steps | ((halv < NUSI_FIT_TRIALS_MASK ? halv : NUSI_FIT_TRIALS_MASK) << NUSI_FIT_TRIALS_SHIFT);
