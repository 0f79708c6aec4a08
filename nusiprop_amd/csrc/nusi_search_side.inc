// The search for a profile-likelihood limit, one side: the body of `for (int side = 1; side >= 0; --side)` up to the
// side's result.  Newton's iteration in a on lambda(a) = delta / 2 (include/nusi.h); each outer step runs
// k_conditional_fit's iteration at the held a, warm-started from the step before's theta, with the sum S2_0 added to
// the round's butterfly (the Newton direction inside it: nusi_ldlt_solve.inc).  nusi_detector.hip includes it in
// k_interval and, per data set, in k_toys_limit; the site writes res and word where its call wants them (k_toys_limit:
// and tallies the word).
// In scope: side, which; what nusi_search_setup.inc takes and leaves; sth (the best fit's word); lgC and the lambdas
// add, min, any(bool).
// It leaves behind: upper, res (the limit, NaN where there is none) and word (the side's status word).
// The long-lived flags are bits of one register each (cf: the data set's, fl: the outer chain's, il: the inner
// chain's; the comment in nusi_search_setup.inc says why) and must stay so.
        const bool upper = side == 1;
        const bool asked = (which & (upper ? NUSI_LIMIT_UPPER : NUSI_LIMIT_LOWER)) != 0;
        double a = 0.0, res = __builtin_nan("");
        int word = 0, fl = 0;
        if (asked) {
            if (sth & (NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR)) {
                word = NUSI_LIMIT_NO_FIT;
            } else if (S10 == 0.0) {
                res = upper ? __builtin_inf() : 0.0;
                word = upper ? NUSI_LIMIT_UNBOUNDED : (NUSI_LIMIT_UNBOUNDED | NUSI_LIMIT_AT_ZERO);
            } else if (upper) {
                a = ahat + step;
                fl = kRun | kRan;
            } else if (ahat == 0.0) {
                res = 0.0;
                word = NUSI_LIMIT_AT_ZERO;
            } else {
                a = ahat - step;
                if (!(a > 0.0)) a = 0.5 * ahat;
                fl = kRun | kRan;
            }
        }
        double th[KA], aprev = a;
#pragma unroll
        for (int i = 0; i < KA; ++i) th[i] = i < KT ? thh[(i + 1) < NC ? i + 1 : 0] : 0.0;
        int steps = 0, inner = 0, flags = 0;
        // (every round of the outer loop ends a chain or counts a step towards NUSI_LIMIT_ITER_MAX)
        while (__any((fl & kRun) != 0)) {
            // --- k_conditional_fit's iteration at a, from th (the header's start where an active den is not > 0 there) ---
            const double asig = a * X[0];
            const bool sup = b > 0.0 || (cf & kSupt) || (a > 0.0 && X[0] > 0.0);
            const bool act = d > 0.0 && sup;
            double dsum[1] = {act ? d : 0.0}, dmin[1] = {act ? d : 1.0};
            det_butterfly(dsum, lgC, add);
            det_butterfly(dmin, lgC, min);
            const double D0 = dsum[0], dq = 0.0625 * (dmin[0] < 1.0 ? dmin[0] : 1.0);
            double the[KA], pp[KA], S20 = 0.0;
#pragma unroll
            for (int i = 0; i < KA; ++i) {
                the[i] = th[i];
                pp[i] = 0.0;
            }
            double tt = 1.0;
            int ist = 0, isteps = 0, trials = 0;
            int il = ((fl & kRun) ? kIRun : 0) | kFirst | kWarm;   // (the inner chain's flags, bits as well)
            while (__any((il & kIRun) != 0)) {
                double v[NI];
                double den = asig;
#pragma unroll
                for (int i = 0; i < KT; ++i) den = den + the[i] * X[i + 1];
                den = den + b;
                const double wq0 = d / den;
                const double wq = act ? wq0 : 0.0;
                const double r0 = wq / den;
                const double r = act ? r0 : 0.0;
                {
                    int i = KT;
#pragma unroll
                    for (int j = 0; j < KT; ++j) {
                        v[j] = X[j + 1] * wq;
                        const double xr = X[j + 1] * r;
#pragma unroll
                        for (int k = j; k < KT; ++k) v[i++] = xr * X[k + 1];
                    }
                    v[NI - 1] = X[0] * wq;
                }
                det_butterfly(v, lgC, add);
                const bool bad = any(act && !(den > 0.0));
                if (il & kIRun) {
                    double g[KA];
#pragma unroll
                    for (int j = 0; j < KT; ++j) g[j] = (S1h[j + 1] - v[j]) + pw_[j] * (the[j] - pm_[j]);
                    bool ok, changed = true;
                    if (il & kFirst) {
                        ok = !bad;
                        if (!ok) {
                            if (il & kWarm) {
                                il &= ~kWarm;
#pragma unroll
                                for (int j = 0; j < KT; ++j) {
                                    const double x = D0 / ((double)nl * S1h[j + 1]);
                                    th[j] = S1h[j + 1] > 0.0 ? x : 0.0;
                                    the[j] = th[j];
                                }
                            } else {
                                il &= ~kIRun;
                                ist |= NUSI_FIT_NOT_CONVERGED;
                            }
                        }
                    } else {
                        double slope = 0.0;
#pragma unroll
                        for (int j = 0; j < KT; ++j) slope = slope + pp[j] * g[j];
                        ok = !bad && ((il & kQuad) || !(slope > 0.0));
                        if (!ok) {
                            if (trials == NUSI_FIT_TRIALS_MAX) {
                                il &= ~kIRun;
                                ist |= NUSI_FIT_NOT_CONVERGED;
                            } else {
                                ++trials;
                                tt = tt * 0.5;
#pragma unroll
                                for (int j = 0; j < KT; ++j) the[j] = th[j] + tt * pp[j];
                            }
                        } else {
                            changed = false;
#pragma unroll
                            for (int j = 0; j < KT; ++j) changed = changed || the[j] != th[j];
                            ++isteps;
                        }
                    }
                    if (ok) {
                        bool fs[KA], conv = true;
                        S20 = v[NI - 1];
#pragma unroll
                        for (int j = 0; j < KT; ++j) {
                            th[j] = the[j];
                            fs[j] = S1h[j + 1] > 0.0 && (th[j] > 0.0 || g[j] < 0.0);
                            const double sc = (S1h[j + 1] + v[j]) + pw_[j] * (th[j] + pm_[j]);
                            const double ag = g[j] < 0.0 ? -g[j] : g[j];
                            if (fs[j] && !(ag <= ku_ * sc)) conv = false;
                        }
                        if (conv) {
                            il &= ~kIRun;
                        } else if ((!(il & kFirst) && !changed) || isteps == NUSI_FIT_ITER_MAX) {
                            il &= ~kIRun;
                            ist |= NUSI_FIT_NOT_CONVERGED;
                        } else {
                            il &= ~kFirst;
#define LS_N KT
#define LS_NA KA
#define LS_PW(j) pw_[j]
#include "nusi_ldlt_solve.inc"
#undef LS_N
#undef LS_NA
#undef LS_PW
                            if (sing || !(acc < 0.0)) {
                                il &= ~kIRun;
                                ist |= NUSI_FIT_SINGULAR;
                            } else {
                                double ratio[KA];
                                tt = 1.0;
#pragma unroll
                                for (int j = 0; j < KT; ++j) {
                                    const double x = th[j] / -pp[j];
                                    ratio[j] = (fs[j] && pp[j] < 0.0) ? x : 1.0;
                                    if (ratio[j] < tt) tt = ratio[j];
                                }
                                const bool clipped = tt < 1.0;
                                il = (!clipped && -acc <= dq) ? (il | kQuad) : (il & ~kQuad);
                                trials = 0;
#pragma unroll
                                for (int j = 0; j < KT; ++j) {
                                    const double x = th[j] + tt * pp[j];
                                    the[j] = (clipped && fs[j] && pp[j] < 0.0 && ratio[j] == tt) ? 0.0 : x;
                                }
                            }
                        }
                    }
                }
            }
            // --- lambda(a) - delta / 2 from ratios, its magnitude, and the step in a ---
            double mu = asig;
#pragma unroll
            for (int i = 0; i < KT; ++i) mu = mu + th[i] * X[i + 1];
            mu = mu + b;
            double lv[2];
            {
                const double dmu = mu - muh;
                const double ratio = mu / muh;
                const double lr = ratio > 0.0 ? nm::log_i(ratio) : -__builtin_inf();
                const double pl = d * lr;
                const double admu = dmu < 0.0 ? -dmu : dmu, apl = pl < 0.0 ? -pl : pl;
                const double tl = dmu - pl, ml = admu + apl;
                lv[0] = (cf & kLact) ? tl : dmu;
                lv[1] = (cf & kLact) ? ml : admu;
            }
            det_butterfly(lv, lgC, add);
            if (fl & kRun) {
                inner += isteps;
                if (ist & (NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR)) {
                    flags |= NUSI_LIMIT_NOT_CONVERGED;
                    fl &= ~kRun;
                } else {
                    ++steps;
                    double lam = lv[0], mg = lv[1];
#pragma unroll
                    for (int j = 0; j < KT; ++j)
                        if (pw_[j] > 0.0) {
                            const double dj = th[j] - thh[(j + 1) < NC ? j + 1 : 0];
                            const double sj = (th[j] - pm_[j]) + (thh[(j + 1) < NC ? j + 1 : 0] - pm_[j]);
                            const double pd = ((0.5 * pw_[j]) * dj) * sj;
                            lam = lam + pd;
                            mg = mg + (pd < 0.0 ? -pd : pd);
                        }
                    const double h = lam - hd;
                    const double eps = klu_ * (mg + hd);
                    const double g0 = S10 - S20;
                    const double ah = h < 0.0 ? -h : h;
                    if (!upper && a == 0.0) {   // the one look at zero: the limit is there, or the search goes back
                        if (!(h > 0.0)) {
                            flags |= NUSI_LIMIT_AT_ZERO;
                            fl &= ~kRun;
                        } else if (steps == NUSI_LIMIT_ITER_MAX) {
                            flags |= NUSI_LIMIT_NOT_CONVERGED;
                            fl &= ~kRun;
                        } else {
                            fl = (fl | kZeroDone) & ~kSeen;
                            a = 0.5 * aprev;
                        }
                    } else if (ah <= eps || ((fl & kSeen) && !(h > 0.0))) {
                        fl &= ~kRun;
                    } else {
                        fl = h > 0.0 ? (fl | kSeen) : (fl & ~kSeen);
                        if (steps == NUSI_LIMIT_ITER_MAX || !(upper ? g0 > 0.0 : g0 < 0.0)) {
                            flags |= NUSI_LIMIT_NOT_CONVERGED;
                            fl &= ~kRun;
                        } else {
                            double an = a - h / g0;
                            if (!upper && !(an > 0.0)) {
                                fl &= ~kSeen;
                                if ((cf & kZeroOk) && !(fl & kZeroDone)) {
                                    aprev = a;
                                    an = 0.0;
                                } else {
                                    an = 0.5 * a;
                                }
                            }
                            if (!(an < __builtin_inf())) {
                                flags |= NUSI_LIMIT_NOT_CONVERGED;
                                fl &= ~kRun;
                            } else if (an == a) {
                                fl &= ~kRun;
                            } else {
                                a = an;
                            }
                        }
                    }
                }
            }
        }
        if (fl & kRan) {
            res = a;
            word = steps | flags | ((inner < NUSI_LIMIT_INNER_MASK ? inner : NUSI_LIMIT_INNER_MASK) << NUSI_LIMIT_INNER_SHIFT);
        }
