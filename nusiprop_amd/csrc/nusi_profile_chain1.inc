// k_detector_profile's iteration as ONE chain a lane: the best fit without templates (NC == 1) of k_interval,
// k_toys_limit and k_inject, which nusi_detector.hip includes it in.  The operations are those of one chain j of
// k_detector_profile (its set-up and nusi_profile_chain4.inc), so the estimate and the word have
// nusi_plan_response_profile's bits.
// In scope: X[0] (the lane's s_c), S1[1] = {tree(s)} (k_interval forms it by the butterfly, the per-toy kernels copy
// S1h[0]), b, d, in, gmask, lgC and the lambda add.
// It leaves behind: a[0] (the estimate), m (its mu_c), st (the status word, complete); and s, act, run, max.
    auto max = [](double x, double y) { return y > x ? y : x; };
    const double s = X[0];
    double a[1];
    const bool act = d > 0.0 && s > 0.0;
    bool run = S1[0] != 0.0 && (__ballot(act) & gmask) != 0;
    int st = run ? 0 : NUSI_FIT_FLAT;
    {
        const double x0 = d / S1[0], x1 = b / s;
        a[0] = act ? x0 - x1 : 0.0;
    }
    det_butterfly(a, lgC, max);
    a[0] = (run && a[0] > 0.0) ? a[0] : 0.0;
    // (every running chain counts its steps and stops at NUSI_FIT_ITER_MAX: the loop is bounded)
    while (__any(run)) {
        double v[2];
        {
            double den = a[0] * s;
            den = den + b;
            const double qq = s / den;
            const double uu = act ? qq : 0.0;
            const double r = d * uu;
            v[0] = r;
            v[1] = r * uu;
        }
        det_butterfly(v, lgC, add);
        {
            const double S2 = v[0], S3 = v[1];
            const double g = S1[0] - S2;
            const double dn = S2 - S1[0];
            const double an = a[0] + dn / S3;
            if (run) {
                ++st;
                if (!(g < 0.0)) {
                    run = false;
                    if (a[0] == 0.0) st |= NUSI_FIT_BOUNDARY;
                } else if (!(an > a[0])) {
                    run = false;
                } else {
                    a[0] = an;
                    if ((st & NUSI_FIT_STEPS_MASK) == NUSI_FIT_ITER_MAX) {
                        run = false;
                        st |= NUSI_FIT_NOT_CONVERGED;
                    }
                }
            }
        }
    }
    double m = a[0] * s;
    m = m + b;
    if ((__ballot(in && d > 0.0 && m == 0.0) & gmask) != 0) st |= NUSI_FIT_INFINITE;
