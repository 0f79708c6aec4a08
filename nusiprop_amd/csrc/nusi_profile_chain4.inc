// k_detector_profile's iteration: Newton's iteration on the signal's scale alone, kEvQ = 4 chains (spectra) a lane,
// from the start's maximum over the bins to the last step.  nusi_detector.hip includes it in k_detector_profile and,
// per data set, in k_ensemble_profile.  The chains' set-up (act, run, st and the lane's candidate for the start) stays
// with each kernel: k_detector_profile forms act before the butterfly of S1 and the rest after it, k_ensemble_profile
// all of it per data set in one loop, and either order in the other kernel moved that kernel's instructions.
// In scope: s[kEvQ] (the lane's s_c per spectrum, 0 on padding lanes), S1[kEvQ] = tree(s), b, d, lgC, the lambdas add
// and max; a[kEvQ] (the lane's d / S1 - b / s where act, else 0), act[kEvQ], run[kEvQ], st[kEvQ] (0, or FLAT).
// It leaves behind: a (the estimates), st (the steps, BOUNDARY and NOT_CONVERGED added; the site adds INFINITE from its
// mu), run (all false).
    det_butterfly(a, lgC, max);
#pragma unroll
    for (int j = 0; j < kEvQ; ++j) a[j] = (run[j] && a[j] > 0.0) ? a[j] : 0.0;
    // (every running chain counts its steps and stops at NUSI_FIT_ITER_MAX: the loop is bounded)
    while (__any(run[0] || run[1] || run[2] || run[3])) {
        double v[2 * kEvQ];
#pragma unroll
        for (int j = 0; j < kEvQ; ++j) {
            double den = a[j] * s[j];
            den = den + b;
            const double q = s[j] / den;
            const double u = act[j] ? q : 0.0;
            const double r = d * u;
            v[j] = r;
            v[kEvQ + j] = r * u;
        }
        det_butterfly(v, lgC, add);
#pragma unroll
        for (int j = 0; j < kEvQ; ++j) {
            const double S2 = v[j], S3 = v[kEvQ + j];
            const double g = S1[j] - S2;
            const double dn = S2 - S1[j];
            const double an = a[j] + dn / S3;
            if (run[j]) {
                ++st[j];
                if (!(g < 0.0)) {
                    run[j] = false;
                    if (a[j] == 0.0) st[j] |= NUSI_FIT_BOUNDARY;
                } else if (!(an > a[j])) {
                    run[j] = false;
                } else {
                    a[j] = an;
                    if ((st[j] & NUSI_FIT_STEPS_MASK) == NUSI_FIT_ITER_MAX) {
                        run[j] = false;
                        st[j] |= NUSI_FIT_NOT_CONVERGED;
                    }
                }
            }
        }
    }
