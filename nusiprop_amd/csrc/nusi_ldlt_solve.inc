// The Newton direction of the damped iterations: pp = -H^-1 g on the free set fs by L D L^T in ascending order (the
// other components: an identity row, pp = 0); a component at zero that the direction pushes below leaves fs and the
// solve is repeated.  Then acc = g . pp over fs.  Included where the direction is formed by nusi_fit_newton.inc,
// nusi_conditional_newton.inc and the inner iteration of nusi_search_side.inc, which #define in front of the #include and
// #undef behind it:
//   LS_N       the number of components
//   LS_NA      the arrays' length, max(LS_N, 1)
//   LS_PW(j)   the prior's weight of component j, added to H_jj
// In scope besides: v[] (the round's sums: H_jk, j <= k row-major, from v[LS_N]), g[LS_NA], fs[LS_NA], th[LS_NA],
// pp[LS_NA].
// It leaves behind: pp (the direction), fs (the free set it holds on), sing (a pivot was not > 0: pp is not to be used),
// acc.
    bool sing = false;
#pragma unroll 1
    for (int rep = 0; rep <= LS_N; ++rep) {
        double Lm[LS_NA][LS_NA], Dg[LS_NA], y[LS_NA];
        sing = false;
        int i0 = LS_N;
        double hm[LS_NA][LS_NA];
#pragma unroll
        for (int j = 0; j < LS_N; ++j)
#pragma unroll
            for (int k = j; k < LS_N; ++k) {
                const double hv = v[i0++] + (j == k ? LS_PW(j) : 0.0);
                hm[k][j] = (fs[j] && fs[k]) ? hv : (j == k ? 1.0 : 0.0);
            }
#pragma unroll
        for (int i = 0; i < LS_N; ++i) {
            double cw[LS_NA];
#pragma unroll
            for (int j = 0; j < i; ++j) {
                double x = hm[i][j];
#pragma unroll
                for (int k = 0; k < j; ++k) x = x - cw[k] * Lm[j][k];
                cw[j] = x;
                Lm[i][j] = x / Dg[j];
            }
            double x = hm[i][i];
#pragma unroll
            for (int k = 0; k < i; ++k) x = x - cw[k] * Lm[i][k];
            if (!(x > 0.0)) sing = true;
            Dg[i] = x;
        }
#pragma unroll
        for (int i = 0; i < LS_N; ++i) {
            double x = fs[i] ? -g[i] : 0.0;
#pragma unroll
            for (int k = 0; k < i; ++k) x = x - Lm[i][k] * y[k];
            y[i] = x;
        }
#pragma unroll
        for (int i = LS_N - 1; i >= 0; --i) {
            double x = y[i] / Dg[i];
#pragma unroll
            for (int k = i + 1; k < LS_N; ++k) x = x - Lm[k][i] * pp[k];
            pp[i] = x;
        }
        if (sing) break;
        bool rm = false;
#pragma unroll
        for (int j = 0; j < LS_N; ++j)
            if (fs[j] && th[j] == 0.0 && pp[j] < 0.0) {
                fs[j] = false;
                rm = true;
            }
        if (!rm) break;
    }
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < LS_N; ++j)
        if (fs[j]) acc = acc + g[j] * pp[j];
