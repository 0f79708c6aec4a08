// k_inject<NC>'s set-up in front of its loop over the toys (the lane's place, the front half X[0], the templates, tree(X),
// the rows of the outputs, the expectation mu_inj the toys are drawn from, the conditional fit's held term): the text of
// k_inject<NC> and k_nuis_inject<NC, MODE>.  Expects the kernel's arguments R, S, bg, T, ii, o, u0, nqb, M, C, lgC, Q, P.
    constexpr int KT = NC - 1, KA = KT > 0 ? KT : 1;
    const int tid = (int)threadIdx.x, u = u0 + (int)blockIdx.x, t = u / nqb;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, qb0 = (u - t * nqb) * QB, q = qb0 + grp;
    const int cc = c < C ? c : C - 1, qc = q < Q ? q : Q - 1;
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)qc * M;
    const bool in = c < C;
    int p0, p1;
    ens_share(P, (int)blockIdx.z, (int)gridDim.z, p0, p1);
    double X[NC];
    {
        double s0 = 0.0;
#pragma unroll 4
        for (int n = 1; n < M; ++n) s0 = s0 + Rt[(size_t)n * C] * Sq[n];
        X[0] = in ? s0 : 0.0;
    }
#pragma unroll
    for (int j = 1; j < NC; ++j) X[j] = in ? T[(size_t)(j - 1) * C + cc] : 0.0;
    const double b = in ? bg[cc] : 0.0;
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto min = [](double x, double y) { return y < x ? y : x; };
    auto any = [&](bool x) { return (__ballot(x) & gmask) != 0; };
    double S1h[NC];   // tree(X_j): the data do not enter
#pragma unroll
    for (int j = 0; j < NC; ++j) S1h[j] = X[j];
    det_butterfly(S1h, lgC, add);
    const size_t rq = (size_t)t * Q + qc;                     // the spectrum's row of the call's arrays
    const size_t rc = (size_t)(u - u0) * QB + grp;            // ... and of the chunk's scratch
    const size_t rth = (o.theta_compact ? rc : rq) * P, rst = (o.stat_compact ? rc : rq) * P;
    const double atest = ii.a_test[qc];
    const double qobs = ii.qobs ? ii.qobs[rq] : __builtin_nan("");
    // the expectation the toys are drawn from (padding lanes: 0, which draws nothing)
    double mu_inj = ii.a_inj[qc] * X[0];
#pragma unroll
    for (int j = 1; j < NC; ++j) mu_inj = mu_inj + ii.th_inj[j] * X[j];
    mu_inj = mu_inj + b;
    const double asig = atest * X[0];   // the held term of the conditional fit's den
    bool supt = false;                  // a live template supports the bin
    int nlt = 0;                        // the live templates
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        if (S1h[i + 1] > 0.0 && X[i + 1] > 0.0) supt = true;
        nlt += S1h[i + 1] > 0.0 ? 1 : 0;
    }

