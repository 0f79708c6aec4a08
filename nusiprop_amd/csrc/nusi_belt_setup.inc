// k_belt<NC>'s set-up in front of its loop over the passes (the record's place, the front half X[0], the templates,
// tree(X), the test scale, the conditional fit's held term, and mu_inj, qobs, valid, which the observed pass sets): the
// text of k_belt<NC> and k_nuis_belt<NC>.  Expects the kernel's arguments R, S, bg, T, ii, o, u0, nrb, M, C, lgC, Q, P.
    constexpr int KT = NC - 1, KA = KT > 0 ? KT : 1;
    const int G = ii.G, QG = Q * G;
    const int tid = (int)threadIdx.x, u = u0 + (int)blockIdx.x, t = u / nrb;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, row = (u - t * nrb) * QB + grp;
    const int cc = c < C ? c : C - 1, rc = row < QG ? row : QG - 1, q = rc / G, gp = rc - q * G;   // q < Q, gp < G
    const int pair = t * Q + q;
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)q * M;
    const bool in = c < C;
    const bool mine = row < QG && pair >= ii.pr0 && pair < ii.pr1;   // the record is this launch's to store
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
    const double rf = ii.ref ? ii.ref[pair] : 1.0;
    const double agrid = ii.frac[gp] * rf;
    const bool agood = rf >= 0.0 && agrid < __builtin_inf();
    const double atest = agood ? agrid : 0.0;
    const size_t rg = (size_t)pair * G + gp;                    // the record's row of the call's [ntab][Q][G] arrays
    const double asig = atest * X[0];   // the held term of the conditional fit's den
    bool supt = false;                  // a live template supports the bin
    int nlt = 0;                        // the live templates
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        if (S1h[i + 1] > 0.0 && X[i + 1] > 0.0) supt = true;
        nlt += S1h[i + 1] > 0.0 ? 1 : 0;
    }
    double mu_inj = 0.0, qobs = __builtin_nan("");   // both set by the observed pass
    bool valid = false;

