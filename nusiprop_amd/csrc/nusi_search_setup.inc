// The search for a profile-likelihood limit, what both sides share: the uniform values it holds for long, the chain's
// flags, and the first step in a from the quadratic model at the best fit.  nusi_detector.hip includes it in k_interval
// and, per data set, in k_toys_limit, after the best fit and in front of the loop over the sides, whose body is
// nusi_search_side.inc.
// In scope: NC, KT = NC - 1, KA = max(KT, 1) (constexpr); X[NC], b, d, in; the best fit's thh[NC], S1h[NC] = tree(X),
// muh (its mu_c); pr (FitPrior), ku, klu, delta; lgC and the lambdas add, any(bool).
// It leaves behind, for nusi_search_side.inc: pm_[KA], pw_[KA], ku_, klu_, hd = delta / 2; S10, ahat; the flags' names
// (an enum), cf (kLact | kSupt | kZeroOk), nl (the live templates), step, NI (constexpr).
    // (uniform values the search holds for long, moved to vector registers: the scalar file is the tight one here)
    double pm_[KA], pw_[KA], ku_ = ku, klu_ = klu, hd = 0.5 * delta;
#pragma unroll
    for (int i = 0; i < KA; ++i) {
        pm_[i] = i < KT ? pr.m[(i + 1) < NC ? i + 1 : 0] : 0.0;
        pw_[i] = i < KT ? pr.w[(i + 1) < NC ? i + 1 : 0] : 0.0;
        asm volatile("" : "+v"(pm_[i]), "+v"(pw_[i]));
    }
    asm volatile("" : "+v"(ku_), "+v"(klu_), "+v"(hd));
    const double S10 = S1h[0], ahat = thh[0];
    // The chain's long-lived flags are bits of ONE vector register: held as bools they are lane masks, a pair of scalar
    // registers each, and with the inner iteration's own the kernel ran out of scalar registers (73 spilled at NC = 4).
    enum { kLact = 1, kSupt = 2, kZeroOk = 4, kRun = 8, kSeen = 16, kZeroDone = 32, kRan = 64, kIRun = 1, kFirst = 2, kWarm = 4, kQuad = 8 };
    int cf = (in && d > 0.0 && muh > 0.0) ? kLact : 0;   // kSupt: a live template supports the bin
    int nl = 0;
#pragma unroll
    for (int i = 0; i < KT; ++i) {
        if (S1h[i + 1] > 0.0 && X[i + 1] > 0.0) cf |= kSupt;
        nl += S1h[i + 1] > 0.0 ? 1 : 0;
    }
    if (!any(d > 0.0 && X[0] > 0.0 && !(b > 0.0) && !(cf & kSupt))) cf |= kZeroOk;
    double step;
    {
        const double wq0 = d / muh;
        const double wq = (cf & kLact) ? wq0 : 0.0;
        const double r0 = wq / muh;
        const double rqq = (cf & kLact) ? r0 : 0.0;
        double S3[1] = {(X[0] * rqq) * X[0]};
        det_butterfly(S3, lgC, add);
        // the quadratic model's step rounded up to a power of two: 2^ceil(e / 2), delta / S3 = f 2^e, f in [1/2, 1)
        const int e = __builtin_amdgcn_frexp_exp(delta / S3[0]);   // frexp's exponent (0 for inf), no stack slot
        const double pw2 = ldexp(1.0, ((e + 1025) >> 1) - 512);
        const double lin = hd / S10;
        step = S3[0] > 0.0 ? pw2 : lin;
    }
    constexpr int NI = 1 + KT + KT * (KT + 1) / 2;   // an inner round's sums: S2_j, H_jk (1 <= j <= k), then S2_0
