// The statistic of one spectrum of the block from its row of LDS, by the lane that owns it, in the defined serial order:
// the Poisson terms mu_c - data_c log(mu_c) ascending in c from 0.0, then the Gaussian penalties of the templates with a
// prior, ascending.  nusi_detector.hip includes it behind the kernel's one barrier, inside
// `if (tid < QB && qb0 + tid < Q) { ... }`, in k_detector_fit, k_components_fit, k_conditional_fit and k_interval; the site then writes sum.
// In scope: smu (the block's rows: mu [C], then theta_1 .. theta_K), RS (a row's doubles), tid, C, data, pr (FitPrior),
// and NP = 1 + K (constexpr): the components with a slot in pr, the signal's in front (k_components_fit: NP = J + K, the
// further signal components' slots with weight 0).
// It leaves behind: sum.
        double sum = 0.0;
        for (int k = 0; k < C; ++k) {
            const double mk = smu[tid * RS + k], dk = data[k];
            double term = mk;
            if (dk != 0.0) {
                const double pl = dk * nm::log_i(mk);
                term = mk - pl;
            }
            sum = sum + term;
        }
#pragma unroll
        for (int j = 1; j < NP; ++j)
            if (pr.w[j] > 0.0) {
                const double dl = smu[tid * RS + C + j - 1] - pr.m[j];
                const double pen = ((0.5 * pr.w[j]) * dl) * dl;
                sum = sum + pen;
            }
