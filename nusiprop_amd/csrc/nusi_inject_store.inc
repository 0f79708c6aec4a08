// One toy's record of k_inject<NC> and k_nuis_inject<NC, MODE> to the call's outputs, behind nusi_toy_body.inc: theta_hat_0
// and the statistic, the two words, the counts (integer atomics).
        if (c == 0 && q < Q) {
            if (o.theta) o.theta[rth + p] = th0;
            if (o.stat) o.stat[rst + p] = stat;
            if (o.words) {
                o.words[(rq * P + p) * 2] = sth;
                o.words[(rq * P + p) * 2 + 1] = st;
            }
            if (o.tally) {
                int* ty = o.tally + rq * 4;
                if (nofit) atomicAdd(ty + 0, 1);
                if (nocond && !nofit) atomicAdd(ty + 1, 1);
                if (sth & (NUSI_FIT_BOUNDARY | NUSI_FIT_FLAT)) atomicAdd(ty + 2, 1);
                if (sth & NUSI_FIT_INFINITE) atomicAdd(ty + 3, 1);
            }
            if (o.exceed && stat >= qobs) atomicAdd(o.exceed + rq, 1);
        }
