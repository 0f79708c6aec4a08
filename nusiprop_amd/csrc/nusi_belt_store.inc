// One pass's record of k_belt<NC> and k_nuis_belt<NC>, behind nusi_toy_body.inc: the observed pass sets valid, qobs and
// mu_inj and (slice 0) stores the observed side; a toy's pass stores its raw record and adds to the counts.
        if (obs) {
            valid = agood && !nofit && !nocond;
            qobs = valid ? stat : __builtin_nan("");
            mu_inj = valid ? mu : 0.0;
            if (c == 0 && mine && blockIdx.z == 0) {
                const size_t ro = (size_t)pair * (1 + G);
                if (gp == 0) {
                    if (o.thobs) {
#pragma unroll
                        for (int j = 0; j < NC; ++j) o.thobs[ro * NC + j] = thh[j];
                    }
                    if (o.wobs) o.wobs[(size_t)(pair - (o.wobs_compact ? ii.pr0 : 0)) * (1 + G)] = sth;
                }
                if (o.thobs) {
                    o.thobs[(ro + 1 + gp) * NC] = agood ? atest : __builtin_nan("");
#pragma unroll
                    for (int j = 0; j < KT; ++j) o.thobs[(ro + 1 + gp) * NC + 1 + j] = agood ? th[j] : __builtin_nan("");
                }
                if (o.wobs) o.wobs[(size_t)(pair - (o.wobs_compact ? ii.pr0 : 0)) * (1 + G) + 1 + gp] = agood ? st : 0;
                if (o.qobs) o.qobs[rg] = qobs;
            }
        } else if (c == 0 && mine) {
            if (o.theta) o.theta[rg * P + p] = valid ? th0 : __builtin_nan("");
            if (o.stat) o.stat[rg * P + p] = valid ? stat : __builtin_nan("");
            if (o.words) {
                o.words[(rg * P + p) * 2] = valid ? sth : 0;
                o.words[(rg * P + p) * 2 + 1] = valid ? st : 0;
            }
            if (o.tally && valid) {
                int* ty = o.tally + ((size_t)(pair - (o.tally_compact ? ii.pr0 : 0)) * G + gp) * 4;
                if (nofit) atomicAdd(ty + 0, 1);
                if (nocond && !nofit) atomicAdd(ty + 1, 1);
                if (sth & (NUSI_FIT_BOUNDARY | NUSI_FIT_FLAT)) atomicAdd(ty + 2, 1);
                if (sth & NUSI_FIT_INFINITE) atomicAdd(ty + 3, 1);
            }
            if (o.exceed && valid && stat >= qobs)
                atomicAdd(o.exceed + (size_t)(pair - (o.exceed_compact ? ii.pr0 : 0)) * G + gp, 1);
        }
