// The body of k_cascade_bs and of k_cascade_bs_impulse (nusi_cascade.hip includes it in both: a call to a shared
// __device__ body, inlined, did not compile to the ordinary instances' code).  In scope: the instance's NJ, P, SPL, RT,
// CW, kNR, kImp and kMass, the kernel's arguments g, pts, gidx, grp, t, fh, flux, flux_fla, and ia (ImpulseArgs).
// kImp (the impulse-source instance): column p of the workgroup carries the unit source S = e_n, n = n0 + p, with
// norm = 1: its source term at (step i, bin b) is sig[i] = tabulated_src(step_c[i], 1, w[i], z[i], 1) where b + i = n
// and 0 elsewhere -- no pw[] rows in LDS, no srcb / Src traffic, no pow() prologue; flux / flux_fla may be nullptr.
// kMass (k_cascade_mass_impulse, with kImp): the workgroup's unit sources go into ONE mass state mj, whole (norm = 3:
// no third), and the other two rows get 0.0 -- workgroup k of the launch is (table k / (3 ngrp), state (k / ngrp) % 3,
// bin group k % ngrp), and its columns are written at "point" ((p 3 + mj) (T + 1) + n), the layout G3[p][j][n][3][N].
    extern __shared__ __attribute__((aligned(16))) double lds[];
    using Cfg = BsCfg<NJ, P, SPL, RT, CW>;
    // the power-law sources: formed on the record wave (into srcb, a block ahead) where that is one round of 64 (one
    // point, 16 steps: C3, cascade 24.8 -> 23.7 ms), else in the chain (the record wave's loop of 6 rounds for the
    // gamma batch cost C5 3.25 -> 4.16 ms; at 48 steps its records already fill both phases, C4)
    constexpr bool kSrcRec = 4 * NJ * P <= 64;
    constexpr int LPP = Cfg::LPP, PPW = Cfg::PPW, NC = Cfg::NC, NB = Cfg::NB, NF = kBsFields, S4 = 4 * NJ, NQ = 12 * P;
    const int N = g.N, Nz = g.Nz, T = g.T, nst = Nz - 1;
    // the wave index through readfirstlane: wave-uniform in an SGPR, so every role test and per-wave row base is scalar
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), nw = nthr >> 6;
    // the push waves, the record wave, then the CW chain waves; the push row blocks dealt so that the push waves
    // sharing a SIMD with a chain wave (wave w on SIMD w % 4) hold the top rows, which the wavefront consumes first
    // (fewest MFMAs)
    const int recw = nw - 1 - CW, chw = nw - CW;
    const bool is_chain = wave >= chw, is_rec = wave == recw;
    NUSI_WS_HWID();
    // kImp: the workgroup's first source-axis bin n0; its table's point and its columns n0 .. min(T, n0 + P - 1)
    const int ing = kImp ? ia.ngrp : 1;
    const int in0 = kImp ? 1 + P * ((int)blockIdx.x % ing) : 0;
    const int itj = (int)blockIdx.x / ing;    // kMass: 3 (table of the launch) + source state
    const int mj = kMass ? itj % 3 : 0;       // kMass: the mass state that takes the source (wave-uniform)
    const int2 gr = kImp ? make_int2(ia.p0 + (kMass ? itj / 3 : itj), min(P, T + 1 - in0))
                         : grp ? grp[blockIdx.x] : make_int2((int)blockIdx.x, 1);
    const int R = gr.y;                                   // points of this workgroup (<= P), one table
    auto pidx = [&](int p) {                              // (gidx == nullptr: point blockIdx.x; kImp: the table's point)
        if constexpr (kImp) return gr.x;
        else return gidx ? gidx[gr.x + p] : gr.x + p;
    };
    const Point& P0 = pts[pidx(0)];
    double* rec = lds;                       // [2][NF][4][NJ]  records of block q in slot q & 1
    double* srcb = rec + 2 * NF * S4;        // [2][4][NJ][P]   block q's DSNB sources c_i Lum (stage, step, point)
    double* Tp = srcb + 8 * NC;              // [8][NC]         T_j of each column by stage
    double* AX = Tp + 8 * NC;                // [2][4][NC]      rows published by block q (parity q & 1)
    double* fqb = AX + 8 * NC;               // [2][4][3][P]    the previous pass' last step, F[:, N-1-sg], block q
    double* fin = fqb + 2 * NQ;              // [2][4][3][P]    the last pass' output F[:, b] of block q's stages (to finalise)
    double* pinf = fin + 2 * NQ;             // [13][P]         per point: a3, rs, power law (1) / DSNB (0), index, U2[9]
    double* rdE = pinf + 13 * P;             // [N]
    double* pw = rdE + N;                    // [P][T + 2]      each power-law point's pw on table edge e
    double* sGt = pw + (kImp ? 0 : (size_t)P * (T + 2));   // (kImp: no pw rows)
    double* sAt = sGt + T;
    double* sdg = sAt + T;                   // [4][T]: alpha(n, n+k), k = 1..4 (0 past the table)
    double* sEmin = sdg + 4 * T;
    double* sEmax = sEmin + N;
    double* sgz = sEmax + N;                 // z, step_c, step_s, sfr [Nz each]
    double* sig = sgz + 4 * Nz;              // [Nz]            kImp only: the unit source term of each step
    GridDev gl = g;
    gl.Emin = sEmin;
    gl.Emax = sEmax;
    gl.z = sgz;
    gl.step_c = sgz + Nz;
    gl.step_s = sgz + 2 * Nz;
    gl.sfr = sgz + 3 * Nz;
    const double* __restrict__ Al = t.A + (size_t)P0.tslot * g.PT;
    {
        const double* __restrict__ Gt = t.G + (size_t)P0.tslot * T;
        const double* __restrict__ At = t.At + (size_t)P0.tslot * T;
        for (int n = tid; n < T; n += nthr) {
            sGt[n] = Gt[n];
            sAt[n] = At[n];
#pragma unroll
            for (int k = 1; k <= 4; ++k) sdg[(k - 1) * T + n] = (n + k < T) ? Al[(size_t)(n + k) * (n + k - 1) / 2 + n] : 0.0;
        }
        for (int b = tid; b < N; b += nthr) {
            sEmin[b] = g.Emin[b];
            sEmax[b] = g.Emax[b];
            rdE[b] = 1.0 / (g.Emax[b] - g.Emin[b]);   // cascade_aux_init's expression
        }
        for (int i = tid; i < Nz; i += nthr) {
            sgz[i] = g.z[i];
            sgz[Nz + i] = g.step_c[i];
            sgz[2 * Nz + i] = g.step_s[i];
            sgz[3 * Nz + i] = g.sfr[i];
        }
        if constexpr (kImp) {
            for (int p = tid; p < P; p += nthr) {   // no source factors, not the DSNB; the column's output index
                pinf[p] = pinf[P + p] = 0.0;
                pinf[2 * P + p] = 1.0;
                pinf[3 * P + p] = (double)((kMass ? gr.x * 3 + mj : gr.x) * (T + 1) + in0 + p);
#pragma unroll
                for (int f = 0; f < 9; ++f) pinf[(4 + f) * P + p] = P0.U2[f];
            }
            for (int i = tid; i < Nz; i += nthr)
                sig[i] = i ? tabulated_src(g.step_c[i], kMass ? 3.0 : 1.0, ia.w[i], g.z[i], 1.0) : 0.0;
        } else {
        for (int p = tid; p < P; p += nthr) {   // the points' source factors (src_factors), kind and index
            const int pid = p < R ? pidx(p) : 0;
            const SrcFactors f = src_factors(pts[pid]);
            pinf[p] = f.a3;
            pinf[P + p] = f.rs;
            pinf[2 * P + p] = p < R && pts[pid].source == NUSI_SOURCE_POWER_LAW ? 1.0 : 0.0;
            pinf[3 * P + p] = (double)pid;
#pragma unroll
            for (int f = 0; f < 9; ++f) pinf[(4 + f) * P + p] = pts[pid].U2[f];   // the finalise's, off the chain's global path
        }
        for (int q = tid; q < P * (T + 1); q += nthr) {   // cascade_aux_init's pw[e] of every power-law point
            const int p = q / (T + 1), e = 1 + q - p * (T + 1);
            if (p >= R) continue;
            const Point& Q = pts[pidx(p)];
            if (Q.source != NUSI_SOURCE_POWER_LAW) continue;
            const int i = min(Nz - 1, max(1, e - N + 1)), b = e - i;
            const double E = (b < N) ? g.Emin[b] : g.Emax[N - 1];
            pw[(size_t)p * (T + 2) + e] = nm::pow(E / 1e14 * (1 + g.z[i]), -Q.si);
        }
        }   // !kImp
    }
    const bool nonres = kNR || P0.non_resonant;   // the points of a workgroup share a table, hence the flags
    const int npass = (nst + NJ - 1) / NJ;
    double* const fhw = fh + (size_t)blockIdx.x * 3 * N * P;   // this workgroup's F FIFO [3][N][P] (passes > 1)
    int jb = 0, njp = 0, Ts = 0, c0 = 0, nblk = 0;
    auto pass_geom = [&](int pass) {
        jb = pass * NJ;
        njp = nst - jb < NJ ? nst - jb : NJ;   // steps of this pass
        Ts = N - 1 + njp;                      // its stages
        c0 = T - 1 - jb;                       // the table column of its stage 0
        nblk = (Ts + 3) / 4;
    };
    if (is_chain) {
        // ---- chain wave cw: lane (cp, cjp) solves step slot j = cjp of point cp (PPW points per wave, so a point's
        // steps never cross waves).  A stage is split into its loads (records, source operands, published row,
        // diagonal alphas: none depends on the previous stage's solve) and its solve, and the loads of stage d + 1
        // are issued before the solve of stage d, so one LDS latency per stage is hidden behind the dependent
        // solve.  The power-law sources are formed here (powerlaw_src_h), the DSNB ones read from srcb; the
        // finalise of the last pass goes to the record wave through `fin`
        __builtin_amdgcn_s_setprio(3);   // the chain's instructions (and LDS requests) before the push waves'
        const int cw = wave - chw;
        const int cp = cw * PPW + lane / LPP, cjp = lane - LPP * (lane / LPP);
        const bool clane = lane < PPW * LPP && cp < R;
        const double u0 = P0.u[0], u1 = P0.u[1], u2 = P0.u[2];
        const int cpc = cp < P ? cp : P - 1;
        const double* const cpw = pw + (size_t)cpc * (T + 2);
        struct StageIn {
            double rz0, rz1, rz2, l10, l20, l21, u01, u02, u12, ru00, ru11, ru22, sde, src, cj, ab, sd[4], fq0, fq1, fq2;
            double ss, dEb1;   // the resonant-only running sum's step_s and dE of the bin above
            int pmb;
        };
#pragma unroll 1
        for (int pass = 0; pass < npass; ++pass) {
            pass_geom(pass);
            const bool last_pass = pass == npass - 1;
            __syncthreads();   // the previous pass is done with Tp, AX and the records (pass 0: the prologue's LDS)
            for (int q = lane; q < 16 * NC; q += 64) Tp[q] = 0.0;   // Tp and AX
            const bool cpl = pinf[2 * P + cpc] != 0.0;
            const SrcFactors csf{pinf[cpc], pinf[P + cpc]};
            __syncthreads();
            double px0 = 0.0, px1 = 0.0, px2 = 0.0, racc = 0.0, Th[4] = {0.0, 0.0, 0.0, 0.0};
            const int j = cjp, i = Nz - 1 - jb - j;
            const int ic = i < 1 ? 1 : i;   // (lanes past the pass' steps read in range and are masked)
            // stage sg = 4 q + d of the pass: its loads
            auto load = [&](int q, int d) {
                const int sg = 4 * q + d, r = c0 - sg;
                const int b = N - 1 - sg + j, bc = b < 0 ? 0 : (b > N - 1 ? N - 1 : b);
                const int rc = r < 0 ? 0 : r;
                const double* Rc = rec + (size_t)(q & 1) * NF * S4 + d * NJ + j;
                StageIn in;
                in.rz0 = Rc[BR_RZ0 * S4]; in.rz1 = Rc[BR_RZ1 * S4]; in.rz2 = Rc[BR_RZ2 * S4];
                in.pmb = (int)Rc[BR_PERM * S4];
                in.l10 = Rc[BR_L10 * S4]; in.l20 = Rc[BR_L20 * S4]; in.l21 = Rc[BR_L21 * S4];
                in.u01 = Rc[BR_U01 * S4]; in.u02 = Rc[BR_U02 * S4]; in.u12 = Rc[BR_U12 * S4];
                in.ru00 = Rc[BR_RU00 * S4]; in.ru11 = Rc[BR_RU11 * S4]; in.ru22 = Rc[BR_RU22 * S4];
                in.sde = Rc[BR_SDE * S4];
                if constexpr (kImp) {   // the unit impulse of column cp: bin b + i of the source axis is its own
                    in.src = (b + i == in0 + cp) ? sig[ic] : 0.0;
                } else {
                const double sdn = srcb[(q & 1) * 4 * NC + d * NC + j * P + cpc];
                if (kSrcRec) {   // the record wave formed every source
                    in.src = sdn;
                } else {         // both, selected branch-free (a branch here made the compiler wait for every LDS load)
                    const double spw = powerlaw_src_h(gl, csf, cpw, ic, bc);
                    in.src = cpl ? spw : sdn;
                }
                }
                in.cj = gl.step_c[ic];
                const int qq = (sg - 1) >> 2;   // block whose publication serves stage sg
                in.ab = AX[((qq & 1) * 4 + (sg - 1 - 4 * qq)) * NC + j * P + cpc];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) in.sd[kk] = sdg[kk * T + rc];
                const double* fq = fqb + (q & 1) * NQ + d * 3 * P + cpc;
                in.fq0 = fq[0]; in.fq1 = fq[P]; in.fq2 = fq[2 * P];
                if (!nonres) {
                    in.ss = gl.step_s[ic];
                    in.dEb1 = (bc + 1 < N) ? sEmax[bc + 1] - sEmin[bc + 1] : 1.0;
                } else {
                    in.ss = in.dEb1 = 0.0;
                }
                return in;
            };
            // ... and its solve
            auto solve = [&](int q, int d, const StageIn& in) {
                const int sg = 4 * q + d;
                const int b = N - 1 - sg + j;
                const int nu = (d == 0) ? 4 : d;   // columns r+1 .. r+nu not yet pushed
                double f0 = wave_shr1(px0, 0.0), f1 = wave_shr1(px1, 0.0), f2 = wave_shr1(px2, 0.0);   // every lane active
                if (cjp == 0) {   // the first step: the previous pass' last step (fqb, staged by the record wave), or 0
                    f0 = in.fq0;
                    f1 = in.fq1;
                    f2 = in.fq2;
                }
                double Tn = 0.0;
                if (clane && j < njp && b >= 0 && b < N) {
                    double add;
                    if (nonres) {
                        double sa = in.ab;
#pragma unroll
                        for (int kk = 4; kk >= 1; --kk)
                            if (kk <= nu) sa = fma(in.sd[kk - 1], Th[kk - 1], sa);
                        add = in.cj * sa;
                    } else {
                        add = resonant_add(racc, u0, u1, u2, px0, px1, px2, in.ss, in.sd[0], in.dEb1, in.sde, in.cj,
                                           b == N - 1);
                    }
                    double x0, x1, x2;
                    if constexpr (kMass) {   // the source per row: the unit source in row mj, 0.0 in the others
                        const double s0 = mj == 0 ? in.src : 0.0, s1 = mj == 1 ? in.src : 0.0, s2 = mj == 2 ? in.src : 0.0;
                        if (__all(in.pmb == kIdPerm))
                            cascade_solve3_id(f0, f1, f2, add, s0, s1, s2, u0, u1, u2, in.rz0, in.rz1, in.rz2, in.l10,
                                              in.l20, in.l21, in.u01, in.u02, in.u12, in.ru11, in.ru22, x0, x1, x2);
                        else
                            cascade_solve3(f0, f1, f2, add, s0, s1, s2, u0, u1, u2, in.rz0, in.rz1, in.rz2, in.pmb,
                                           in.l10, in.l20, in.l21, in.u01, in.u02, in.u12, in.ru00, in.ru11, in.ru22, x0,
                                           x1, x2);
                    } else
                    if (__all(in.pmb == kIdPerm))   // (every active lane: no row exchange -- always, in practice)
                        cascade_solve_id(f0, f1, f2, add, in.src, u0, u1, u2, in.rz0, in.rz1, in.rz2, in.l10, in.l20,
                                         in.l21, in.u01, in.u02, in.u12, in.ru11, in.ru22, x0, x1, x2);
                    else
                        cascade_solve(f0, f1, f2, add, in.src, u0, u1, u2, in.rz0, in.rz1, in.rz2, in.pmb, in.l10,
                                      in.l20, in.l21, in.u01, in.u02, in.u12, in.ru00, in.ru11, in.ru22, x0, x1, x2);
                    if (j == njp - 1) {   // the pass's last step: the output (the record wave finalises it), or the next pass' input
                        if (last_pass) {
                            double* fo = fin + (((q & 1) * 4 + d) * 3) * P + cp;
                            fo[0] = x0;
                            fo[P] = x1;
                            fo[2 * P] = x2;
                        } else {
                            fhw[((size_t)0 * N + b) * P + cp] = x0;
                            fhw[((size_t)1 * N + b) * P + cp] = x1;
                            fhw[((size_t)2 * N + b) * P + cp] = x2;
                        }
                    }
                    px0 = x0; px1 = x1; px2 = x2;
                    if (nonres && b > 0) Tn = (u0 * x0 + u1 * x1 + u2 * x2) * in.sde;
                }
                Th[3] = Th[2]; Th[2] = Th[1]; Th[1] = Th[0]; Th[0] = Tn;
                if (clane && j < njp) Tp[(sg & 7) * NC + j * P + cp] = Tn;
            };
#pragma unroll 1
            for (int q = 0; q < nblk; ++q) {
                NUSI_BS_STAMP(pass * nblk + q, 0);
                if (4 * q < Ts) solve(q, 0, load(q, 0));           // phase A
                NUSI_BS_STAMP(pass * nblk + q, 1);
                __syncthreads();
                NUSI_BS_STAMP(pass * nblk + q, 2);
#pragma unroll
                for (int d = 1; d < 4; ++d)                          // phase B
                    if (4 * q + d < Ts) {
                        const StageIn in = load(q, d);
                        if (d < 3 && cw == 0) NUSI_BS_CSTAMP(pass * nblk + q, 2 * (d - 1));
                        solve(q, d, in);
                        if (d < 3 && cw == 0) NUSI_BS_CSTAMP(pass * nblk + q, 2 * (d - 1) + 1);
                    }
                NUSI_BS_STAMP(pass * nblk + q, 3);
                __syncthreads();
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the FIFO stores land before the next pass reads them
        }
    } else if (is_rec) {
        __builtin_amdgcn_s_setprio(3);
        // ---- records and DSNB sources: block 0 (and the FIFO of blocks 0, 1) before the blocks; in block q the
        // records of block q + 1 (block q + 1's slot was last read in block q - 1): one round of 64 lanes goes wholly
        // into phase B, where the chain solves three stages (C5 / C3: phase A then waits on the chain alone); of
        // three rounds (48 steps) the first goes into phase A; the DSNB sources into phase B.  The FIFO values of
        // block q + 2 are loaded in phase A of block q and stored in phase A of block q + 1
        constexpr int kRecRounds = (S4 + 63) / 64, kRecA = kRecRounds <= 1 ? 0 : (kRecRounds + 2) / 3;
        constexpr int kRecSplit = 64 * kRecA < S4 ? 64 * kRecA : S4;
        auto records = [&](int qb, int e0, int e1) {
            for (int e = e0 + lane; e < e1; e += 64) {
                const int sb = e / NJ, jj = e - NJ * (e / NJ), s2 = 4 * qb + sb;
                const int b = N - 1 - s2 + jj, i = Nz - 1 - jb - jj;
                if (jj < njp && s2 < Ts && b >= 0 && b < N) {
                    double* Rw = rec + (size_t)(qb & 1) * NF * S4 + e;
                    const RecM m = record_phase1(gl, P0, sGt, sAt, rdE, i, b);
                    Rw[BR_RZ0 * S4] = m.rz0;
                    Rw[BR_RZ1 * S4] = m.rz1;
                    Rw[BR_RZ2 * S4] = m.rz2;
                    Rw[BR_SDE * S4] = nonres ? gl.step_s[i] * rdE[b] : (gl.Emax[b] - gl.Emin[b]);
                    record_phase2<true>(m, Rw - S4, S4);   // (PR_L10 .. PR_RU22, the permutation: BR_* = PR_* - 1)
                }
            }
        };
        bool any_dsnb = false;   // (set after the first barrier: the prologue writes pinf)
        auto sources = [&](int qb) {   // the DSNB points' (k_source_dsnb's table); with kSrcRec the power-law ones too
            if (kImp || (!kSrcRec && !any_dsnb)) return;
            for (int e = lane; e < S4 * P; e += 64) {
                const int p = e % P, sj = e / P, sb = sj / NJ, jj = sj - NJ * sb, s2 = 4 * qb + sb;
                const int b = N - 1 - s2 + jj, i = Nz - 1 - jb - jj;
                if (p < R && jj < njp && s2 < Ts && b >= 0 && b < N) {
                    if (pinf[2 * P + p] == 0.0)
                        srcb[(qb & 1) * 4 * NC + e] = t.Src[(size_t)pinf[3 * P + p] * T * nst + src_index(Nz, jb + jj, b)];
                    else if (kSrcRec)
                        srcb[(qb & 1) * 4 * NC + e] =
                            powerlaw_src_h(gl, SrcFactors{pinf[p], pinf[P + p]}, pw + (size_t)p * (T + 2), i, b);
                }
            }
        };
        // The DSNB sources of block qb from k_source_dsnb's table a block ahead (src_load into registers in phase B of
        // block qb - 2, src_store into srcb in phase B of block qb - 1): the table's latency off the record wave's path
        // (sources() loaded and stored them within one phase B: C2a's cascade 0.295 against C2b's 0.176 ms).  The same
        // values in the same places.
        constexpr bool kAhead = P == 1 && RT == 4;   // (one point, one pass shape: the others' registers)
        constexpr int SQL = (S4 * P + 63) / 64;
        auto src_valid = [&](int qb, int e, int& p, int& b, int& i) {
            p = e % P;
            const int sj = e / P, sb = sj / NJ, jj = sj - NJ * sb, s2 = 4 * qb + sb;
            b = N - 1 - s2 + jj;
            i = Nz - 1 - jb - jj;
            return e < S4 * P && p < R && jj < njp && s2 < Ts && b >= 0 && b < N;
        };
        auto src_load = [&](int qb, double (&v)[SQL]) {
            if (!any_dsnb) return;
#pragma unroll
            for (int u = 0; u < SQL; ++u) {
                int p, b, i;
                const int e = lane + 64 * u;
                v[u] = (src_valid(qb, e, p, b, i) && pinf[2 * P + p] == 0.0)
                           ? t.Src[(size_t)pinf[3 * P + p] * T * nst + src_index(Nz, jb + (e / P) % NJ, b)] : 0.0;
            }
        };
        auto src_store = [&](int qb, const double (&v)[SQL]) {
            if (!kSrcRec && !any_dsnb) return;
#pragma unroll
            for (int u = 0; u < SQL; ++u) {
                int p, b, i;
                const int e = lane + 64 * u;
                if (src_valid(qb, e, p, b, i)) {
                    if (pinf[2 * P + p] == 0.0)
                        srcb[(qb & 1) * 4 * NC + e] = v[u];
                    else if (kSrcRec)
                        srcb[(qb & 1) * 4 * NC + e] =
                            powerlaw_src_h(gl, SrcFactors{pinf[p], pinf[P + p]}, pw + (size_t)p * (T + 2), i, b);
                }
            }
        };
        auto finalise = [&](int qb) {   // the last pass' stages of block qb (nuSIprop.hpp:328-336)
            for (int e = lane; e < 4 * P; e += 64) {
                const int d = e / P, p = e - P * (e / P), sg = 4 * qb + d, b = N - 1 - sg + njp - 1;
                if (p < R && sg < Ts && b >= 0 && b < N) {
                    const double* fo = fin + (((qb & 1) * 4 + d) * 3) * P + p;
                    const int cpid = (int)pinf[3 * P + p];
                    const double* U2 = pinf + 4 * P + p;
                    const double dE = gl.Emax[b] - gl.Emin[b];
                    const double g0 = fo[0] / dE, g1 = fo[P] / dE, g2 = fo[2 * P] / dE;
                    double* fx = flux + (size_t)cpid * 3 * N;
                    double* fl = flux_fla + (size_t)cpid * 3 * N;
                    if (!kImp || flux) {
                        fx[b] = g0;
                        fx[N + b] = g1;
                        fx[2 * N + b] = g2;
                    }
                    if (!kImp || flux_fla)
                        for (int f = 0; f < 3; ++f)
                            fl[f * N + b] = U2[(3 * f + 0) * P] * g0 + U2[(3 * f + 1) * P] * g1 + U2[(3 * f + 2) * P] * g2;
                }
            }
        };
        constexpr int FQL = (NQ + 63) / 64;   // FIFO values per lane and block
        auto fifo_load = [&](int pass, int qb, double (&v)[FQL]) {
#pragma unroll
            for (int u = 0; u < FQL; ++u) {
                const int e = lane + 64 * u, d = e / (3 * P), c = (e / P) % 3, p = e % P, sg = 4 * qb + d, bq = N - 1 - sg;
                v[u] = (pass > 0 && e < NQ && sg < Ts && bq >= 0)
                           ? __builtin_nontemporal_load(fhw + ((size_t)c * N + bq) * P + p) : 0.0;
            }
        };
        auto fifo_store = [&](int qb, const double (&v)[FQL]) {
#pragma unroll
            for (int u = 0; u < FQL; ++u)
                if (lane + 64 * u < NQ) fqb[(qb & 1) * NQ + lane + 64 * u] = v[u];
        };
#pragma unroll 1
        for (int pass = 0; pass < npass; ++pass) {
            pass_geom(pass);
            __syncthreads();
            any_dsnb = false;
            for (int p = 0; p < R; ++p) any_dsnb = any_dsnb || pinf[2 * P + p] == 0.0;
            records(0, 0, S4);
            sources(0);
            double sv[SQL];
            if (kAhead) src_load(1, sv);
            double fv[FQL];
            fifo_load(pass, 0, fv);
            fifo_store(0, fv);
            fifo_load(pass, 1, fv);
            __syncthreads();
#pragma unroll 1
            for (int q = 0; q < nblk; ++q) {
                NUSI_BS_STAMP(pass * nblk + q, 0);
                fifo_store(q + 1, fv);                  // block q + 1's FIFO values (loaded a block ago)
                fifo_load(pass, q + 2, fv);
                if (4 * (q + 1) < Ts) records(q + 1, 0, kRecSplit);   // phase A
                NUSI_BS_STAMP(pass * nblk + q, 1);
                __syncthreads();
                NUSI_BS_STAMP(pass * nblk + q, 2);
                if (4 * (q + 1) < Ts) {                                // phase B
                    records(q + 1, kRecSplit, S4);
                    if (kAhead) {
                        src_store(q + 1, sv);           // block q + 1's sources (loaded a block ago)
                        if (4 * (q + 2) < Ts) src_load(q + 2, sv);
                    } else
                        sources(q + 1);
                }
                if (pass == npass - 1 && q > 0) finalise(q - 1);
                NUSI_BS_STAMP(pass * nblk + q, 3);
                __syncthreads();
            }
            if (pass == npass - 1) finalise(nblk - 1);   // (after the loop's last barrier: the chain's last block is in fin)
        }
    } else {
        // ---- push: block q adds columns c0+1-4q .. c0+4-4q (the T of stages 4q-1 .. 4q-4) into the rows below
        // r = c0-4q: in phase A the tiles holding rows r-1 .. r-4 (published to AX), in phase B the others
        int rb = 0;   // this push wave's row block: the waves sharing no SIMD with a chain or the record wave take the
        {             // bottom rows (busiest), then those beside the record wave, then those beside a chain wave
            const int npush = nw - 1 - CW;
            auto cls = [&](int w) {
                for (int c = chw; c < nw; ++c)
                    if ((c & 3) == (w & 3)) return 2;
                return (recw & 3) == (w & 3) ? 1 : 0;
            };
            const int mine = cls(wave);
            for (int w = 0; w < npush; ++w) {
                const int o = cls(w);
                if (o < mine || (o == mine && w < wave)) ++rb;
            }
        }
        const int rw0 = rb * 16 * RT;
#pragma unroll 1
        for (int pass = 0; pass < npass; ++pass) {
            pass_geom(pass);
            __syncthreads();
            __syncthreads();
            nusi_f64x4 acc[RT][NB];
#pragma unroll
            for (int a = 0; a < RT; ++a)
#pragma unroll
                for (int s = 0; s < NB; ++s) acc[a][s] = nusi_f64x4{0.0, 0.0, 0.0, 0.0};
            auto load_blk = [&](int q, double (&dst)[RT]) {
                int c = c0 + 1 - 4 * q + (lane >> 4);
                c = c < 1 ? 1 : (c > T - 1 ? T - 1 : c);
                const size_t cb = (size_t)c * (c - 1) / 2;
#pragma unroll
                for (int a = 0; a < RT; ++a) {
                    const int row = rw0 + 16 * a + (lane & 15);
                    dst[a] = Al[cb + (row < c - 1 ? row : c - 1)];
                }
            };
            auto push = [&](int q, const double (&ab)[RT], bool phase_a) {
                const int r = c0 - 4 * q, hi = r - 1;
                const double* Tq = Tp + ((4 * q - 1 - (lane >> 4)) & 7) * NC + (lane & 15);
#pragma unroll
                for (int a = 0; a < RT; ++a) {
                    const bool crit = rw0 + 16 * a <= hi && rw0 + 16 * a + 15 >= hi - 3;   // uniform
                    if (crit == phase_a && rw0 + 16 * a < r)   // tiles wholly at or above r hold consumed rows only
#pragma unroll
                        for (int s = 0; s < NB; ++s)
                            acc[a][s] = __builtin_amdgcn_mfma_f64_16x16x4f64(ab[a], Tq[16 * s], acc[a][s], 0, 0, 0);
                }
                if (phase_a)
#pragma unroll
                    for (int a = 0; a < RT; ++a)
                        if (rw0 + 16 * a <= hi && rw0 + 16 * a + 15 >= hi - 3)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                const int row = rw0 + 16 * a + (lane >> 4) + 4 * e;
                                const int slot = hi - row;
                                if (slot >= 0 && slot < 4)
#pragma unroll
                                    for (int s = 0; s < NB; ++s)
                                        AX[((q & 1) * 4 + slot) * NC + 16 * s + (lane & 15)] = acc[a][s][e];
                            }
            };
            auto block = [&](int q, double (&ab)[RT]) {   // ab holds block q's A operands; then block q + 2's
                const bool doq = nonres && q >= 1 && 4 * q < Ts;
                NUSI_BS_STAMP(pass * nblk + q, 0);
                if (doq) push(q, ab, true);
                NUSI_BS_STAMP(pass * nblk + q, 1);
                __syncthreads();
                NUSI_BS_STAMP(pass * nblk + q, 2);
                if (doq) push(q, ab, false);
                load_blk(q + 2, ab);
                NUSI_BS_STAMP(pass * nblk + q, 3);
                __syncthreads();
            };
            double ab0[RT], ab1[RT];
            load_blk(0, ab0);
            load_blk(1, ab1);
#pragma unroll 1
            for (int q = 0; q < nblk; q += 2) {
                block(q, ab0);
                if (q + 1 < nblk) block(q + 1, ab1);
            }
        }
    }
