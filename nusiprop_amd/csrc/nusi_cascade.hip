// nuSIprop MI355X -- Stage B: the implicit redshift cascade + finalisation
// (calculate_flux::evolve, nuSIprop.hpp:255-336).
//
//   k_cascade_bs<NJ, P, SPL, RT, CW, kNR>  the wavefront with its push on the fp64 matrix cores, block-synchronous
//                         roles; one point, two or up to 16 points sharing a table per workgroup, step passes on
//                         long grids (NUSI_CASCADE_AUTO / MFMA, every shape)
//   k_cascade_bs_impulse  its impulse-source instance: 16 source-axis bins of a table per workgroup, the response
//                         matrix of nusi_plan_response (both kernels include nusi_cascade_bs_body.inc)
//   k_cascade_mass_impulse  ... with the unit source in one mass state per workgroup: the mass-resolved response of
//                         nusi_plan_response_mass (the third kernel that includes the body)
//   k_response_apply      spectra on resident response matrices (nusi_plan_response_apply)
//   k_response_compose    a source's flavour composition on mass-resolved rows (nusi_plan_response_compose)
//   k_source_dsnb         the DSNB source terms it reads
//   k_source_tab          ... and the tabulated sources' (nusi_plan_set_source)
//   k_cascade             the bit-exact scalar cascade, one wavefront per point, any N (NUSI_CASCADE_WAVEFRONT /
//                         REG / LDS).  (The per-stage kernels of rounds 1-3 -- k_cascade_wf, _reg, _ws, _wsp, _gb --
//                         are gone; DESIGN.md Appendix A keeps their measurements.)
//   k_cascade_mass        its copy with the source per mass state (nusi_plan_response_mass's scalar fallback)
#include <hip/hip_runtime.h>

#include <utility>

#include "nusi_internal.hpp"

namespace nusi {
// ---------------------------------------------------------------------------
// Stage B -- the cascade.
//
// For each redshift step i (sequential, z_max -> 0) the bins are swept from
// the top down; bin b needs the already-updated bins m > b of the same step
// (nuSIprop.hpp:289-291), i.e. an upper-triangular solve.  It is done
// right-looking: as soon as bin b is final, its weight
//     T_b = s_i * sum_l u_l F_l[b] / dE_b
// is pushed into every lower bin's accumulator acc[b'] += alpha(b', b) T_b
// (one coalesced column read of the packed transposed table per bin), so the
// sequential chain per bin is only the 3x3 solve.  Everything that does not
// depend on the flux (Zdr, the LU of M, the source term) is precomputed for
// 64 bins at a time, one bin per lane, into LDS.
//
// One wavefront (64 lanes) per point; F[3][N] and acc[N] live in LDS.
// ---------------------------------------------------------------------------
constexpr int kPreFields = 14;
enum { PR_RZ0, PR_RZ1, PR_RZ2, PR_SRC, PR_L10, PR_L20, PR_L21, PR_U01, PR_U02, PR_U12, PR_RU00, PR_RU11, PR_RU22, PR_SDE };

size_t cascade_lds_bytes(int N) { return sizeof(double) * (4 * (size_t)N + kPreFields * 64) + sizeof(int) * 64; }

// gsl_linalg_LU_decomp on 3x3 (partial pivoting, Doolittle), nuSIprop.hpp:309
NUSI_FN void lu3_factor(double A[3][3], int perm[3])
{
    perm[0] = 0; perm[1] = 1; perm[2] = 2;
    for (int j = 0; j < 2; ++j) {
        double amax = fabs(A[j][j]);
        int ip = j;
        for (int i = j + 1; i < 3; ++i)
            if (fabs(A[i][j]) > amax) { amax = fabs(A[i][j]); ip = i; }
        if (ip != j) {
            for (int c = 0; c < 3; ++c) { const double t = A[j][c]; A[j][c] = A[ip][c]; A[ip][c] = t; }
            const int t = perm[j]; perm[j] = perm[ip]; perm[ip] = t;
        }
        const double ajj = A[j][j];
        if (ajj != 0.0)
            for (int i = j + 1; i < 3; ++i) {
                const double aij = A[i][j] / ajj;
                A[i][j] = aij;
                for (int c = j + 1; c < 3; ++c) A[i][c] = A[i][c] - aij * A[j][c];
            }
    }
}

// Per-point tables shared by the records of every (step, bin) (LDS; cascade_aux_init):
//   rdE[b] = 1 / dE_b                                                           [N]
//   pw[e]  = pow(E_e / E0 * (1 + z_i), -si) on table edge e = b + i (lower edge of bin b at
//            step i; the upper edge is e + 1), power-law source only            [T + 2]
// Along e the argument depends on b + i only (E_b (1 + z_i) = E_{b+i}, the index-shift
// identity), so 2 (Nz-1) N pow() calls per point become T + 1.  pw[e] is evaluated at one
// (b, i) of its edge; the other pairs' arguments differ from it by rounding only (<= 2 ulp).
constexpr int kAuxDoubles = 2;   // cascade_aux_doubles(N, T) = N + T + kAuxDoubles
NUSI_FN int cascade_aux_doubles(int N, int T) { return N + T + kAuxDoubles; }
__device__ inline void cascade_aux_init(const GridDev& g, const Point& P, double* rdE, double* pw, int tid, int nthr)
{
    const int N = g.N, Nz = g.Nz, T = g.T;
    for (int b = tid; b < N; b += nthr) rdE[b] = 1.0 / (g.Emax[b] - g.Emin[b]);
    if (P.source == 1)
        for (int e = tid + 1; e <= T + 1; e += nthr) {
            const int i = min(Nz - 1, max(1, e - N + 1)), b = e - i;
            const double E = (b < N) ? g.Emin[b] : g.Emax[N - 1];
            pw[e] = nm::pow(E / 1e14 * (1 + g.z[i]), -P.si);
        }
}

// the DSNB source, out of line: it is not the scans' source and inlined it would cost every
// record's caller registers
__device__ __attribute__((noinline)) double lum_out(const Point& P, double z, double sfr_z, double Em, double Ep)
{
    return lum(P, z, sfr_z, Em, Ep);
}

// flux-independent fields of bin b at step i (every PR_* field, the LU permutation in R[kPreFields]):
// Zdr, M = I + offdiag and its LU (nuSIprop.hpp:289-310) and the source term c_i Lum (:283).
// 1/dE_b and 1/Zdr are multiplied in (the reference divides; M's off-diagonals are ~1e-22 of
// the diagonal), the power-law source reads pw[]; the DSNB source is evaluated in full.

// 1/x to about an ulp: the hardware reciprocal estimate (v_rcp_f64) refined by two Newton steps.  The
// records' divisions use it (a correctly rounded fp64 division is a ~10-instruction dependent chain);
// the reference divides, so the fluxes move by rounding only (tests: FLUX_RTOL against the oracle).
NUSI_FN double rcp_nr(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = fma(-x, r, 1.0);
    r = fma(r, e, r);
    e = fma(-x, r, 1.0);
    return fma(r, e, r);
}

// The record of (step i, bin b) in two phases (k_cascade_bs runs them on different waves; cascade_record runs them
// back to back -- the same operations either way):
//   phase 1: 1/Zdr_k and the off-diagonals of M = I + offdiag (nuSIprop.hpp:289-300)
//   phase 2: the LU of M (GSL's partial pivoting, :309) from those
struct RecM { double rz0, rz1, rz2, m01, m02, m10, m12, m20, m21; };
NUSI_FN RecM record_phase1(const GridDev& g, const Point& P, const double* __restrict__ Gt,
                           const double* __restrict__ At, const double* rdE, int i, int b)
{
    const double c = g.step_c[i], s = g.step_s[i];
    const double u0 = P.u[0], u1 = P.u[1], u2 = P.u[2];
    const double rd = rdE[b];
    const double Gw = s * Gt[b + i - 1], Aw = s * At[b + i - 1];
    RecM m;
    m.rz0 = rcp_nr(1.0 + c * (Gw * u0 - Aw * (u0 * u0)) * rd);
    m.rz1 = rcp_nr(1.0 + c * (Gw * u1 - Aw * (u1 * u1)) * rd);
    m.rz2 = rcp_nr(1.0 + c * (Gw * u2 - Aw * (u2 * u2)) * rd);
    // M = I + offdiag, M[k][l] = Aw u_k u_l / dE_b / Zdr_k
    m.m01 = Aw * u0 * u1 * rd * m.rz0;
    m.m02 = Aw * u0 * u2 * rd * m.rz0;
    m.m10 = Aw * u1 * u0 * rd * m.rz1;
    m.m12 = Aw * u1 * u2 * rd * m.rz1;
    m.m20 = Aw * u2 * u0 * rd * m.rz2;
    m.m21 = Aw * u2 * u1 * rd * m.rz2;
    return m;
}
__device__ __attribute__((noinline)) void lu3_factor_out(double (&A)[3][3], int (&perm)[3]) { lu3_factor(A, perm); }
// the LU fields PR_L10 .. PR_RU22 and the permutation (R[kPreFields * stride])
template <bool kCallFree>
NUSI_FN void record_phase2(const RecM& m, double* R, int stride)
{
    // LU without row exchanges when partial pivoting would not exchange (M ~ I: always, in
    // practice); the same operations as lu3_factor on that path (a / 1.0 == a), else lu3_factor
    const double a11 = 1.0 - m.m10 * m.m01, a12 = m.m12 - m.m10 * m.m02;
    const double a21 = m.m21 - m.m20 * m.m01, a22 = 1.0 - m.m20 * m.m02;
    if (fabs(m.m10) <= 1.0 && fabs(m.m20) <= 1.0 && fabs(a21) <= fabs(a11) && a11 != 0.0) {
        const double ra11 = rcp_nr(a11);
        const double l21 = a21 * ra11;
        const double u22 = a22 - l21 * a12;
        R[PR_L10 * stride] = m.m10;
        R[PR_L20 * stride] = m.m20;
        R[PR_L21 * stride] = l21;
        R[PR_U01 * stride] = m.m01;
        R[PR_U02 * stride] = m.m02;
        R[PR_U12 * stride] = a12;
        R[PR_RU00 * stride] = 1.0;
        R[PR_RU11 * stride] = ra11;
        R[PR_RU22 * stride] = rcp_nr(u22);
        R[kPreFields * stride] = (double)(0 | (1 << 2) | (2 << 4));
    } else {
        double M[3][3] = {{1.0, m.m01, m.m02}, {m.m10, 1.0, m.m12}, {m.m20, m.m21, 1.0}};
        int pm[3];
        if (kCallFree) lu3_factor(M, pm);
        else lu3_factor_out(M, pm);
        R[PR_L10 * stride] = M[1][0];
        R[PR_L20 * stride] = M[2][0];
        R[PR_L21 * stride] = M[2][1];
        R[PR_U01 * stride] = M[0][1];
        R[PR_U02 * stride] = M[0][2];
        R[PR_U12 * stride] = M[1][2];
        R[PR_RU00 * stride] = 1.0 / M[0][0];
        R[PR_RU11 * stride] = 1.0 / M[1][1];
        R[PR_RU22 * stride] = 1.0 / M[2][2];
        R[kPreFields * stride] = (double)(pm[0] | (pm[1] << 2) | (pm[2] << 4));
    }
}

// kCallFree: the caller's points all use the power-law source and the pivoting LU is inlined, so
// the record code makes no calls (a call inside the wavefront kernel's stage loop makes the
// compiler drain every outstanding alpha prefetch, vmcnt(0), after it)
template <bool kCallFree>
NUSI_FN void cascade_record(const GridDev& g, const Point& P, const double* __restrict__ Gt,
                            const double* __restrict__ At, const double* rdE, const double* pw, int i, int b,
                            double* R, int stride)
{
    const double c = g.step_c[i], s = g.step_s[i];
    const double rd = rdE[b];
    const RecM m = record_phase1(g, P, Gt, At, rdE, i, b);
    R[PR_RZ0 * stride] = m.rz0;
    R[PR_RZ1 * stride] = m.rz1;
    R[PR_RZ2 * stride] = m.rz2;
    record_phase2<kCallFree>(m, R, stride);
    double src;
    if (kCallFree || P.source == 1)   // nuSIprop.hpp:656
        src = P.norm_total / 3.0 * g.sfr[i] * (g.Emax[b] * pw[b + i + 1] - g.Emin[b] * pw[b + i]) * rcp_nr(1 - P.si);
    else
        src = lum_out(P, g.z[i], g.sfr[i], g.Emin[b], g.Emax[b]);
    R[PR_SRC * stride] = c * src;
    R[PR_SDE * stride] = P.non_resonant ? s * rd : (g.Emax[b] - g.Emin[b]);
}

// the 3x3 solve of one bin (nuSIprop.hpp:289-313) from its fields and the coupling `add` to the
// bins above; x = F[:, b] of this step
NUSI_FN void cascade_solve(double f0, double f1, double f2, double add, double src0, double u0, double u1, double u2,
                           double rz0, double rz1, double rz2, int pmb, double l10, double l20, double l21, double u01,
                           double u02, double u12, double ru00, double ru11, double ru22, double& x0, double& x1,
                           double& x2)
{
    const double v0 = (f0 + (src0 + u0 * add)) * rz0;
    const double v1 = (f1 + (src0 + u1 * add)) * rz1;
    const double v2 = (f2 + (src0 + u2 * add)) * rz2;
    const int p0 = pmb & 3, p1 = (pmb >> 2) & 3, p2 = (pmb >> 4) & 3;
    x0 = (p0 == 0) ? v0 : (p0 == 1) ? v1 : v2;
    x1 = (p1 == 0) ? v0 : (p1 == 1) ? v1 : v2;
    x2 = (p2 == 0) ? v0 : (p2 == 1) ? v1 : v2;
    x1 = x1 - l10 * x0;
    x2 = x2 - l20 * x0;
    x2 = x2 - l21 * x1;
    x2 = x2 * ru22;
    x1 = (x1 - u12 * x2) * ru11;
    x0 = (x0 - u01 * x1 - u02 * x2) * ru00;
}

// cascade_solve where every lane's LU kept the rows in place (the permutation 0 | 1 << 2 | 2 << 4, and then ru00 =
// 1 / 1.0 = 1.0: the product by it is exact and dropped) -- the same bits as cascade_solve
constexpr int kIdPerm = 0 | (1 << 2) | (2 << 4);
NUSI_FN void cascade_solve_id(double f0, double f1, double f2, double add, double src0, double u0, double u1, double u2,
                              double rz0, double rz1, double rz2, double l10, double l20, double l21, double u01,
                              double u02, double u12, double ru11, double ru22, double& x0, double& x1, double& x2)
{
    x0 = (f0 + (src0 + u0 * add)) * rz0;
    x1 = (f1 + (src0 + u1 * add)) * rz1;
    x2 = (f2 + (src0 + u2 * add)) * rz2;
    x1 = x1 - l10 * x0;
    x2 = x2 - l20 * x0;
    x2 = x2 - l21 * x1;
    x2 = x2 * ru22;
    x1 = (x1 - u12 * x2) * ru11;
    x0 = x0 - u01 * x1 - u02 * x2;
}

// cascade_solve and cascade_solve_id with the source per mass state (s0, s1, s2: the mass-resolved response of
// nusi_plan_response_mass; include/nusi.h).  Everything after the right-hand sides is the text above.
NUSI_FN void cascade_solve3(double f0, double f1, double f2, double add, double s0, double s1, double s2, double u0,
                            double u1, double u2, double rz0, double rz1, double rz2, int pmb, double l10, double l20,
                            double l21, double u01, double u02, double u12, double ru00, double ru11, double ru22,
                            double& x0, double& x1, double& x2)
{
    const double v0 = (f0 + (s0 + u0 * add)) * rz0;
    const double v1 = (f1 + (s1 + u1 * add)) * rz1;
    const double v2 = (f2 + (s2 + u2 * add)) * rz2;
    const int p0 = pmb & 3, p1 = (pmb >> 2) & 3, p2 = (pmb >> 4) & 3;
    x0 = (p0 == 0) ? v0 : (p0 == 1) ? v1 : v2;
    x1 = (p1 == 0) ? v0 : (p1 == 1) ? v1 : v2;
    x2 = (p2 == 0) ? v0 : (p2 == 1) ? v1 : v2;
    x1 = x1 - l10 * x0;
    x2 = x2 - l20 * x0;
    x2 = x2 - l21 * x1;
    x2 = x2 * ru22;
    x1 = (x1 - u12 * x2) * ru11;
    x0 = (x0 - u01 * x1 - u02 * x2) * ru00;
}
NUSI_FN void cascade_solve3_id(double f0, double f1, double f2, double add, double s0, double s1, double s2, double u0,
                               double u1, double u2, double rz0, double rz1, double rz2, double l10, double l20,
                               double l21, double u01, double u02, double u12, double ru11, double ru22, double& x0,
                               double& x1, double& x2)
{
    x0 = (f0 + (s0 + u0 * add)) * rz0;
    x1 = (f1 + (s1 + u1 * add)) * rz1;
    x2 = (f2 + (s2 + u2 * add)) * rz2;
    x1 = x1 - l10 * x0;
    x2 = x2 - l20 * x0;
    x2 = x2 - l21 * x1;
    x2 = x2 * ru22;
    x1 = (x1 - u12 * x2) * ru11;
    x0 = x0 - u01 * x1 - u02 * x2;
}

// The tabulated source term of bin b at step i (NUSI_SOURCE_TABULATED + slot, include/nusi.h): c = step_c[i],
// w = the slot's redshift weight w[i] (get_SFR(z_i) where none was given), z = z[i], S = the slot's bin integral
// S[b + i] -- the source-frame bin [E_b (1 + z_i), E_{b+1} (1 + z_i)] is source-axis bin b + i (the index-shift
// identity of pw[]).  The one place the expression is written: k_source_tab (the MFMA cascade's table) and the scalar
// k_cascade both call it, so the two cascades see the same source bits.
NUSI_FN double tabulated_src(double c, double norm, double w, double z, double S)
{
    return c * ((norm / 3.0) * (w / (1 + z)) * S);
}
// a source slot in the plan's slot storage: S [T + 1] (the source axis), then w [Nz]
NUSI_FN size_t source_slot_doubles(int T, int Nz) { return (size_t)T + 1 + Nz; }

// slots: the plan's source slots (source_slot_doubles each), read by tabulated points only (else may be nullptr)
__global__ __launch_bounds__(64) void k_cascade(GridDev g, const Point* __restrict__ pts, TablesDev t,
                                                const double* __restrict__ slots, double* __restrict__ flux,
                                                double* __restrict__ flux_fla)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int N = g.N, Nz = g.Nz, T = g.T;
    const int p = blockIdx.x, lane = threadIdx.x;
    const Point& P = pts[p];
    double* F0 = lds;
    double* F1 = lds + N;
    double* F2 = lds + 2 * N;
    double* acc = lds + 3 * N;
    double* pre = lds + 4 * N;
    int* perm = (int*)(pre + kPreFields * 64);
    const double u0 = P.u[0], u1 = P.u[1], u2 = P.u[2];
    const double uk[3] = {u0, u1, u2};
    const double* __restrict__ Gt = t.G + (size_t)P.tslot * T;
    const double* __restrict__ At = t.At + (size_t)P.tslot * T;
    const double* __restrict__ Al = t.A + (size_t)P.tslot * g.PT;
    const bool nonres = P.non_resonant;
    const bool tab = P.source >= NUSI_SOURCE_TABULATED;   // (lum() would take any such source for the DSNB)
    const double* __restrict__ tS = tab ? slots + (size_t)(P.source - NUSI_SOURCE_TABULATED) * source_slot_doubles(T, Nz) : nullptr;
    const double* __restrict__ tw = tab ? tS + T + 1 : nullptr;

    for (int b = lane; b < N; b += 64) F0[b] = F1[b] = F2[b] = 0.0;

    for (int i = Nz - 1; i > 0; --i) {
        const double c = g.step_c[i], s = g.step_s[i], zi = g.z[i], sfri = g.sfr[i];
        for (int b = lane; b < N; b += 64) acc[b] = 0.0;
        double next_acc = 0.0;     // acc of the next (lower) bin, carried in registers
        double racc = 0.0;         // resonant-only running sum (nuSIprop.hpp:261-278)
        double px0 = 0.0, px1 = 0.0, px2 = 0.0;   // F[:, b+1] of this step
        for (int base = ((N - 1) / 64) * 64; base >= 0; base -= 64) {
            __syncthreads();
            {   // ---- parallel: flux-independent quantities for bins base..base+63
                const int b = base + lane;
                if (b < N) {
                    const double dEb = g.Emax[b] - g.Emin[b];
                    const double Gw = s * Gt[b + i - 1], Aw = s * At[b + i - 1];
                    double Zd[3], M[3][3];
                    for (int k = 0; k < 3; ++k) Zd[k] = 1.0 + c * (Gw * uk[k] - Aw * (uk[k] * uk[k])) / dEb;
                    for (int k = 0; k < 3; ++k)
                        for (int l = 0; l < 3; ++l) M[k][l] = (k == l) ? 1.0 : (Aw * uk[k] * uk[l] / dEb) / Zd[k];
                    int pm[3];
                    lu3_factor(M, pm);
                    const double src0 = tab ? tabulated_src(c, P.norm_total, tw[i], zi, tS[b + i])
                                            : c * lum(P, zi, sfri, g.Emin[b], g.Emax[b]);
                    pre[PR_RZ0 * 64 + lane] = 1.0 / Zd[0];
                    pre[PR_RZ1 * 64 + lane] = 1.0 / Zd[1];
                    pre[PR_RZ2 * 64 + lane] = 1.0 / Zd[2];
                    pre[PR_SRC * 64 + lane] = src0;
                    pre[PR_L10 * 64 + lane] = M[1][0];
                    pre[PR_L20 * 64 + lane] = M[2][0];
                    pre[PR_L21 * 64 + lane] = M[2][1];
                    pre[PR_U01 * 64 + lane] = M[0][1];
                    pre[PR_U02 * 64 + lane] = M[0][2];
                    pre[PR_U12 * 64 + lane] = M[1][2];
                    pre[PR_RU00 * 64 + lane] = 1.0 / M[0][0];
                    pre[PR_RU11 * 64 + lane] = 1.0 / M[1][1];
                    pre[PR_RU22 * 64 + lane] = 1.0 / M[2][2];
                    pre[PR_SDE * 64 + lane] = nonres ? s / dEb : dEb;
                    perm[lane] = pm[0] | (pm[1] << 2) | (pm[2] << 4);
                }
            }
            __syncthreads();
            const int top = (base + 63 < N - 1) ? base + 63 : N - 1;
            for (int b = top; b >= base; --b) {
                const int l = b - base;
                const double accb_lds = (b > 0) ? acc[b - 1] : 0.0;   // for next_acc (before this bin's pushes)
                double src0 = pre[PR_SRC * 64 + l];
                double add;   // c * (coupling of this bin to the bins above)
                if (nonres) {
                    add = c * next_acc;
                } else {
                    if (b != N - 1) {
                        const double Sres = u0 * px0 + u1 * px1 + u2 * px2;
                        const size_t rd = (size_t)(b + i) * (b + i - 1) / 2 + (b + i - 1);   // alpha(b+i-1, b+i)
                        racc += Sres * (s * Al[rd]) / (g.Emax[b + 1] - g.Emin[b + 1]) / pre[PR_SDE * 64 + l];
                    }
                    add = c * racc * pre[PR_SDE * 64 + l];
                }
                const double v0 = (F0[b] + (src0 + u0 * add)) * pre[PR_RZ0 * 64 + l];
                const double v1 = (F1[b] + (src0 + u1 * add)) * pre[PR_RZ1 * 64 + l];
                const double v2 = (F2[b] + (src0 + u2 * add)) * pre[PR_RZ2 * 64 + l];
                const int pmv = perm[l];
                const int p0 = pmv & 3, p1 = (pmv >> 2) & 3, p2 = (pmv >> 4) & 3;
                double x0 = (p0 == 0) ? v0 : (p0 == 1) ? v1 : v2;
                double x1 = (p1 == 0) ? v0 : (p1 == 1) ? v1 : v2;
                double x2 = (p2 == 0) ? v0 : (p2 == 1) ? v1 : v2;
                x1 = x1 - pre[PR_L10 * 64 + l] * x0;
                x2 = x2 - pre[PR_L20 * 64 + l] * x0;
                x2 = x2 - pre[PR_L21 * 64 + l] * x1;
                x2 = x2 * pre[PR_RU22 * 64 + l];
                x1 = (x1 - pre[PR_U12 * 64 + l] * x2) * pre[PR_RU11 * 64 + l];
                x0 = (x0 - pre[PR_U01 * 64 + l] * x1 - pre[PR_U02 * 64 + l] * x2) * pre[PR_RU00 * 64 + l];
                if (lane == 0) { F0[b] = x0; F1[b] = x1; F2[b] = x2; }
                px0 = x0; px1 = x1; px2 = x2;
                if (nonres && b > 0) {
                    const double Tb = (u0 * x0 + u1 * x1 + u2 * x2) * pre[PR_SDE * 64 + l];
                    const int r = b + i - 1;                       // table column of bin b
                    const double* col = Al + (size_t)r * (r - 1) / 2 + (i - 1);
                    next_acc = accb_lds + col[b - 1] * Tb;
                    for (int bp = lane; bp < b - 1; bp += 64) acc[bp] += col[bp] * Tb;
                }
            }
        }
    }
    __syncthreads();
    // finalise (nuSIprop.hpp:328-336)
    for (int b = lane; b < N; b += 64) {
        const double dE = g.Emax[b] - g.Emin[b];
        const double f0 = F0[b] / dE, f1 = F1[b] / dE, f2 = F2[b] / dE;
        double* fo = flux + (size_t)p * 3 * N;
        double* fl = flux_fla + (size_t)p * 3 * N;
        fo[b] = f0;
        fo[N + b] = f1;
        fo[2 * N + b] = f2;
        for (int f = 0; f < 3; ++f) fl[f * N + b] = P.U2[3 * f + 0] * f0 + P.U2[3 * f + 1] * f1 + P.U2[3 * f + 2] * f2;
    }
}

// k_cascade with the source per mass state: the scalar fallback of nusi_plan_response_mass.  A COPY of k_cascade's
// text, not an include of it (k_cascade is the bit-exact yardstick of the test suite and its instructions stay where
// they are); the differences are the three marked lines.  Workgroup c is column col0 + c of the call in the layout
// [p][j][n]: its point record pts[c] is a tabulated point on the private unit-vector slot n with norm = 3 (the whole
// unit source, no third), and the source goes into row j = ((col0 + c) / M) % 3 alone.
__global__ __launch_bounds__(64) void k_cascade_mass(GridDev g, const Point* __restrict__ pts, TablesDev t,
                                                     const double* __restrict__ slots, double* __restrict__ flux,
                                                     double* __restrict__ flux_fla, long long col0, int M)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int N = g.N, Nz = g.Nz, T = g.T;
    const int p = blockIdx.x, lane = threadIdx.x;
    const int mj = (int)(((col0 + p) / M) % 3);   // (mass) the row that takes the source
    const Point& P = pts[p];
    double* F0 = lds;
    double* F1 = lds + N;
    double* F2 = lds + 2 * N;
    double* acc = lds + 3 * N;
    double* pre = lds + 4 * N;
    int* perm = (int*)(pre + kPreFields * 64);
    const double u0 = P.u[0], u1 = P.u[1], u2 = P.u[2];
    const double uk[3] = {u0, u1, u2};
    const double* __restrict__ Gt = t.G + (size_t)P.tslot * T;
    const double* __restrict__ At = t.At + (size_t)P.tslot * T;
    const double* __restrict__ Al = t.A + (size_t)P.tslot * g.PT;
    const bool nonres = P.non_resonant;
    const double* __restrict__ tS = slots + (size_t)(P.source - NUSI_SOURCE_TABULATED) * source_slot_doubles(T, Nz);
    const double* __restrict__ tw = tS + T + 1;

    for (int b = lane; b < N; b += 64) F0[b] = F1[b] = F2[b] = 0.0;

    for (int i = Nz - 1; i > 0; --i) {
        const double c = g.step_c[i], s = g.step_s[i], zi = g.z[i];
        for (int b = lane; b < N; b += 64) acc[b] = 0.0;
        double next_acc = 0.0;     // acc of the next (lower) bin, carried in registers
        double racc = 0.0;         // resonant-only running sum (nuSIprop.hpp:261-278)
        double px0 = 0.0, px1 = 0.0, px2 = 0.0;   // F[:, b+1] of this step
        for (int base = ((N - 1) / 64) * 64; base >= 0; base -= 64) {
            __syncthreads();
            {   // ---- parallel: flux-independent quantities for bins base..base+63
                const int b = base + lane;
                if (b < N) {
                    const double dEb = g.Emax[b] - g.Emin[b];
                    const double Gw = s * Gt[b + i - 1], Aw = s * At[b + i - 1];
                    double Zd[3], M[3][3];
                    for (int k = 0; k < 3; ++k) Zd[k] = 1.0 + c * (Gw * uk[k] - Aw * (uk[k] * uk[k])) / dEb;
                    for (int k = 0; k < 3; ++k)
                        for (int l = 0; l < 3; ++l) M[k][l] = (k == l) ? 1.0 : (Aw * uk[k] * uk[l] / dEb) / Zd[k];
                    int pm[3];
                    lu3_factor(M, pm);
                    const double src0 = tabulated_src(c, P.norm_total, tw[i], zi, tS[b + i]);
                    pre[PR_RZ0 * 64 + lane] = 1.0 / Zd[0];
                    pre[PR_RZ1 * 64 + lane] = 1.0 / Zd[1];
                    pre[PR_RZ2 * 64 + lane] = 1.0 / Zd[2];
                    pre[PR_SRC * 64 + lane] = src0;
                    pre[PR_L10 * 64 + lane] = M[1][0];
                    pre[PR_L20 * 64 + lane] = M[2][0];
                    pre[PR_L21 * 64 + lane] = M[2][1];
                    pre[PR_U01 * 64 + lane] = M[0][1];
                    pre[PR_U02 * 64 + lane] = M[0][2];
                    pre[PR_U12 * 64 + lane] = M[1][2];
                    pre[PR_RU00 * 64 + lane] = 1.0 / M[0][0];
                    pre[PR_RU11 * 64 + lane] = 1.0 / M[1][1];
                    pre[PR_RU22 * 64 + lane] = 1.0 / M[2][2];
                    pre[PR_SDE * 64 + lane] = nonres ? s / dEb : dEb;
                    perm[lane] = pm[0] | (pm[1] << 2) | (pm[2] << 4);
                }
            }
            __syncthreads();
            const int top = (base + 63 < N - 1) ? base + 63 : N - 1;
            for (int b = top; b >= base; --b) {
                const int l = b - base;
                const double accb_lds = (b > 0) ? acc[b - 1] : 0.0;   // for next_acc (before this bin's pushes)
                const double src0 = pre[PR_SRC * 64 + l];
                const double s0 = mj == 0 ? src0 : 0.0, s1 = mj == 1 ? src0 : 0.0, s2 = mj == 2 ? src0 : 0.0;   // (mass)
                double add;   // c * (coupling of this bin to the bins above)
                if (nonres) {
                    add = c * next_acc;
                } else {
                    if (b != N - 1) {
                        const double Sres = u0 * px0 + u1 * px1 + u2 * px2;
                        const size_t rd = (size_t)(b + i) * (b + i - 1) / 2 + (b + i - 1);   // alpha(b+i-1, b+i)
                        racc += Sres * (s * Al[rd]) / (g.Emax[b + 1] - g.Emin[b + 1]) / pre[PR_SDE * 64 + l];
                    }
                    add = c * racc * pre[PR_SDE * 64 + l];
                }
                const double v0 = (F0[b] + (s0 + u0 * add)) * pre[PR_RZ0 * 64 + l];   // (mass)
                const double v1 = (F1[b] + (s1 + u1 * add)) * pre[PR_RZ1 * 64 + l];
                const double v2 = (F2[b] + (s2 + u2 * add)) * pre[PR_RZ2 * 64 + l];
                const int pmv = perm[l];
                const int p0 = pmv & 3, p1 = (pmv >> 2) & 3, p2 = (pmv >> 4) & 3;
                double x0 = (p0 == 0) ? v0 : (p0 == 1) ? v1 : v2;
                double x1 = (p1 == 0) ? v0 : (p1 == 1) ? v1 : v2;
                double x2 = (p2 == 0) ? v0 : (p2 == 1) ? v1 : v2;
                x1 = x1 - pre[PR_L10 * 64 + l] * x0;
                x2 = x2 - pre[PR_L20 * 64 + l] * x0;
                x2 = x2 - pre[PR_L21 * 64 + l] * x1;
                x2 = x2 * pre[PR_RU22 * 64 + l];
                x1 = (x1 - pre[PR_U12 * 64 + l] * x2) * pre[PR_RU11 * 64 + l];
                x0 = (x0 - pre[PR_U01 * 64 + l] * x1 - pre[PR_U02 * 64 + l] * x2) * pre[PR_RU00 * 64 + l];
                if (lane == 0) { F0[b] = x0; F1[b] = x1; F2[b] = x2; }
                px0 = x0; px1 = x1; px2 = x2;
                if (nonres && b > 0) {
                    const double Tb = (u0 * x0 + u1 * x1 + u2 * x2) * pre[PR_SDE * 64 + l];
                    const int r = b + i - 1;                       // table column of bin b
                    const double* col = Al + (size_t)r * (r - 1) / 2 + (i - 1);
                    next_acc = accb_lds + col[b - 1] * Tb;
                    for (int bp = lane; bp < b - 1; bp += 64) acc[bp] += col[bp] * Tb;
                }
            }
        }
    }
    __syncthreads();
    // finalise (nuSIprop.hpp:328-336)
    for (int b = lane; b < N; b += 64) {
        const double dE = g.Emax[b] - g.Emin[b];
        const double f0 = F0[b] / dE, f1 = F1[b] / dE, f2 = F2[b] / dE;
        double* fo = flux + (size_t)p * 3 * N;
        double* fl = flux_fla + (size_t)p * 3 * N;
        fo[b] = f0;
        fo[N + b] = f1;
        fo[2 * N + b] = f2;
        for (int f = 0; f < 3; ++f) fl[f * N + b] = P.U2[3 * f + 0] * f0 + P.U2[3 * f + 1] * f1 + P.U2[3 * f + 2] * f2;
    }
}

typedef double nusi_f64x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// Helpers of the MFMA cascade k_cascade_bs (below): the power-law source, the DSNB source table, the chain's
// hand-off between redshift steps and the resonant-only running sum.
// ---------------------------------------------------------------------------

// the power-law source term c_i Lum of bin b at step i (nuSIprop.hpp:283, :656), the expression
// cascade_record stores in PR_SRC
NUSI_FN double powerlaw_src(const GridDev& g, const Point& P, const double* pw, int i, int b)
{
    return g.step_c[i] * (P.norm_total / 3.0 * g.sfr[i] * (g.Emax[b] * pw[b + i + 1] - g.Emin[b] * pw[b + i]) * rcp_nr(1 - P.si));
}
// the same with the point's factors hoisted: a3 = norm_total / 3.0, rs = rcp_nr(1 - si) (the same operations,
// once per point instead of once per record)
struct SrcFactors { double a3, rs; };
NUSI_FN SrcFactors src_factors(const Point& P) { return SrcFactors{P.norm_total / 3.0, rcp_nr(1 - P.si)}; }
NUSI_FN double powerlaw_src_h(const GridDev& g, const SrcFactors& f, const double* pw, int i, int b)
{
    return g.step_c[i] * (f.a3 * g.sfr[i] * (g.Emax[b] * pw[b + i + 1] - g.Emin[b] * pw[b + i]) * f.rs);
}

// The DSNB source term c_i Lum(z_i, Emin_b, Emax_b) (nuSIprop.hpp:283, :659-662) of every (step slot J, bin b)
// of a point, computed before the MFMA cascade (it costs two Li2 / Li3 pairs per record, far more than a
// wavefront stage) in the diagonal layout src[(b - J + Nz - 2) (Nz - 1) + J]: the lanes of one stage (b - J
// constant) read consecutive doubles.  The expression is cascade_record's, so the records are the same bits.
NUSI_FN size_t src_index(int Nz, int J, int b) { return (size_t)(b - J + Nz - 2) * (Nz - 1) + J; }
__global__ __launch_bounds__(256) void k_source_dsnb(GridDev g, const Point* __restrict__ pts, double* __restrict__ src)
{
    const int p = blockIdx.y, N = g.N, Nz = g.Nz, nst = Nz - 1;
    const Point& P = pts[p];
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (P.source != NUSI_SOURCE_DSNB || e >= nst * N) return;
    const int J = e / N, b = e - J * N, i = Nz - 1 - J;
    src[(size_t)p * g.T * nst + src_index(Nz, J, b)] = g.step_c[i] * lum(P, g.z[i], g.sfr[i], g.Emin[b], g.Emax[b]);
}
size_t cascade_src_doubles(const GridDev& g) { return (size_t)g.T * (g.Nz - 1); }
hipError_t launch_source_dsnb(const GridDev& g, const Point* pts, int npts, double* src, hipStream_t s)
{
    const int ne = (g.Nz - 1) * g.N;
    hipLaunchKernelGGL(k_source_dsnb, dim3((ne + 255) / 256, npts), dim3(256), 0, s, g, pts, src);
    return hipGetLastError();
}
// The tabulated points' rows of the same table, from their slots' vectors (tabulated_src).  One work-item per
// element of the row in storage order, o = d (Nz - 1) + J with d = b - J + Nz - 2: consecutive lanes write
// consecutive doubles, and b + i = d + 1, so a diagonal's Nz - 1 elements share one S.  Elements whose bin lies
// off the grid are never read and stay unwritten, like k_source_dsnb's.
__global__ __launch_bounds__(256) void k_source_tab(GridDev g, const Point* __restrict__ pts,
                                                    const double* __restrict__ slots, double* __restrict__ src)
{
    const int p = blockIdx.y, N = g.N, Nz = g.Nz, T = g.T, nst = Nz - 1;
    const Point& P = pts[p];
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (P.source < NUSI_SOURCE_TABULATED || o >= T * nst) return;
    const int d = o / nst, J = o - d * nst, b = d + J - (Nz - 2), i = Nz - 1 - J;
    if (b < 0 || b >= N) return;
    const double* __restrict__ S = slots + (size_t)(P.source - NUSI_SOURCE_TABULATED) * source_slot_doubles(T, Nz);
    const double* __restrict__ w = S + T + 1;
    src[(size_t)p * T * nst + o] = tabulated_src(g.step_c[i], P.norm_total, w[i], g.z[i], S[d + 1]);
}
hipError_t launch_source_tab(const GridDev& g, const Point* pts, int npts, const double* slots, double* src,
                             hipStream_t s)
{
    const int ne = (g.Nz - 1) * g.T;
    hipLaunchKernelGGL(k_source_tab, dim3((ne + 255) / 256, npts), dim3(256), 0, s, g, pts, slots, src);
    return hipGetLastError();
}
size_t cascade_slot_doubles(const GridDev& g) { return source_slot_doubles(g.T, g.Nz); }

// The chain's hand-off between steps: step slot j solves bin b at stage sg, right after slot j-1 solved the same
// bin at stage sg-1 (nuSIprop.hpp:257-315: step i starts from step i+1's F[:, b]).  wave_shr1 moves each lane's
// value to the next lane (DPP wave_shr:1, a register move across the wave); lane 0 receives `fill`.  It must run
// with every lane of the wave active (a disabled source lane would leave its neighbour's old value).
__device__ __forceinline__ double wave_shr1(double v, double fill)
{
    const long long x = __double_as_longlong(v), f = __double_as_longlong(fill);
    const int lo = __builtin_amdgcn_update_dpp((int)f, (int)x, 0x138, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(f >> 32), (int)(x >> 32), 0x138, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// The resonant-only chain (nuSIprop.hpp:261-278, 285-287): the running sum of the bins above, from the
// lane's own solve of bin b+1 (x = F[:, b+1] of this step).  sde = dE_b.
NUSI_FN double resonant_add(double& racc, double u0, double u1, double u2, double px0, double px1, double px2,
                            double sj, double sd, double dEb1, double sde, double cj, bool top)
{
    if (!top) racc += (u0 * px0 + u1 * px1 + u2 * px2) * (sj * sd) / dEb1 / sde;
    return cj * racc * sde;
}


// Diagnostic build only (-DNUSI_WS_TRACE, scripts/build_variant.sh): s_memtime stamps of workgroup 0's waves
// at the start of each stage's work and at its barrier (read the shares, not the length: the stamps cost
// cycles).  nusi_debug_ws_trace() copies them out.  Compiled out of the product.
#ifdef NUSI_WS_TRACE
constexpr int kTrWaves = 16, kTrStages = 512, kTrBlocks = 8192;
__device__ unsigned long long g_ws_trace[kTrWaves * kTrStages * 4];   // [wave][stage][start, barrier, chain: loaded, solved]
__device__ unsigned int g_ws_hwid[kTrBlocks * kTrWaves];   // HW_ID (SE, CU, SIMD, wave slot) of every wave
#define NUSI_WS_HWID()                                                                                             \
    do {                                                                                                           \
        if ((threadIdx.x & 63) == 0 && blockIdx.x < kTrBlocks)                                                     \
            g_ws_hwid[blockIdx.x * kTrWaves + (threadIdx.x >> 6)] = __builtin_amdgcn_s_getreg(4 | (31 << 11));     \
    } while (0)
// k_cascade_bs: [wave][block][phase A start, its barrier, phase B start, its barrier], no waits
#define NUSI_BS_STAMP(blk, which)                                                                                  \
    do {                                                                                                           \
        if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && (blk) < kTrStages)                                       \
            g_ws_trace[((threadIdx.x >> 6) * kTrStages + (blk)) * 4 + (which)] = __builtin_amdgcn_s_memtime();      \
    } while (0)
// k_cascade_bs chain wave 0, phase B, in wave slot 15: [block][stage 4q+1 loaded, solved, 4q+2 loaded, solved]
// (the "loaded" stamps wait for the stage's LDS loads first)
#define NUSI_BS_CSTAMP(blk, which)                                                                                 \
    do {                                                                                                           \
        if (((which) & 1) == 0) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                \
        if (blockIdx.x == 0 && (threadIdx.x & 63) == 0 && (blk) < kTrStages)                                       \
            g_ws_trace[(15 * kTrStages + (blk)) * 4 + (which)] = __builtin_amdgcn_s_memtime();                      \
    } while (0)
#else
#define NUSI_BS_STAMP(blk, which) do { } while (0)
#define NUSI_BS_CSTAMP(blk, which) do { } while (0)
#define NUSI_WS_HWID() do { } while (0)
#endif

// ---------------------------------------------------------------------------
// k_cascade_bs: the MFMA cascade with block-synchronous roles (round 4).  The wavefront (stage sg: step slot j
// solves bin N-1-sg+j; every active step reads the same table column r = T-1-sg, the index-shift identity), its
// push as rank-4 blocks on v_mfma_f64_16x16x4f64 (ACC[rows, steps] += alpha[rows, 4 columns] . T[4 columns, steps],
// the transfer-matrix x flux-batch GEMM whose batch is the steps in flight and, for points sharing a table, the
// points), the records and the solves.  The per-stage kernels of rounds 2-3 synchronised every wave of
// the workgroup once per STAGE, so a stage cost a barrier, an LDS round trip of the chain's records and its
// dependent solve (~2 000 cycles against a ~700-cycle floor).  The data dependencies only
// need a meeting point twice per BLOCK of four stages:
//   * block q's push (columns of stages 4q-4 .. 4q-1) needs the chain's T_j of those stages;
//   * the chain's stages 4q+1 .. 4q+4 need the rows block q publishes; stage 4q needs block q-1's.
// So every block runs in two phases between two barriers:
//   phase A: the waves holding the four rows block q publishes push block q into those tiles and publish
//            them (AX); the chain solves stage 4q (block q-1's rows);
//   phase B: the chain solves stages 4q+1 .. 4q+3 back to back (block q's rows, its own four diagonal
//            columns as before); the other push tiles add block q (their rows are published later).
// The record wave forms block q + 1's records over both phases (a third in A, where the chain solves one stage,
// the rest in B) and stages the DSNB sources; the chain forms the power-law sources itself.
// The chain is CW waves of PPW = P / CW whole points: lane (point p, j) runs step slot j (SPL = 1); slot j takes
// F[:, b] from slot j-1's solve of the previous stage by a DPP wave shift, or (first step of a pass > 0) the previous
// pass' last step through a global FIFO prefetched a block ahead.  Each stage's loads are issued a stage ahead of
// its solve, and the last pass' finalise (three divisions and six stores per bin) runs on the record wave.
// The A operands of block q + 2 are loaded while block q is pushed (two register buffers, the block loop
// unrolled by two), so the publishing tiles never wait for HBM.
// Columns: the NC = NJ P right-hand sides (point p, step j) at c = j P + p; a push tile is 16 columns (one
// step of 16 points, or 16 steps of one point), so one template <NJ, P, SPL, RT, CW> covers
//   <48, 1, 1, 4, 1>  one point per workgroup (C4)
//   <48, 2, 1, 2, 2>  two points sharing a table, a chain wave per point
//   <6, 16, 1, 2, 2>  the gamma batch, up to 16 points of a table, 8 per chain wave, step passes of 6
//   <16, 1, 1, 8, 1>  step passes of 16 on long grids (C3)
// (kNR: every point of the launch non-resonant, the resonant-only terms compiled out).  The MFMA sums each
// element's four columns in its own order whichever column it is, so a point's fluxes depend on its grouping only
// through the step passes (to rounding).  Waves: push waves of 16 RT rows, the chain waves, the record wave.
// ---------------------------------------------------------------------------
// Two shipped placements (measured against their absence, DESIGN.md "Retired build variants"):
//   * the chain and record waves sit beside the least-busy push waves (wave w runs on SIMD f(w % 4), HW_ID in the
//     trace build): C5 cascade 3.19 -> 2.82 ms, C3 23.4 -> 21.4, C4 equal (profiles/r4/ab/r4u, r4v);
//   * the chain and record waves run at raised issue priority (s_setprio 3; the push waves 0): C5 cascade 3.51 ->
//     3.25 ms, C3 29.1 -> 24.8, C4 0.555 -> 0.528 (profiles/r4/ab/r4n, r4o).  Sleeping the push waves at phase B's
//     start (to let the chain's loads first) measured no gain.
template <int NJ, int P, int SPL, int RT, int CW>
struct BsCfg {
    static constexpr int LPP = NJ / SPL;   // chain lanes per point
    static constexpr int PPW = P / CW;     // points per chain wave
    static constexpr int NC = NJ * P;      // right-hand columns
    static constexpr int NB = NC / 16;     // push column tiles
    static_assert(SPL == 1 && P % CW == 0 && NC % 16 == 0 && LPP * PPW <= 64, "a step slot per chain lane, whole points per chain wave, whole column tiles");
};

// record fields of the block-synchronous kernel: PR_* without PR_SRC (the sources have a block of their own), so
// fields >= PR_L10 sit one lower -- record_phase2 writes them through a base pointer one field stride lower
enum { BR_RZ0, BR_RZ1, BR_RZ2, BR_L10, BR_L20, BR_L21, BR_U01, BR_U02, BR_U12, BR_RU00, BR_RU11, BR_RU22, BR_SDE, BR_PERM,
       kBsFields };
static_assert(PR_L10 - 1 == BR_L10 && PR_RU22 - 1 == BR_RU22 && kPreFields - 1 == BR_PERM, "record_phase2's fields, shifted");

// The impulse-source instance's arguments (k_cascade_bs_impulse, the response matrix of nusi_plan_response): workgroup k
// takes the table of point p0 + k / ngrp and the P source-axis bins n = 1 + P (k % ngrp) .. (the last group of a table
// is partial), column n of point p written where an ordinary launch writes "point" p (T + 1) + n.
struct ImpulseArgs {
    const double* w;   // [Nz] the redshift weights
    int p0, ngrp;
};

template <int NJ, int P, int SPL, int RT, int CW, bool kNR>   // kNR: every point of the launch non-resonant
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_cascade_bs(GridDev g, const Point* __restrict__ pts, const int* __restrict__ gidx, const int2* __restrict__ grp,
                  TablesDev t, double* __restrict__ fh, double* __restrict__ flux, double* __restrict__ flux_fla)
{
    constexpr bool kImp = false, kMass = false;
    const ImpulseArgs ia{};
#include "nusi_cascade_bs_body.inc"
}
// The impulse-source instance, of the gamma batch's shape: 16 source-axis bins of one table on the MFMA N dimension,
// step passes of 6 (launch_cascade_impulse).  flux = G, flux_fla = G_fla.
template <bool kNR>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_cascade_bs_impulse(GridDev g, const Point* __restrict__ pts, ImpulseArgs ia, TablesDev t, double* __restrict__ fh,
                          double* __restrict__ flux, double* __restrict__ flux_fla)
{
    constexpr int NJ = 6, P = 16, SPL = 1, RT = 2, CW = 2;
    constexpr bool kImp = true, kMass = false;
    const int* const gidx = nullptr;
    const int2* const grp = nullptr;
#include "nusi_cascade_bs_body.inc"
}
// The mass-resolved impulse instance (nusi_plan_response_mass): k_cascade_bs_impulse with the unit source in one mass
// state per workgroup (kMass in the body): three times its workgroups, (table, source state j, bin group) decoded from
// blockIdx.x and ia.ngrp.  flux = G3, flux_fla = G3_fla, [p][j][n][3][N].  (Its name keeps clear of the patterns that
// count the k_cascade_bs and k_cascade_bs_impulse instances in the resource tests.)
template <bool kNR>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(4, 4)))
void k_cascade_mass_impulse(GridDev g, const Point* __restrict__ pts, ImpulseArgs ia, TablesDev t, double* __restrict__ fh,
                            double* __restrict__ flux, double* __restrict__ flux_fla)
{
    constexpr int NJ = 6, P = 16, SPL = 1, RT = 2, CW = 2;
    constexpr bool kImp = true, kMass = true;
    const int* const gidx = nullptr;
    const int2* const grp = nullptr;
#include "nusi_cascade_bs_body.inc"
}
// the redshift-step slots of a one-pass wavefront: up to 48 (Nz - 1 rounded up to 16, 32 or 48), 0 beyond
static int wf_nj(const GridDev& g) { const int n = g.Nz - 1; return n <= 16 ? 16 : n <= 32 ? 32 : n <= 48 ? 48 : 0; }

static thread_local const char* t_cascade_kernel = "";   // the kernel the latest launch on this thread chose
const char* last_cascade_kernel() { return t_cascade_kernel; }

// the block-synchronous kernel (k_cascade_bs): push waves of 16 RT rows, the chain wave, the record wave
static int bs_push_waves(const GridDev& g, int RT) { return (g.T - 1 + 16 * RT - 1) / (16 * RT); }
template <int NJ, int P, int SPL, int RT, int CW>
static size_t bs_lds(const GridDev& g)
{
    constexpr int NC = NJ * P;
    return sizeof(double) * (2 * (size_t)kBsFields * 4 * NJ + 3 * 8 * (size_t)NC + 48 * (size_t)P + 13 * (size_t)P +
                             3 * (size_t)g.N + (size_t)P * (g.T + 2) + 6 * (size_t)g.T + 4 * (size_t)g.Nz);
}
template <int NJ, int P, int SPL, int RT, int CW>
static bool bs_fits_t(const GridDev& g)
{
    return g.T >= 2 && g.Nz >= 2 && bs_push_waves(g, RT) + CW + 1 <= 16 && bs_lds<NJ, P, SPL, RT, CW>(g) <= 160 * 1024;
}
template <int NJ, int P, int SPL, int RT, int CW>
static void launch_bs_t(const GridDev& g, const Point* pts, const int* gidx, const int2* grp, int nwg, TablesDev t,
                        double* fh, double* flux, double* flux_fla, hipStream_t s, bool all_nr)
{
    const int nthr = 64 * (bs_push_waves(g, RT) + CW + 1);
    const size_t lds = bs_lds<NJ, P, SPL, RT, CW>(g);
    if (all_nr)   // the instance without the resonant-only running sum (every BASELINE workload)
        hipLaunchKernelGGL((k_cascade_bs<NJ, P, SPL, RT, CW, true>), dim3(nwg), dim3(nthr), lds, s, g, pts, gidx, grp, t, fh,
                           flux, flux_fla);
    else
        hipLaunchKernelGGL((k_cascade_bs<NJ, P, SPL, RT, CW, false>), dim3(nwg), dim3(nthr), lds, s, g, pts, gidx, grp, t,
                           fh, flux, flux_fla);
}
// P = 1: <wf_nj, 1, 1, 4, 1> for one pass of up to 48 steps, else step passes of 48 (rows <= 14 x 64) or of 16 (rows
// <= 14 x 128; force_passes: that instance on any grid it fits); P = 2: <wf_nj or 48, 2, 1, 2, 2>; P = 16 (the gamma
// batch): <6, 16, 1, 2, 2>
int cascade_bs_config(const GridDev& g, int P, bool force_passes)
{
    const int nj = wf_nj(g);
    if (P == 1 && force_passes) return bs_fits_t<16, 1, 1, 8, 1>(g) ? 16 + 1000 : 0;   // NUSI_OPT_STEP_PASSES = 1
    if (P == 1) {
        if (nj && bs_fits_t<48, 1, 1, 4, 1>(g)) return nj;
        if (bs_fits_t<48, 1, 1, 4, 1>(g)) return 48;
        if (bs_fits_t<16, 1, 1, 8, 1>(g)) return 16 + 1000;   // 128-row push waves
        return 0;
    }
    if (P == 2) return bs_fits_t<48, 2, 1, 2, 2>(g) ? (nj ? nj : 48) : 0;
    if (P == 16) return bs_fits_t<6, 16, 1, 2, 2>(g) ? 6 : 0;
    return 0;
}
size_t cascade_bs_scratch_doubles(const GridDev& g, int P) { return (size_t)3 * g.N * P; }
hipError_t launch_cascade_bs(const GridDev& g, const Point* pts, int P, const int* gidx, const int2* grp, int nwg,
                             TablesDev t, double* fh, double* flux, double* flux_fla, hipStream_t s, bool all_nr,
                             bool force_passes)
{
    if (nwg <= 0) return hipSuccess;
    const int c = cascade_bs_config(g, P, force_passes && P == 1);
    if (!c) return hipErrorInvalidValue;
    if (P == 1) {
        t_cascade_kernel = "k_cascade_bs";
        switch (c) {
        case 16: launch_bs_t<16, 1, 1, 4, 1>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr); break;
        case 32: launch_bs_t<32, 1, 1, 4, 1>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr); break;
        case 48: launch_bs_t<48, 1, 1, 4, 1>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr); break;
        default: launch_bs_t<16, 1, 1, 8, 1>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr); break;
        }
    } else if (P == 2) {
        t_cascade_kernel = "k_cascade_bs_pairs";
        switch (c) {
        case 16: launch_bs_t<16, 2, 1, 2, 2>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr); break;
        case 32: launch_bs_t<32, 2, 1, 2, 2>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr); break;
        default: launch_bs_t<48, 2, 1, 2, 2>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr); break;
        }
    } else {
        t_cascade_kernel = "k_cascade_bs_gamma";
        launch_bs_t<6, 16, 1, 2, 2>(g, pts, gidx, grp, nwg, t, fh, flux, flux_fla, s, all_nr);
    }
    return hipGetLastError();
}

// The impulse cascade (nusi_plan_response): the gamma batch's shape without its pw[] rows, plus sig[Nz]
static size_t imp_lds(const GridDev& g)
{
    return bs_lds<6, 16, 1, 2, 2>(g) - sizeof(double) * 16 * ((size_t)g.T + 2) + sizeof(double) * (size_t)g.Nz;
}
int cascade_impulse_groups(const GridDev& g) { return (g.T + 15) / 16; }   // workgroups per table: bins 1 .. T in 16s
bool cascade_impulse_fits(const GridDev& g)
{
    return g.T >= 2 && g.Nz >= 2 && bs_push_waves(g, 2) + 2 + 1 <= 16 && imp_lds(g) <= 160 * 1024;
}
size_t cascade_impulse_scratch_doubles(const GridDev& g) { return (size_t)cascade_impulse_groups(g) * 3 * g.N * 16; }
hipError_t launch_cascade_impulse(const GridDev& g, const Point* pts, int p0, int npts, const double* w, TablesDev t,
                                  double* fh, double* G, double* G_fla, hipStream_t s, bool all_nr)
{
    if (npts <= 0) return hipSuccess;
    if (!cascade_impulse_fits(g)) return hipErrorInvalidValue;
    t_cascade_kernel = "k_cascade_bs_impulse";
    const int ngrp = cascade_impulse_groups(g), nthr = 64 * (bs_push_waves(g, 2) + 2 + 1);
    const ImpulseArgs ia{w, p0, ngrp};
    if (all_nr)
        hipLaunchKernelGGL((k_cascade_bs_impulse<true>), dim3(npts * ngrp), dim3(nthr), imp_lds(g), s, g, pts, ia, t, fh, G,
                           G_fla);
    else
        hipLaunchKernelGGL((k_cascade_bs_impulse<false>), dim3(npts * ngrp), dim3(nthr), imp_lds(g), s, g, pts, ia, t, fh,
                           G, G_fla);
    return hipGetLastError();
}

// The mass-resolved impulse cascade: 3 cascade_impulse_groups workgroups and 3 cascade_impulse_scratch_doubles of
// FIFO per table of the launch
hipError_t launch_cascade_mass_impulse(const GridDev& g, const Point* pts, int p0, int npts, const double* w, TablesDev t,
                                       double* fh, double* G3, double* G3_fla, hipStream_t s, bool all_nr)
{
    if (npts <= 0) return hipSuccess;
    if (!cascade_impulse_fits(g)) return hipErrorInvalidValue;
    t_cascade_kernel = "k_cascade_mass_impulse";
    const int ngrp = cascade_impulse_groups(g), nthr = 64 * (bs_push_waves(g, 2) + 2 + 1);
    if ((long long)npts * 3 * ngrp > 2147483647LL) return hipErrorInvalidValue;
    const ImpulseArgs ia{w, p0, ngrp};
    if (all_nr)
        hipLaunchKernelGGL((k_cascade_mass_impulse<true>), dim3(npts * 3 * ngrp), dim3(nthr), imp_lds(g), s, g, pts, ia, t,
                           fh, G3, G3_fla);
    else
        hipLaunchKernelGGL((k_cascade_mass_impulse<false>), dim3(npts * 3 * ngrp), dim3(nthr), imp_lds(g), s, g, pts, ia, t,
                           fh, G3, G3_fla);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_response_apply: spectra on resident response matrices (nusi_plan_response_apply),
//     out[t][q][r] = scale[q] * acc,  acc = 0.0;  for n = 1 .. M-1 ascending: acc = acc + G[t][n][r] * S[q][n]
// (the product and the sum rounded separately: the translation unit is built with -ffp-contract=off, and the pragma
// below says so here).  Bandwidth-bound: lanes on r (rows are contiguous for fixed n), kApplyQ spectra as
// accumulators per lane, so G is read once per chunk of spectra; S[q][n] is wave-uniform (scalar loads).  A row
// r = 3-vector index k, bin b holds +0.0 for n <= b (the cascade's direction), and adding +0.0 * S to a non-negative
// sum changes no bit: each wave starts at n = (its lowest bin) + 1.
// ---------------------------------------------------------------------------
constexpr int kApplyQ = 8, kApplyThreads = 256;
__global__ __launch_bounds__(kApplyThreads) void k_response_apply(const double* __restrict__ G, const double* __restrict__ S,
                                                                  const double* __restrict__ scale,
                                                                  double* __restrict__ out, int M, int N, int Q, int nrb)
{
#pragma clang fp contract(off)
    const int R3 = 3 * N;
    const int t = (int)blockIdx.x / nrb, rb = (int)blockIdx.x - t * nrb, q0 = (int)blockIdx.y * kApplyQ;
    const int r = rb * kApplyThreads + (int)threadIdx.x;
    const int rw = __builtin_amdgcn_readfirstlane(r & ~63), bw = rw % N;
    const int nlo = (bw + 63 < N) ? bw + 1 : 1;   // (a wave that crosses into the next mass state starts at bin 0)
    const int rc = r < R3 ? r : R3 - 1;
    const double* __restrict__ Gr = G + (size_t)t * M * R3 + rc;
    const double* Sq[kApplyQ];
#pragma unroll
    for (int k = 0; k < kApplyQ; ++k) Sq[k] = S + (size_t)(q0 + k < Q ? q0 + k : Q - 1) * M;
    double acc[kApplyQ];
#pragma unroll
    for (int k = 0; k < kApplyQ; ++k) acc[k] = 0.0;
#pragma unroll 4
    for (int n = nlo; n < M; ++n) {
        const double gv = Gr[(size_t)n * R3];
#pragma unroll
        for (int k = 0; k < kApplyQ; ++k) acc[k] = acc[k] + gv * Sq[k][n];
    }
    if (r < R3)
#pragma unroll
        for (int k = 0; k < kApplyQ; ++k)
            if (q0 + k < Q) out[((size_t)t * Q + q0 + k) * R3 + r] = (scale ? scale[q0 + k] : 1.0) * acc[k];
}
hipError_t launch_response_apply(const GridDev& g, const double* G, int ntab, const double* S, int Q, const double* scale,
                                 double* out, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0) return hipSuccess;
    const int nrb = (3 * g.N + kApplyThreads - 1) / kApplyThreads;
    hipLaunchKernelGGL(k_response_apply, dim3((unsigned)ntab * nrb, (Q + kApplyQ - 1) / kApplyQ), dim3(kApplyThreads), 0, s,
                       G, S, scale, out, g.T + 1, g.N, Q, nrb);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_response_compose: a source's flavour composition on mass-resolved response matrices (nusi_plan_response_compose),
//     out[t][c][x] = (kappa[t][c][0] A[t][0][x] + kappa[t][c][1] A[t][1][x]) + kappa[t][c][2] A[t][2][x]
// (products and sums rounded separately).  Bandwidth-bound and elementwise: lanes on x, a workgroup reads its three
// values of A once and writes the Qc compositions of them; kappa[t][c][:] is wave-uniform (scalar loads).
// ---------------------------------------------------------------------------
constexpr int kComposeThreads = 256;
__global__ __launch_bounds__(kComposeThreads) void k_response_compose(const double* __restrict__ A,
                                                                      const double* __restrict__ kappa,
                                                                      double* __restrict__ out, size_t X, int Qc,
                                                                      unsigned nxb)
{
#pragma clang fp contract(off)
    const size_t t = blockIdx.x / nxb, xb = blockIdx.x - t * nxb;
    const size_t x = xb * kComposeThreads + threadIdx.x;
    if (x >= X) return;
    const double* __restrict__ At = A + t * 3 * X + x;
    const double a0 = At[0], a1 = At[X], a2 = At[2 * X];
    const double* __restrict__ kt = kappa + t * (size_t)Qc * 3;
    double* __restrict__ ot = out + t * (size_t)Qc * X + x;
    for (int c = 0; c < Qc; ++c) {
        const double k0 = kt[3 * c], k1 = kt[3 * c + 1], k2 = kt[3 * c + 2];
        ot[(size_t)c * X] = (k0 * a0 + k1 * a1) + k2 * a2;
    }
}
// (the caller has checked ntab x ceil(X / 256) < 2^31)
hipError_t launch_response_compose(const double* A, int ntab, size_t X, const double* kappa, int Qc, double* out,
                                   hipStream_t s)
{
    if (ntab <= 0 || Qc <= 0 || X == 0) return hipSuccess;
    const size_t nxb = (X + kComposeThreads - 1) / kComposeThreads;
    hipLaunchKernelGGL(k_response_compose, dim3((unsigned)(nxb * ntab)), dim3(kComposeThreads), 0, s, A, kappa, out, X, Qc,
                       (unsigned)nxb);
    return hipGetLastError();
}

// the scalar cascade with the source per mass state (k_cascade_mass): the columns col0 .. col0 + npts - 1 of a
// mass-resolved response, M = T + 1
hipError_t launch_cascade_mass_exact(const GridDev& g, const Point* pts, int npts, TablesDev t, const double* slots,
                                     double* flux, double* flux_fla, long long col0, hipStream_t s)
{
    t_cascade_kernel = "k_cascade_mass";
    const size_t lds = cascade_lds_bytes(g.N);
    hipLaunchKernelGGL(k_cascade_mass, dim3(npts), dim3(64), lds, s, g, pts, t, slots, flux, flux_fla, col0, g.T + 1);
    return hipGetLastError();
}

// the bit-exact scalar cascade (NUSI_CASCADE_WAVEFRONT / REG / LDS): k_cascade, one wavefront per point, any N
hipError_t launch_cascade_exact(const GridDev& g, const Point* pts, int npts, TablesDev t, const double* slots,
                                double* flux, double* flux_fla, hipStream_t s)
{
    t_cascade_kernel = "k_cascade";
    const size_t lds = cascade_lds_bytes(g.N);
    hipLaunchKernelGGL(k_cascade, dim3(npts), dim3(64), lds, s, g, pts, t, slots, flux, flux_fla);
    return hipGetLastError();
}

}  // namespace nusi

#ifdef NUSI_WS_TRACE
// diagnostic build: workgroup 0's block stamps of the latest k_cascade_bs launch, [wave][block][phase stamps]
extern "C" int nusi_debug_ws_trace(unsigned long long* out, int n)
{
    const int m = n < nusi::kTrWaves * nusi::kTrStages * 4 ? n : nusi::kTrWaves * nusi::kTrStages * 4;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(nusi::g_ws_trace), sizeof(unsigned long long) * m) == hipSuccess ? 0 : -5;
}
// HW_ID of every wave of the first kTrBlocks workgroups, [block][wave]
extern "C" int nusi_debug_ws_hwid(unsigned int* out, int n)
{
    const int m = n < nusi::kTrBlocks * nusi::kTrWaves ? n : nusi::kTrBlocks * nusi::kTrWaves;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(nusi::g_ws_hwid), sizeof(unsigned int) * m) == hipSuccess ? 0 : -5;
}
#endif
