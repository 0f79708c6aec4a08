// nuSIprop MI355X -- folding fluxes and response matrices with a detector (nusi_plan_set_detector; no reference
// counterpart: the reference stops at get_flux_fla).
//
//   k_detector_fold<CT>   rows [.][3 N] times the detector matrix D [3 N][C] on the fp64 matrix cores
//                         (nusi_plan_fold_flux, nusi_plan_response_fold); CT = ceil(C / 16) column tiles
//   k_detector_events     spectra on folded response matrices R [t][M][C]: expected counts per reconstructed bin
//                         and the Poisson statistic (nusi_plan_response_events), in a defined order
//   k_detector_profile    that statistic profiled over the flux normalisation: Newton's iteration per (t, q), its
//                         sums over the bins as butterflies inside a wave (nusi_plan_response_profile)
//   k_detector_fit<NC>    that statistic minimised over NC = 1 + K normalisations, the signal's and K background
//                         templates' under Gaussian priors: a damped Newton iteration per (t, q) (nusi_plan_response_fit)
//   k_components_fit<J, NC>
//                         that fit with J = 2 .. 3 signal components per (t, q), each a stack of rows of its own, in front
//                         of the K = NC - J templates (nusi_plan_response_fit_components)
//   k_ensemble_profile, k_ensemble_fit<NC>, k_ensemble_best
//                         those two iterations for P data sets on one front half, and per (data set, table) the best
//                         spectrum's record only (nusi_plan_response_ensemble)
//   k_conditional_fit<K>, k_interval<NC>
//                         the fit with the signal's scale held, and the limits on that scale (nusi_plan_response_fit_fixed,
//                         nusi_plan_response_limit)
//   k_toys_limit<NC>, k_toys_band
//                         those limits for P data sets on one front half, and per (table, spectrum) the order statistics
//                         of the P limits (nusi_plan_response_ensemble_limit)
//   k_poisson_draw        Poisson counts around expectations mu [rows][C], P per bin, from the counter-based generator
//                         of nusi_draw.hpp (nusi_plan_draw_counts)
//   k_inject<NC>          per (table, spectrum) P toys drawn from the injected expectation where they are fitted: the
//                         best fit, one conditional fit and the statistic per toy; k_toys_band then selects the order
//                         statistics of theta_hat_0 and of the statistic (nusi_plan_response_inject)
//   k_normal_draw         truncated normal variates from the same generator (nusi_plan_draw_normals)
//   k_nuis_inject<NC, MODE>, k_nuis_belt<NC>
//                         k_inject and k_belt with the toys' constrained nuisances randomised (NUSI_OPT_TOY_NUISANCE): the
//                         prior means redrawn per toy, or the nuisances thrown from their priors
//   k_belt<NC>, k_belt_accept
//                         k_inject's toy body once against the data and then per toy, on records (table, spectrum, grid
//                         point of the test scale), the toys drawn from the observed conditional fit's expectation; then
//                         per (table, spectrum) the accepted grid points as an interval (nusi_plan_response_belt)
//   k_composition_belt<NCF>, k_composition_accept
//                         k_belt's construction for the flavour composition: per (table, spectrum, point of the composition
//                         grid) the free fit of three signal components and the fit at the held composition, against the
//                         data and then per toy; then the accepted points (nusi_plan_response_composition_belt)
//
// The iterations several of these kernels run exist once, as text the kernels #include inside their bodies (not as
// __device__ helpers, which moved the kernels' registers: DESIGN.md sec. 4, "The shared iterations"):
//   nusi_fit_newton.inc          k_detector_fit's iteration: k_detector_fit, k_ensemble_fit, and for NC > 1 the best fit
//                                of k_interval, k_toys_limit, k_inject; k_components_fit with FN_NSIG = J signal components
//   nusi_profile_chain4.inc      k_detector_profile's, four chains a lane: k_detector_profile, k_ensemble_profile
//   nusi_profile_chain1.inc      k_detector_profile's, one chain a lane: the best fit at NC = 1 of k_interval,
//                                k_toys_limit, k_inject
//   nusi_conditional_newton.inc  k_conditional_fit's rounds: k_conditional_fit, k_inject, k_belt
//   nusi_toy_body.inc            one data set's best fit, conditional fit and statistic: k_inject, k_belt and their
//                                k_nuis_ forms
//   nusi_composition_body.inc    one data set's free fit, held fit and statistic: k_composition_belt (it #includes
//                                nusi_fit_newton.inc twice and nusi_profile_chain1.inc)
//   nusi_inject_setup.inc, nusi_inject_store.inc, nusi_belt_setup.inc, nusi_belt_store.inc
//                                what stands around the toy's draw in k_inject and k_belt: those and k_nuis_inject, k_nuis_belt
//   nusi_search_setup.inc, nusi_search_side.inc
//                                the search for a limit: k_interval, k_toys_limit
//   nusi_ldlt_solve.inc          the Newton direction, inside the fit's, the conditional fit's and the search's text
//   nusi_fit_statistic.inc       the statistic's serial sum from LDS: k_detector_fit, k_components_fit, k_conditional_fit,
//                                k_interval
#include <hip/hip_runtime.h>

#include "nusi_internal.hpp"
#include "nusi_libm.hpp"
#include "nusi_draw.hpp"

namespace nusi {

typedef double det_f64x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// k_detector_fold: out[t][n][c] = sum_{r < 3 N} X[t][n][r] D[c][r] (+ bg[c]), a batched fp64 GEMM
// (rows x 3 N) . (3 N x C) on v_mfma_f64_16x16x4_f64.
//
// One workgroup (4 waves) takes 16 rows n0 .. n0 + 15 of one table and every column.  K = the 3 N entries of a row
// runs in chunks of kFoldKC staged through LDS: rows are 3 N doubles apart, so the loads go along a row (each wave
// instruction reads 512 contiguous bytes), eight per thread, issued a chunk ahead of the MFMAs that consume them.
// The four waves split a chunk's K quads (wave w takes quads w, w + 4, ..), each holding a full 16 x 16 CT
// accumulator; the partial sums meet in LDS and wave 0 adds them in wave order.  The detector is read from the
// plan's K-major copy Dt [3 N][16 CT] (zero-padded columns) straight from L2: lane l's B operand of column tile ct
// is Dt[k = l >> 4][16 ct + (l & 15)], 128 contiguous bytes per K.
//
// Operand maps (as in nusi_cascade_bs_body.inc): A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15],
// C/D element e of lane l = [row = (l >> 4) + 4 e][col = l & 15].
//
// tri (response rows): G[n][.][b] = +0.0 for b >= n, so the tile reads only the bins b < nb = min(N, n0 + 16) of
// each flavour; K then runs over the compacted index kk = f nb + b.  A K remainder is zero-filled on the A side
// (the B side reads a clamped, finite entry), so it adds +0.0.  Every term is non-negative: the sum is at most
// gamma_{3 N} from exact in any order, and +0.0 where every product is zero.
// ---------------------------------------------------------------------------
constexpr int kFoldThreads = 256, kFoldKC = 128, kFoldLd = kFoldKC + 2, kFoldRows = 16;

template <int CT>
__global__ __launch_bounds__(kFoldThreads) void k_detector_fold(const double* __restrict__ X, const double* __restrict__ Dt,
                                                                const double* __restrict__ bg, double* __restrict__ out,
                                                                int rows, int N, int C, int ntile, int tri)
{
    constexpr int kStage = kFoldRows * kFoldLd, kRed = 3 * CT * 256, kLds = kStage > kRed ? kStage : kRed;
    constexpr int Cp = 16 * CT;
    __shared__ double sh[kLds];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = (int)blockIdx.x / ntile, n0 = ((int)blockIdx.x - t * ntile) * kFoldRows;
    const int nb = (tri && n0 + kFoldRows < N) ? n0 + kFoldRows : N;
    const int K = 3 * nb, R3 = 3 * N, nch = (K + kFoldKC - 1) / kFoldKC;
    const int skip = N - nb;
    auto rmap = [&](int kk) { return kk + ((kk >= nb) + (kk >= 2 * nb)) * skip; };   // compacted K -> entry of the row
    const double* __restrict__ Xt = X + ((size_t)t * rows + n0) * R3;
    const int kl = tid & (kFoldKC - 1), rp = tid >> 7;
    const int rlast = rows - 1 - n0;   // last valid row of the tile (>= 0)
    auto load = [&](int ch, double (&v)[8]) {
        const int kk = ch * kFoldKC + kl;
        const bool ok = kk < K;
        const int r = rmap(ok ? kk : K - 1);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int row = rp + 2 * j;
            const double x = Xt[(size_t)(row < rlast ? row : rlast) * R3 + r];
            v[j] = (ok && row <= rlast) ? x : 0.0;
        }
    };
    det_f64x4 acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) acc[ct] = det_f64x4{0.0, 0.0, 0.0, 0.0};
    double v[8];
    load(0, v);
#pragma unroll 1
    for (int ch = 0; ch < nch; ++ch) {
        __syncthreads();   // the previous chunk's MFMAs have read sh
#pragma unroll
        for (int j = 0; j < 8; ++j) sh[(rp + 2 * j) * kFoldLd + kl] = v[j];
        __syncthreads();
        if (ch + 1 < nch) load(ch + 1, v);
        const int kc0 = ch * kFoldKC;
#pragma unroll
        for (int i = 0; i < kFoldKC / 16; ++i) {
            const int kq = wave + 4 * i;
            if (kc0 + 4 * kq < K) {   // (uniform per wave)
                const int kk = kc0 + 4 * kq + (lane >> 4);
                const double a = sh[(lane & 15) * kFoldLd + 4 * kq + (lane >> 4)];
                const double* __restrict__ Dr = Dt + (size_t)rmap(kk < K ? kk : K - 1) * Cp + (lane & 15);
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Dr[16 * ct], acc[ct], 0, 0, 0);
            }
        }
    }
    __syncthreads();
    if (wave > 0)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) sh[((wave - 1) * CT + ct) * 256 + e * 64 + lane] = acc[ct][e];
    __syncthreads();
    if (wave == 0)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                double s = acc[ct][e];
#pragma unroll
                for (int w = 0; w < 3; ++w) s = s + sh[(w * CT + ct) * 256 + e * 64 + lane];
                const int row = n0 + (lane >> 4) + 4 * e, col = 16 * ct + (lane & 15);
                if (row < rows && col < C) out[((size_t)t * rows + row) * C + col] = bg ? s + bg[col] : s;
            }
}

int detector_ld(int C) { return 16 * ((C + 15) / 16); }

hipError_t launch_detector_fold(const GridDev& g, const double* X, int ntab, int rows, bool tri, const double* Dt, int C,
                                const double* bg, double* out, hipStream_t s)
{
    if (ntab <= 0 || rows <= 0) return hipSuccess;
    const int ntile = (rows + kFoldRows - 1) / kFoldRows;
    const dim3 grid((unsigned)ntab * ntile), block(kFoldThreads);
    switch ((C + 15) / 16) {
    case 1: hipLaunchKernelGGL((k_detector_fold<1>), grid, block, 0, s, X, Dt, bg, out, rows, g.N, C, ntile, (int)tri); break;
    case 2: hipLaunchKernelGGL((k_detector_fold<2>), grid, block, 0, s, X, Dt, bg, out, rows, g.N, C, ntile, (int)tri); break;
    case 3: hipLaunchKernelGGL((k_detector_fold<3>), grid, block, 0, s, X, Dt, bg, out, rows, g.N, C, ntile, (int)tri); break;
    case 4: hipLaunchKernelGGL((k_detector_fold<4>), grid, block, 0, s, X, Dt, bg, out, rows, g.N, C, ntile, (int)tri); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The event-side kernels (k_detector_events, _profile, _fit<NC>): a block of kEvThreads lanes takes one table t.  Its
// lanes sit on (c, group): c = the low lgC = ceil(log2 C) bits of the thread index (padding lanes c >= C read bin
// C - 1 and store nothing), a group = per spectra (kEvQ, or the fit's one), so a block owns QB = det_qb(lgC, per)
// spectra and the grid is (tables, ceil(Q / QB)): DetGeom.  The 2^lgC lanes of a group lie inside one wave (C <= 64,
// groups aligned).  The events and the profile kernel call det_front and det_poisson; k_detector_fit writes both out
// with one accumulator, because through the helpers k_detector_fit<4> measured 0.4 % slower.
// ---------------------------------------------------------------------------
constexpr int kEvThreads = 256, kEvQ = 4, kEvLds = 1536;
static_assert((kEvThreads >> 6) >= 1 && NUSI_DETECTOR_BINS_MAX <= 64, "event kernels: a block holds at least one group of 64 lanes on c");

constexpr int ceil_log2(int C)
{
    int lg = 0;
    while ((1 << lg) < C) ++lg;
    return lg;
}
constexpr int det_qb(int lgC, int per) { return (kEvThreads >> lgC) * per; }

struct DetGeom {
    int lg, QB;
    dim3 grid;
    DetGeom(int C, int per, int ntab, int Q) : lg(ceil_log2(C)), QB(det_qb(lg, per)), grid((unsigned)ntab, (unsigned)((Q + QB - 1) / QB)) {}
};

// The front half, in the order include/nusi.h defines:
//     acc = 0.0;  for n = 1 .. M-1 ascending: acc = acc + R[t][n][c] * S[q][n]
// (every product and sum rounded separately: -ffp-contract=off, and the pragma below) for the NQ spectra q0 .. of a
// lane (spectra past Q - 1 read spectrum Q - 1).  R[t] (M C doubles) is re-read from L2 with c on neighbouring
// lanes, each value serving NQ accumulators.
template <int NQ>
__device__ __forceinline__ void det_front(const double* __restrict__ R, const double* __restrict__ S, int t, int M, int C,
                                          int cc, int q0, int Q, double (&acc)[NQ])
{
#pragma clang fp contract(off)
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const double* Sq[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) Sq[j] = S + (size_t)(q0 + j < Q ? q0 + j : Q - 1) * M;
#pragma unroll
    for (int j = 0; j < NQ; ++j) acc[j] = 0.0;
#pragma unroll 4
    for (int n = 1; n < M; ++n) {
        const double rv = Rt[(size_t)n * C];
#pragma unroll
        for (int j = 0; j < NQ; ++j) acc[j] = acc[j] + rv * Sq[j][n];
    }
}

// The statistic of one spectrum, in the order include/nusi.h defines:
//     sum over c ascending from 0.0 of  mu_c - data_c * log(mu_c)   (mu_c where data_c == 0),  log = nm::log's body,
// serial in one lane over the spectrum's row of the block's mu in LDS.
__device__ __forceinline__ double det_poisson(const double* row, const double* __restrict__ data, int C)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int k = 0; k < C; ++k) {
        const double m = row[k], d = data[k];
        double term = m;
        if (d != 0.0) {
            const double p = d * nm::log_i(m);
            term = m - p;
        }
        s = s + term;
    }
    return s;
}

// ---------------------------------------------------------------------------
// k_detector_events: spectra on folded response matrices (nusi_plan_response_events):
//     mu = scale[q] * acc + bg[c],  acc = det_front's,  and with data  nll[t][q] = det_poisson(mu).
// The block's mu in LDS: QB rows of C | 1 doubles; the largest over C = 1 .. NUSI_DETECTOR_BINS_MAX is at C = 2
// (512 x 3).
// ---------------------------------------------------------------------------
constexpr int ev_lds_doubles(int C) { return det_qb(ceil_log2(C), kEvQ) * (C | 1); }
constexpr int ev_lds_max()
{
    int m = 0;
    for (int C = 1; C <= NUSI_DETECTOR_BINS_MAX; ++C) m = ev_lds_doubles(C) > m ? ev_lds_doubles(C) : m;
    return m;
}
static_assert(ev_lds_max() <= kEvLds, "k_detector_events: the block's mu does not fit smu[]");

__global__ __launch_bounds__(kEvThreads) void k_detector_events(const double* __restrict__ R, const double* __restrict__ S,
                                                                const double* __restrict__ scale,
                                                                const double* __restrict__ data,
                                                                const double* __restrict__ bg, double* __restrict__ mu,
                                                                double* __restrict__ nll, int M, int C, int lgC, int Q)
{
#pragma clang fp contract(off)
    __shared__ double smu[kEvLds];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = det_qb(lgC, kEvQ), qb0 = (int)blockIdx.y * QB, q0 = qb0 + grp * kEvQ;
    const int cc = c < C ? c : C - 1, Cs = C | 1;
    double acc[kEvQ];
    det_front(R, S, t, M, C, cc, q0, Q, acc);
    const double b = bg[cc];
#pragma unroll
    for (int j = 0; j < kEvQ; ++j) {
        const int q = q0 + j;
        const double sa = (scale ? scale[q < Q ? q : Q - 1] : 1.0) * acc[j];
        const double m = sa + b;
        if (c < C) {
            smu[(grp * kEvQ + j) * Cs + c] = m;
            if (mu && q < Q) mu[((size_t)t * Q + q) * C + c] = m;
        }
    }
    if (!nll) return;   // (uniform)
    __syncthreads();
    // (a block owns QB spectra -- 1024 at C = 1, 512 at C = 2 -- on kEvThreads threads: a strided loop)
    for (int i = tid; i < QB && qb0 + i < Q; i += kEvThreads) {
        const int q = qb0 + i;
        nll[(size_t)t * Q + q] = det_poisson(smu + i * Cs, data, C);
    }
}

hipError_t launch_detector_events(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* scale,
                                  const double* data, const double* bg, int C, double* mu, double* nll, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0) return hipSuccess;
    const DetGeom ge(C, kEvQ, ntab, Q);
    hipLaunchKernelGGL(k_detector_events, ge.grid, dim3(kEvThreads), 0, s, R, S, scale, data, bg, mu, nll, g.T + 1, C, ge.lg, Q);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_detector_profile: the statistic profiled over the flux normalisation (nusi_plan_response_profile): per (t, q) the
// a >= 0 minimising -ln L(a s + B | data), by the iteration include/nusi.h defines, on k_detector_events' block shape:
// four accumulators s_c per lane.  The sums over c are xor-butterflies over a group's lanes: stage k adds the partner
// across 2^k lanes, which is the tree of adjacent pairs, and every lane ends with the same bits (a + b = b + a).
// Strides 1 and 2 are DPP quad permutations; 4 and 8 are the row's half mirror and mirror (the lanes of a quad, or of
// eight, already hold one value, so lane 7 - i, or 15 - i, stands for lane i ^ 4, or i ^ 8); 16 is ds_swizzle, 32 a
// bpermute.  No LDS round trip and no barrier inside the iteration.  The iterate a is uniform over a group's lanes by
// construction; the four chains of a lane run interleaved (the fp64 divisions of one behind the others); a chain that
// has stopped keeps its a, and the wave leaves the loop when no chain of any of its groups runs, so the butterflies
// always run with full exec.  Padding lanes (c >= C) carry s = data = B = 0 and are inactive bins.
// ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double det_dpp(double x)
{
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double det_swizzle16(double x)   // lane i ^ 16: bit mode, and 0x1f, or 0, xor 0x10
{
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(x), 0x401f);
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(x), 0x401f);
    return __hiloint2double(hi, lo);
}
// v[k] = op over the 2^lgC lanes of the group, for NV values at once (lgC is uniform)
template <int NV, class Op>
__device__ __forceinline__ void det_butterfly(double (&v)[NV], int lgC, Op op)
{
    if (lgC > 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = op(v[k], det_dpp<0xb1>(v[k]));    // quad_perm [1, 0, 3, 2]
    if (lgC > 1)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = op(v[k], det_dpp<0x4e>(v[k]));    // quad_perm [2, 3, 0, 1]
    if (lgC > 2)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = op(v[k], det_dpp<0x141>(v[k]));   // row_half_mirror
    if (lgC > 3)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = op(v[k], det_dpp<0x140>(v[k]));   // row_mirror
    if (lgC > 4)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = op(v[k], det_swizzle16(v[k]));
    if (lgC > 5)
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = op(v[k], __shfl_xor(v[k], 32));
}

__global__ __launch_bounds__(kEvThreads) void k_detector_profile(const double* __restrict__ R, const double* __restrict__ S,
                                                                 const double* __restrict__ data,
                                                                 const double* __restrict__ bg, double* __restrict__ ahat,
                                                                 double* __restrict__ nll, double* __restrict__ mu,
                                                                 int* __restrict__ status, int M, int C, int lgC, int Q)
{
#pragma clang fp contract(off)
    __shared__ double smu[kEvLds];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = det_qb(lgC, kEvQ), qb0 = (int)blockIdx.y * QB, q0 = qb0 + grp * kEvQ;
    const int cc = c < C ? c : C - 1, Cs = C | 1;
    double s[kEvQ];
    det_front(R, S, t, M, C, cc, q0, Q, s);
    const bool in = c < C;
    const double b = in ? bg[cc] : 0.0, d = in ? data[cc] : 0.0;
    // the group's lanes in a ballot (written out here and in k_detector_fit: a shared helper moved both kernels' code)
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto max = [](double x, double y) { return y > x ? y : x; };
    double S1[kEvQ], a[kEvQ];
    bool act[kEvQ], run[kEvQ];
    int st[kEvQ];
#pragma unroll
    for (int j = 0; j < kEvQ; ++j) {
        if (!in) s[j] = 0.0;
        S1[j] = s[j];
        act[j] = d > 0.0 && s[j] > 0.0;
    }
    det_butterfly(S1, lgC, add);
#pragma unroll
    for (int j = 0; j < kEvQ; ++j) {
        run[j] = S1[j] != 0.0 && (__ballot(act[j]) & gmask) != 0;
        st[j] = run[j] ? 0 : NUSI_FIT_FLAT;
        const double x0 = d / S1[j], x1 = b / s[j];
        a[j] = act[j] ? x0 - x1 : 0.0;
    }
#include "nusi_profile_chain4.inc"
#pragma unroll
    for (int j = 0; j < kEvQ; ++j) {
        const int q = q0 + j;
        double m = a[j] * s[j];
        m = m + b;
        if ((__ballot(in && d > 0.0 && m == 0.0) & gmask) != 0) st[j] |= NUSI_FIT_INFINITE;
        if (in) {
            smu[(grp * kEvQ + j) * Cs + c] = m;
            if (mu && q < Q) mu[((size_t)t * Q + q) * C + c] = m;
        }
        if (c == 0 && q < Q) {
            ahat[(size_t)t * Q + q] = a[j];
            if (status) status[(size_t)t * Q + q] = st[j];
        }
    }
    if (!nll) return;   // (uniform)
    __syncthreads();
    for (int i = tid; i < QB && qb0 + i < Q; i += kEvThreads) {
        const int q = qb0 + i;
        nll[(size_t)t * Q + q] = det_poisson(smu + i * Cs, data, C);
    }
}

hipError_t launch_detector_profile(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                                   const double* bg, int C, double* ahat, double* nll, double* mu, int* status,
                                   hipStream_t s)
{
    if (ntab <= 0 || Q <= 0) return hipSuccess;
    const DetGeom ge(C, kEvQ, ntab, Q);
    hipLaunchKernelGGL(k_detector_profile, ge.grid, dim3(kEvThreads), 0, s, R, S, data, bg, ahat, nll, mu, status, g.T + 1, C,
                       ge.lg, Q);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_detector_fit<NC>: the statistic minimised over NC = 1 + K non-negative normalisations at once -- the signal's and
// those of K background templates under Gaussian priors (nusi_plan_response_fit), by the damped Newton iteration
// include/nusi.h defines.  Lanes sit on (c, ONE spectrum): a chain holds NC iterates, NC candidates and NC directions
// and a round's NC + NC (NC + 1) / 2 sums, which does not fit several times into 128 registers.  A round evaluates the
// gradient's and the Hessian's sums over the bins at the chain's evaluation point -- the start, or a candidate
// theta + t p -- in ONE det_butterfly over the group's lanes;
// everything after it (accepting the candidate, the free set, the stop, the L D L^T solve, the step length) uses only
// those sums and values uniform over the group, so every lane of a group does it redundantly and theta stays uniform
// by construction.  Groups stop after different numbers of rounds: a stopped chain keeps its theta and skips the
// logic, the wave leaves the loop when none of its chains runs, and the butterfly always runs with full exec.  The
// priors (pm, pw: NC entries, the signal's zeros in front) are uniform over the grid and live in scalar registers.
// LDS: per spectrum of the block its mu and theta_1 .. theta_K, for the statistic and its penalties.
// ---------------------------------------------------------------------------
constexpr int fit_row(int C, int NC) { return (C + NC - 1) | 1; }
constexpr int fit_lds_doubles(int C, int NC) { return det_qb(ceil_log2(C), 1) * fit_row(C, NC); }
constexpr int fit_lds_max(int NC)
{
    int m = 0;
    for (int C = 1; C <= NUSI_DETECTOR_BINS_MAX; ++C) m = fit_lds_doubles(C, NC) > m ? fit_lds_doubles(C, NC) : m;
    return m;
}

struct FitPrior {
    double m[NUSI_FIT_TEMPLATES_MAX + 1], w[NUSI_FIT_TEMPLATES_MAX + 1];
};
// a call's priors (pm, pw: K entries) as the kernels take them: template j's in slot j, zeros in the signal's slot and
// behind slot K
static FitPrior fit_prior(int K, const double* pm, const double* pw)
{
    FitPrior pr;
    for (int j = 0; j <= NUSI_FIT_TEMPLATES_MAX; ++j) {
        pr.m[j] = (j >= 1 && j <= K) ? pm[j - 1] : 0.0;
        pr.w[j] = (j >= 1 && j <= K) ? pw[j - 1] : 0.0;
    }
    return pr;
}
// the stop rules' kappa(C, K) u and kappa_lambda(C, K) u of include/nusi.h, lg = ceil_log2(C) (the conditional fit's
// den is as long as the fit's: the same kappa)
static double fit_ku(int lg, int K) { return (double)(2 * (lg + K) + 18) * 0x1p-53; }
static double fit_klu(int lg, int K) { return (double)(2 * (lg + K) + 14) * 0x1p-53; }

template <int NC>
__global__ __launch_bounds__(kEvThreads) void k_detector_fit(const double* __restrict__ R, const double* __restrict__ S,
                                                             const double* __restrict__ data,
                                                             const double* __restrict__ bg, const double* __restrict__ T,
                                                             const FitPrior pr, const double ku,
                                                             double* __restrict__ theta, double* __restrict__ nll,
                                                             double* __restrict__ mu, int* __restrict__ status, int M,
                                                             int C, int lgC, int Q)
{
#pragma clang fp contract(off)
    constexpr int NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major)
    __shared__ double smu[fit_lds_max(NC)];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, qb0 = (int)blockIdx.y * QB, q = qb0 + grp;
    const int cc = c < C ? c : C - 1, RS = fit_row(C, NC);
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)(q < Q ? q : Q - 1) * M;
    const bool in = c < C;
    double X[NC];
    {
        double s0 = 0.0;
#pragma unroll 4
        for (int n = 1; n < M; ++n) s0 = s0 + Rt[(size_t)n * C] * Sq[n];
        X[0] = in ? s0 : 0.0;
    }
#pragma unroll
    for (int j = 1; j < NC; ++j) X[j] = in ? T[(size_t)(j - 1) * C + cc] : 0.0;
    const double b = in ? bg[cc] : 0.0, d = in ? data[cc] : 0.0;
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto min = [](double x, double y) { return y < x ? y : x; };
    auto any = [&](bool x) { return (__ballot(x) & gmask) != 0; };

    double S1[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) S1[j] = X[j];
    det_butterfly(S1, lgC, add);
#define FN_NSIG 1
#include "nusi_fit_newton.inc"
#undef FN_NSIG
    if (in) {
        smu[grp * RS + c] = m;
        if (mu && q < Q) mu[((size_t)t * Q + q) * C + c] = m;
    }
    if (c == 0) {
#pragma unroll
        for (int j = 1; j < NC; ++j) smu[grp * RS + C + j - 1] = th[j];
        if (q < Q) {
#pragma unroll
            for (int j = 0; j < NC; ++j) theta[((size_t)t * Q + q) * NC + j] = th[j];
            if (status) status[(size_t)t * Q + q] = st;
        }
    }
    if (!nll) return;   // (uniform)
    __syncthreads();
    // (a block owns QB <= kEvThreads spectra)
    if (tid < QB && qb0 + tid < Q) {
        constexpr int NP = NC;
#include "nusi_fit_statistic.inc"
        nll[(size_t)t * Q + qb0 + tid] = sum;
    }
}

hipError_t launch_detector_fit(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                               const double* bg, int C, int K, const double* T, const double* pm, const double* pw,
                               double* theta, double* nll, double* mu, int* status, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0) return hipSuccess;
    const DetGeom ge(C, 1, ntab, Q);
    const FitPrior pr = fit_prior(K, pm, pw);
    const double ku = fit_ku(ge.lg, K);
    const dim3 grid = ge.grid, block(kEvThreads);
    const int M = g.T + 1;
    switch (K) {
    case 1: hipLaunchKernelGGL((k_detector_fit<2>), grid, block, 0, s, R, S, data, bg, T, pr, ku, theta, nll, mu, status, M, C, ge.lg, Q); break;
    case 2: hipLaunchKernelGGL((k_detector_fit<3>), grid, block, 0, s, R, S, data, bg, T, pr, ku, theta, nll, mu, status, M, C, ge.lg, Q); break;
    case 3: hipLaunchKernelGGL((k_detector_fit<4>), grid, block, 0, s, R, S, data, bg, T, pr, ku, theta, nll, mu, status, M, C, ge.lg, Q); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_components_fit<J, NC>: the fit with J = 2 .. 3 SIGNAL components in front of the K = NC - J templates
// (nusi_plan_response_fit_components): every (table, spectrum) brings J rows of its own, R3[t][j], and all NC
// normalisations float, non-negative.  It has k_detector_fit's shape -- lanes on (c, one spectrum), one det_butterfly of
// the round's NC + NC (NC + 1) / 2 sums (27 at NC = 6), everything behind it redundant on a group's lanes, no LDS and no
// barrier inside the iteration -- and its text: nusi_fit_newton.inc with FN_NSIG = J, which makes the liveness rule and
// the FLAT / BOUNDARY flags run over the J signal components and leaves everything else as it is.  The front half loads
// S[q][n] once per n and J values R3[t][j][n][c] into J accumulators, each in events' order.  The priors arrive as the
// fit's FitPrior (template i in slot i); pr below shifts them behind the signal components' compile-time zeros.
// LDS: a row per spectrum of the block, fit_row(C, NC) doubles: its mu and theta_1 .. theta_{NC-1} -- the signal
// components behind the first ride along so that nusi_fit_statistic.inc serves as it is (their weights are 0: no term).
// NC = 5 and 6 do not fit the 128 registers of four waves per SIMD: those instances ask for three and two.
// ---------------------------------------------------------------------------
constexpr int comp_waves(int NC) { return NC <= 4 ? 4 : NC == 5 ? 3 : 2; }

template <int J, int NC>
__global__ __launch_bounds__(kEvThreads) __attribute__((amdgpu_waves_per_eu(comp_waves(NC))))
void k_components_fit(const double* __restrict__ R3, const double* __restrict__ S, const double* __restrict__ data,
                      const double* __restrict__ bg, const double* __restrict__ T, const FitPrior tp, const double ku,
                      double* __restrict__ theta, double* __restrict__ nll, double* __restrict__ mu,
                      int* __restrict__ status, int M, int C, int lgC, int Q)
{
#pragma clang fp contract(off)
    static_assert(J >= 2 && J <= NUSI_FIT_SIGNALS_MAX && NC >= J && NC - J <= NUSI_FIT_TEMPLATES_MAX, "k_components_fit: J signal components and NC - J templates");
    constexpr int NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major)
    __shared__ double smu[fit_lds_max(NC)];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, qb0 = (int)blockIdx.y * QB, q = qb0 + grp;
    const int cc = c < C ? c : C - 1, RS = fit_row(C, NC);
    const double* __restrict__ Rt = R3 + (size_t)t * J * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)(q < Q ? q : Q - 1) * M;
    const bool in = c < C;
    double X[NC];
    {
        double s0[J];
#pragma unroll
        for (int j = 0; j < J; ++j) s0[j] = 0.0;
#pragma unroll 4
        for (int n = 1; n < M; ++n) {
            const double sv = Sq[n];
#pragma unroll
            for (int j = 0; j < J; ++j) s0[j] = s0[j] + Rt[((size_t)j * M + n) * C] * sv;
        }
#pragma unroll
        for (int j = 0; j < J; ++j) X[j] = in ? s0[j] : 0.0;
    }
#pragma unroll
    for (int j = J; j < NC; ++j) X[j] = in ? T[(size_t)(j - J) * C + cc] : 0.0;
    struct {
        double m[NC], w[NC];
    } pr;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        pr.m[j] = j < J ? 0.0 : tp.m[j < J ? 0 : j - J + 1];
        pr.w[j] = j < J ? 0.0 : tp.w[j < J ? 0 : j - J + 1];
    }
    const double b = in ? bg[cc] : 0.0, d = in ? data[cc] : 0.0;
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto min = [](double x, double y) { return y < x ? y : x; };
    auto any = [&](bool x) { return (__ballot(x) & gmask) != 0; };

    double S1[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) S1[j] = X[j];
    det_butterfly(S1, lgC, add);
#define FN_NSIG J
#include "nusi_fit_newton.inc"
#undef FN_NSIG
    if (in) {
        smu[grp * RS + c] = m;
        if (mu && q < Q) mu[((size_t)t * Q + q) * C + c] = m;
    }
    if (c == 0) {
#pragma unroll
        for (int j = 1; j < NC; ++j) smu[grp * RS + C + j - 1] = th[j];
        if (q < Q) {
#pragma unroll
            for (int j = 0; j < NC; ++j) theta[((size_t)t * Q + q) * NC + j] = th[j];
            if (status) status[(size_t)t * Q + q] = st;
        }
    }
    if (!nll) return;   // (uniform)
    __syncthreads();
    // (a block owns QB <= kEvThreads spectra)
    if (tid < QB && qb0 + tid < Q) {
        constexpr int NP = NC;
#include "nusi_fit_statistic.inc"
        nll[(size_t)t * Q + qb0 + tid] = sum;
    }
}

// (J = 2 .. 3, K = 0 .. NUSI_FIT_TEMPLATES_MAX: eight instances; ku = kappa u with J - 1 + K in kappa, one more product
// in den per further signal component)
hipError_t launch_components_fit(const GridDev& g, const double* R3, int ntab, int J, const double* S, int Q,
                                 const double* data, const double* bg, int C, int K, const double* T, const double* pm,
                                 const double* pw, double* theta, double* nll, double* mu, int* status, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0) return hipSuccess;
    const DetGeom ge(C, 1, ntab, Q);
    const FitPrior pr = fit_prior(K, pm, pw);
    const double ku = fit_ku(ge.lg, J - 1 + K);
    const dim3 grid = ge.grid, block(kEvThreads);
    const int M = g.T + 1;
#define NUSI_COMP_FIT(JJ, KK) \
    case (JJ) * 4 + (KK): \
        hipLaunchKernelGGL((k_components_fit<JJ, JJ + KK>), grid, block, 0, s, R3, S, data, bg, T, pr, ku, theta, nll, mu, status, M, C, ge.lg, Q); \
        break;
    switch (J * 4 + K) {
        NUSI_COMP_FIT(2, 0)
        NUSI_COMP_FIT(2, 1)
        NUSI_COMP_FIT(2, 2)
        NUSI_COMP_FIT(2, 3)
        NUSI_COMP_FIT(3, 0)
        NUSI_COMP_FIT(3, 1)
        NUSI_COMP_FIT(3, 2)
        NUSI_COMP_FIT(3, 3)
    default: return hipErrorInvalidValue;
    }
#undef NUSI_COMP_FIT
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The ensemble kernels (nusi_plan_response_ensemble): P data sets data[p][C] against every table and spectrum, and of
// each (p, t) only the BEST spectrum's record (q, nll, theta, status) under the key include/nusi.h defines,
// (isnan(nll), nll, q) compared lexicographically.  k_ensemble_profile runs k_detector_profile's iteration (no
// templates, theta = ahat), k_ensemble_fit<NC> k_detector_fit<NC>'s, on those kernels' block shapes: the iterations are
// those kernels' own text, shared by #include (nusi_profile_chain4.inc, nusi_fit_newton.inc) and not by a helper, which
// moved the existing kernels' code objects and their timing.  det_front, det_poisson and
// det_butterfly are the existing helpers, called as they are.
//
// Grid (tables, q-slices, p-slices).  A block walks the spectrum blocks qb of its q-slice and, per spectrum block, the
// data sets of its p-slice: the front half s = sum_n R S, the sums S1 and the templates' liveness do not depend on the
// data and are computed once per spectrum block and kept in registers; per data set only d, act, live[0], sup, D0,
// dmin, the start and the iteration run.
//
// Per data set: the lanes write their spectrum's row -- the statistic's terms mu_c - data_c log(mu_c) [C], each formed
// on its bin's own lane (the same operations as the serial loops of det_poisson and k_detector_fit, so the same bits;
// one log per lane instead of C in a row on one lane of eight), theta [W], the status word (as a double: exact) --
// to LDS, ONE barrier, the terms' sum in the defined serial order by one lane per spectrum, a reduction under the key
// over each wave (xor shuffles) and lane 0 of each wave writes its wave's record to LDS.  Rows and wave records are
// double-buffered on the data set's parity: the wave records of data set i are merged by thread 0 after the barrier of
// data set i + 1 (after the last: one more barrier), which makes them visible and is passed by every lane only after it
// has read its rows of data set i; buffer i & 1 is next written for data set i + 2, behind that barrier.  Thread 0
// merges into the running record of (p, t) in global memory, which no other block and no other thread touches: for the
// q-slice's first spectrum block it writes, afterwards it reads, compares and writes.  No atomics.  With one q-slice
// the running records are the call's outputs; with more they are the plan's scratch [q-slice][P][ntab] and
// k_ensemble_best merges the slices.  The key is a total order on the (distinct) q, so every tree gives the same record.
//
// LDS: 2 det_qb(lgC, per) rows of ens_row(C, W) = (C + W + 1) | 1 doubles, sized for the largest C, and EnsWin<W>:
// 8 (2 ens_rows_max(per, W) + 8 (W + 2)) bytes.
// ---------------------------------------------------------------------------
struct EnsOut {
    int* q;          // records [slice][P][ntab]; theta [..][W]
    double* nll;
    double* theta;   // (theta, status: NULL = not wanted; never NULL in the scratch)
    int* status;
    size_t slice;    // records per q-slice; 0: one q-slice, the records are the call's outputs
};

constexpr int kEnsWaves = kEvThreads >> 6;
constexpr int ens_row(int C, int W) { return (C + W + 1) | 1; }
constexpr int ens_rows_max(int per, int W)
{
    int m = 0;
    for (int C = 1; C <= NUSI_DETECTOR_BINS_MAX; ++C) {
        const int n = det_qb(ceil_log2(C), per) * ens_row(C, W);
        m = n > m ? n : m;
    }
    return m;
}

template <int W>
struct EnsWin {   // the waves' records of a data set, double-buffered
    double nll[2][kEnsWaves], th[2][kEnsWaves][W];
    int q[2][kEnsWaves], st[2][kEnsWaves];
};

// is record a better than record b?  (isnan(nll), nll, q) ascending; a wave without a spectrum carries (NaN, INT_MAX)
__device__ __forceinline__ bool ens_better(double an, int aq, double bn, int bq)
{
    const bool na = an != an, nb = bn != bn;
    if (na != nb) return nb;
    if (!na && an != bn) return an < bn;
    return aq < bq;
}

// the wave's best (nll, q) on every lane; then lane 0 writes the wave's record from the winner's row
template <int W>
__device__ __forceinline__ void ens_wave_record(double n, int q, EnsWin<W>& win, int buf, int wave, const double* rows,
                                                int RS, int C, int qb0)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double on = __shfl_xor(n, m);
        const int oq = __shfl_xor(q, m);
        if (ens_better(on, oq, n, q)) {
            n = on;
            q = oq;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        win.nll[buf][wave] = n;
        win.q[buf][wave] = q;
        if (q != INT_MAX) {
            const double* row = rows + (size_t)(q - qb0) * RS + C;
#pragma unroll
            for (int j = 0; j < W; ++j) win.th[buf][wave][j] = row[j];
            win.st[buf][wave] = (int)row[W];
        }
    }
}

// thread 0: the nw wave records of buffer buf into the running record r (fresh: the record holds nothing yet)
template <int W>
__device__ __forceinline__ void ens_commit(const EnsWin<W>& win, int buf, int nw, const EnsOut& o, size_t r, bool fresh)
{
    int k = 0;
    for (int i = 1; i < nw; ++i)
        if (ens_better(win.nll[buf][i], win.q[buf][i], win.nll[buf][k], win.q[buf][k])) k = i;
    if (!fresh && !ens_better(win.nll[buf][k], win.q[buf][k], o.nll[r], o.q[r])) return;
    o.nll[r] = win.nll[buf][k];
    o.q[r] = win.q[buf][k];
    if (o.theta)
#pragma unroll
        for (int j = 0; j < W; ++j) o.theta[r * W + j] = win.th[buf][k][j];
    if (o.status) o.status[r] = win.st[buf][k];
}

// a block's share of n items among the nparts blocks along one grid axis: [lo, hi), balanced, never empty for
// nparts <= n
__device__ __forceinline__ void ens_share(int n, int part, int nparts, int& lo, int& hi)
{
    lo = (int)((long long)n * part / nparts);
    hi = (int)((long long)n * (part + 1) / nparts);
}

__global__ __launch_bounds__(kEvThreads) void k_ensemble_profile(const double* __restrict__ R, const double* __restrict__ S,
                                                                 const double* __restrict__ data,
                                                                 const double* __restrict__ bg, const EnsOut o, int M, int C,
                                                                 int lgC, int Q, int P)
{
#pragma clang fp contract(off)
    constexpr int kRows = ens_rows_max(kEvQ, 1);
    __shared__ double srow[2 * kRows];
    __shared__ EnsWin<1> win;
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x, ntab = (int)gridDim.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = det_qb(lgC, kEvQ), nqb = (Q + QB - 1) / QB;
    const int cc = c < C ? c : C - 1, RS = ens_row(C, 1);
    const int nw = QB < kEvThreads ? (QB + 63) >> 6 : kEnsWaves;   // the waves that hold a spectrum's statistic
    int b0, b1, p0, p1;
    ens_share(nqb, (int)blockIdx.y, (int)gridDim.y, b0, b1);
    ens_share(P, (int)blockIdx.z, (int)gridDim.z, p0, p1);
    const bool in = c < C;
    const double b = in ? bg[cc] : 0.0;
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto max = [](double x, double y) { return y > x ? y : x; };
    int it = 0;
    size_t rprev = 0;
    bool fprev = false;
    for (int qb = b0; qb < b1; ++qb) {
        const int qb0 = qb * QB, q0 = qb0 + grp * kEvQ;
        double s[kEvQ], S1[kEvQ];
        det_front(R, S, t, M, C, cc, q0, Q, s);
#pragma unroll
        for (int j = 0; j < kEvQ; ++j) {
            if (!in) s[j] = 0.0;
            S1[j] = s[j];
        }
        det_butterfly(S1, lgC, add);
        for (int p = p0; p < p1; ++p, ++it) {
            const double* __restrict__ dat = data + (size_t)p * C;
            const double d = in ? dat[cc] : 0.0;
            double a[kEvQ];
            bool act[kEvQ], run[kEvQ];
            int st[kEvQ];
#pragma unroll
            for (int j = 0; j < kEvQ; ++j) {
                act[j] = d > 0.0 && s[j] > 0.0;
                run[j] = S1[j] != 0.0 && (__ballot(act[j]) & gmask) != 0;
                st[j] = run[j] ? 0 : NUSI_FIT_FLAT;
                const double x0 = d / S1[j], x1 = b / s[j];
                a[j] = act[j] ? x0 - x1 : 0.0;
            }
#include "nusi_profile_chain4.inc"
            const int buf = it & 1;
            double* rows = srow + buf * kRows;
#pragma unroll
            for (int j = 0; j < kEvQ; ++j) {
                double m = a[j] * s[j];
                m = m + b;
                if ((__ballot(in && d > 0.0 && m == 0.0) & gmask) != 0) st[j] |= NUSI_FIT_INFINITE;
                double term = m;   // det_poisson's term of (spectrum, c), on the bin's own lane
                if (d != 0.0) {
                    const double pl = d * nm::log_i(m);
                    term = m - pl;
                }
                double* row = rows + (grp * kEvQ + j) * RS;
                if (in) row[c] = term;
                if (c == 0) {
                    row[C] = a[j];
                    row[C + 1] = (double)st[j];
                }
            }
            // --- the statistic and the block's best record ---
            __syncthreads();
            if (it > 0 && tid == 0) ens_commit(win, buf ^ 1, nw, o, rprev, fprev);
            rprev = (size_t)blockIdx.y * o.slice + (size_t)p * ntab + t;
            fprev = qb == b0;
            if ((tid >> 6) < nw) {
                double bn = __builtin_nan("");
                int bq = INT_MAX;
                // (a block owns QB spectra -- 1024 at C = 1 -- on kEvThreads threads: ascending i, so ascending q)
                for (int i = tid; i < QB && qb0 + i < Q; i += kEvThreads) {
                    double n = 0.0;   // det_poisson's sum: the terms ascending in c, from 0.0
                    for (int k = 0; k < C; ++k) n = n + rows[i * RS + k];
                    if (ens_better(n, qb0 + i, bn, bq)) {
                        bn = n;
                        bq = qb0 + i;
                    }
                }
                ens_wave_record(bn, bq, win, buf, tid >> 6, rows, RS, C, qb0);
            }
        }
    }
    __syncthreads();
    if (it > 0 && tid == 0) ens_commit(win, (it - 1) & 1, nw, o, rprev, fprev);
}

// Registers: the loop over the data sets keeps more alive around the iteration than k_detector_fit does (the row
// pointers, the lane's place, what the compiler hoists out of the loop), so the allocator is told the aim: four waves
// per SIMD (128 registers) for NC = 2 and 3.  NC = 4 -- k_detector_fit<4> itself stands at 127 -- does not get there
// without scratch (14 registers spilled); it is held to three waves (168) instead and takes 164, no scratch.
template <int NC>
__global__ __launch_bounds__(kEvThreads) __attribute__((amdgpu_waves_per_eu(NC == 4 ? 3 : 4))) void k_ensemble_fit(const double* __restrict__ R, const double* __restrict__ S,
                                                             const double* __restrict__ data,
                                                             const double* __restrict__ bg, const double* __restrict__ T,
                                                             const FitPrior pr, const double ku, const EnsOut o, int M,
                                                             int C, int lgC, int Q, int P)
{
#pragma clang fp contract(off)
    constexpr int NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major)
    constexpr int kRows = ens_rows_max(1, NC);
    __shared__ double srow[2 * kRows];
    __shared__ EnsWin<NC> win;
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x, ntab = (int)gridDim.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, nqb = (Q + QB - 1) / QB;
    const int cc = c < C ? c : C - 1, RS = ens_row(C, NC);
    const int nw = (QB + 63) >> 6;   // the waves that hold a spectrum's statistic
    int b0, b1, p0, p1;
    ens_share(nqb, (int)blockIdx.y, (int)gridDim.y, b0, b1);
    ens_share(P, (int)blockIdx.z, (int)gridDim.z, p0, p1);
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const bool in = c < C;
    double X[NC];
#pragma unroll
    for (int j = 1; j < NC; ++j) X[j] = in ? T[(size_t)(j - 1) * C + cc] : 0.0;
    const double b = in ? bg[cc] : 0.0;
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto min = [](double x, double y) { return y < x ? y : x; };
    auto any = [&](bool x) { return (__ballot(x) & gmask) != 0; };
    int it = 0;
    size_t rprev = 0;
    bool fprev = false;
    for (int qb = b0; qb < b1; ++qb) {
        const int qb0 = qb * QB, q = qb0 + grp;
        const double* __restrict__ Sq = S + (size_t)(q < Q ? q : Q - 1) * M;
        {
            double s0 = 0.0;
#pragma unroll 4
            for (int n = 1; n < M; ++n) s0 = s0 + Rt[(size_t)n * C] * Sq[n];
            X[0] = in ? s0 : 0.0;
        }
        double S1[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) S1[j] = X[j];
        det_butterfly(S1, lgC, add);
        for (int pi = p0; pi < p1; ++pi, ++it) {
            const double* __restrict__ dat = data + (size_t)pi * C;
            const double d = in ? dat[cc] : 0.0;
#define FN_NSIG 1
#include "nusi_fit_newton.inc"
#undef FN_NSIG
            const int buf = it & 1;
            double* rows = srow + buf * kRows;
            double term = m;   // the statistic's term of (spectrum, c), on the bin's own lane
            if (d != 0.0) {
                const double pl = d * nm::log_i(m);
                term = m - pl;
            }
            if (in) rows[grp * RS + c] = term;
            if (c == 0) {
#pragma unroll
                for (int j = 0; j < NC; ++j) rows[grp * RS + C + j] = th[j];
                rows[grp * RS + C + NC] = (double)st;
            }
            // --- the statistic and the block's best record ---
            __syncthreads();
            if (it > 0 && tid == 0) ens_commit(win, buf ^ 1, nw, o, rprev, fprev);
            rprev = (size_t)blockIdx.y * o.slice + (size_t)pi * ntab + t;
            fprev = qb == b0;
            if ((tid >> 6) < nw) {
                double sum = __builtin_nan("");
                int bq = INT_MAX;
                // (a block owns QB <= kEvThreads spectra)
                if (tid < QB && qb0 + tid < Q) {
                    bq = qb0 + tid;
                    sum = 0.0;   // k_detector_fit's sum: the terms ascending in c, from 0.0, then the penalties
                    for (int k = 0; k < C; ++k) sum = sum + rows[tid * RS + k];
#pragma unroll
                    for (int j = 1; j < NC; ++j)
                        if (pr.w[j] > 0.0) {
                            const double dl = rows[tid * RS + C + j] - pr.m[j];
                            const double pen = ((0.5 * pr.w[j]) * dl) * dl;
                            sum = sum + pen;
                        }
                }
                ens_wave_record(sum, bq, win, buf, tid >> 6, rows, RS, C, qb0);
            }
        }
    }
    __syncthreads();
    if (it > 0 && tid == 0) ens_commit(win, (it - 1) & 1, nw, o, rprev, fprev);
}

// The q-slices' records [nslice][n] (n = P ntab) into the call's outputs, one thread per (p, t), slices ascending.
__global__ __launch_bounds__(kEvThreads) void k_ensemble_best(const EnsOut in, int nslice, size_t n, int W, const EnsOut o)
{
    const size_t r = (size_t)blockIdx.x * kEvThreads + threadIdx.x;
    if (r >= n) return;
    int k = 0;
    double bn = in.nll[r];
    int bq = in.q[r];
    for (int i = 1; i < nslice; ++i) {
        const double x = in.nll[(size_t)i * n + r];
        const int xq = in.q[(size_t)i * n + r];
        if (ens_better(x, xq, bn, bq)) {
            bn = x;
            bq = xq;
            k = i;
        }
    }
    const size_t src = (size_t)k * n + r;
    o.nll[r] = bn;
    o.q[r] = bq;
    if (o.theta)
        for (int j = 0; j < W; ++j) o.theta[r * W + j] = in.theta[src * W + j];
    if (o.status) o.status[r] = in.status[src];
}

size_t ensemble_record_bytes(int K) { return sizeof(double) * (2 + K) + 2 * sizeof(int); }

int ensemble_blocks(int C, int K, int Q)
{
    const DetGeom ge(C, K ? 1 : kEvQ, 1, Q);
    return (int)ge.grid.y;
}

hipError_t launch_detector_ensemble(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                                    int P, const double* bg, int C, int K, const double* T, const double* pm,
                                    const double* pw, int qslices, int pslices, void* scratch, int* oq, double* onll,
                                    double* otheta, int* ostatus, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0 || P <= 0) return hipSuccess;
    const DetGeom ge(C, K ? 1 : kEvQ, ntab, Q);
    if (qslices < 1 || qslices > (int)ge.grid.y || pslices < 1 || pslices > P || (qslices > 1 && !scratch))
        return hipErrorInvalidValue;
    const int W = 1 + K, M = g.T + 1;
    const size_t n = (size_t)P * ntab;
    const EnsOut out{oq, onll, otheta, ostatus, 0};
    EnsOut rec = out;
    if (qslices > 1) {   // the scratch: nll, theta, q, status, each [qslices][n]
        const size_t ns = (size_t)qslices * n;
        rec.nll = (double*)scratch;
        rec.theta = rec.nll + ns;
        rec.q = (int*)(rec.theta + ns * W);
        rec.status = rec.q + ns;
        rec.slice = n;
    }
    const dim3 grid((unsigned)ntab, (unsigned)qslices, (unsigned)pslices), block(kEvThreads);
    if (K == 0) {
        hipLaunchKernelGGL(k_ensemble_profile, grid, block, 0, s, R, S, data, bg, rec, M, C, ge.lg, Q, P);
    } else {
        const FitPrior pr = fit_prior(K, pm, pw);
        const double ku = fit_ku(ge.lg, K);
        switch (K) {
        case 1: hipLaunchKernelGGL((k_ensemble_fit<2>), grid, block, 0, s, R, S, data, bg, T, pr, ku, rec, M, C, ge.lg, Q, P); break;
        case 2: hipLaunchKernelGGL((k_ensemble_fit<3>), grid, block, 0, s, R, S, data, bg, T, pr, ku, rec, M, C, ge.lg, Q, P); break;
        case 3: hipLaunchKernelGGL((k_ensemble_fit<4>), grid, block, 0, s, R, S, data, bg, T, pr, ku, rec, M, C, ge.lg, Q, P); break;
        default: return hipErrorInvalidValue;
        }
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || qslices == 1) return e;
    const size_t nblk = (n + kEvThreads - 1) / kEvThreads;
    hipLaunchKernelGGL(k_ensemble_best, dim3((unsigned)nblk), block, 0, s, rec, qslices, n, W, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_conditional_fit<NC>: the statistic minimised over the NC = K templates' normalisations with the signal's scale HELD
// at a given a[q] >= 0 (nusi_plan_response_fit_fixed): the background-only fit at a = 0, and the inner problem of the
// statistic q(a) = 2 (min_theta f(a, theta) - min f) at any a.  It is k_detector_fit's damped Newton iteration on the
// components 1 .. K alone, on that kernel's block shape -- lanes on (c, ONE spectrum), a round's NC + NC (NC + 1) / 2
// sums in one det_butterfly, the logic after it redundant on a group's lanes, full exec in every butterfly -- with the
// signal's term a s_c held in den: den_c = a s_c, + theta_j T_jc (j ascending), + B_c, the fit's order, so the
// conditional mu at some theta has the bits the fit's mu has at (a, theta).  The rounds are a text of their own,
// nusi_conditional_newton.inc (shared with k_inject), operation for operation nusi_fit_newton.inc's on the free
// components, and the Newton direction inside both is one text, nusi_ldlt_solve.inc; arrays of the free components
// are indexed i = j - 1.  What differs is what include/nusi.h's text says differs: the support
// rule counts the held signal (a > 0 and s_c > 0), the start shares the counts among the live templates only, nothing
// is FLAT or BOUNDARY, and component 0 sets no ZERO bit.  LDS: k_detector_fit<1 + NC>'s, a row of mu [C] and
// theta_1 .. theta_K per spectrum of the block: fit_lds_max(NC + 1) doubles.
// ---------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(kEvThreads) void k_conditional_fit(const double* __restrict__ R, const double* __restrict__ S,
                                                                const double* __restrict__ scale,
                                                                const double* __restrict__ data,
                                                                const double* __restrict__ bg, const double* __restrict__ T,
                                                                const FitPrior pr, const double ku,
                                                                double* __restrict__ theta, double* __restrict__ nll,
                                                                double* __restrict__ mu, int* __restrict__ status, int M,
                                                                int C, int lgC, int Q)
{
#pragma clang fp contract(off)
    constexpr int NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major), j, k = 1 .. K
    __shared__ double smu[fit_lds_max(NC + 1)];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, qb0 = (int)blockIdx.y * QB, q = qb0 + grp;
    const int cc = c < C ? c : C - 1, RS = fit_row(C, NC + 1);
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)(q < Q ? q : Q - 1) * M;
    const bool in = c < C;
    double X0, X[NC];
    {
        double s0 = 0.0;
#pragma unroll 4
        for (int n = 1; n < M; ++n) s0 = s0 + Rt[(size_t)n * C] * Sq[n];
        X0 = in ? s0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) X[i] = in ? T[(size_t)i * C + cc] : 0.0;
    const double b = in ? bg[cc] : 0.0, d = in ? data[cc] : 0.0;
    const double a = scale[q < Q ? q : Q - 1];   // (uniform over the group)
    const double asig = a * X0;                  // the held term of den
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto min = [](double x, double y) { return y < x ? y : x; };
    auto any = [&](bool x) { return (__ballot(x) & gmask) != 0; };

    double S1[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) S1[i] = X[i];
    det_butterfly(S1, lgC, add);
    bool live[NC];
    bool sup = b > 0.0 || (a > 0.0 && X0 > 0.0);
    int nl = 0;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        live[i] = S1[i] > 0.0;
        sup = sup || (live[i] && X[i] > 0.0);
        nl += live[i] ? 1 : 0;
    }
    const bool act = d > 0.0 && sup;
    double dsum[1] = {act ? d : 0.0}, dmin[1] = {act ? d : 1.0};   // (1.0: dmin = min(1, the smallest active datum))
    det_butterfly(dsum, lgC, add);
    det_butterfly(dmin, lgC, min);
    const double D0 = dsum[0], dq = 0.0625 * (dmin[0] < 1.0 ? dmin[0] : 1.0);
    double th[NC], the[NC], pp[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const double x = D0 / ((double)nl * S1[i]);
        th[i] = live[i] ? x : 0.0;
        the[i] = th[i];
        pp[i] = 0.0;
    }
    double tt = 1.0;
    int st = 0, steps = 0, halv = 0, trials = 0;
    bool run = true, first = true, quad = false;
#define CF_N NC
#define CF_X(i) X[i]
#define CF_S1(i) S1[i]
#define CF_LIVE(i) live[i]
#include "nusi_conditional_newton.inc"
#undef CF_N
#undef CF_X
#undef CF_S1
#undef CF_LIVE
    double m = asig;
#pragma unroll
    for (int i = 0; i < NC; ++i) m = m + th[i] * X[i];
    m = m + b;
#pragma unroll
    for (int i = 0; i < NC; ++i)
        if (th[i] == 0.0) st |= NUSI_FIT_ZERO << (i + 1);
    if (any(in && d > 0.0 && m == 0.0)) st |= NUSI_FIT_INFINITE;
    st |= steps | ((halv < NUSI_FIT_TRIALS_MASK ? halv : NUSI_FIT_TRIALS_MASK) << NUSI_FIT_TRIALS_SHIFT);
    if (in) {
        smu[grp * RS + c] = m;
        if (mu && q < Q) mu[((size_t)t * Q + q) * C + c] = m;
    }
    if (c == 0) {
#pragma unroll
        for (int i = 0; i < NC; ++i) smu[grp * RS + C + i] = th[i];
        if (q < Q) {
            theta[((size_t)t * Q + q) * (NC + 1)] = a;
#pragma unroll
            for (int i = 0; i < NC; ++i) theta[((size_t)t * Q + q) * (NC + 1) + 1 + i] = th[i];
            if (status) status[(size_t)t * Q + q] = st;
        }
    }
    if (!nll) return;   // (uniform)
    __syncthreads();
    // (a block owns QB <= kEvThreads spectra)
    if (tid < QB && qb0 + tid < Q) {
        constexpr int NP = NC + 1;   // (NC counts the templates alone here)
#include "nusi_fit_statistic.inc"
        nll[(size_t)t * Q + qb0 + tid] = sum;
    }
}

hipError_t launch_conditional_fit(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* scale,
                                  const double* data, const double* bg, int C, int K, const double* T, const double* pm,
                                  const double* pw, double* theta, double* nll, double* mu, int* status, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0) return hipSuccess;
    const DetGeom ge(C, 1, ntab, Q);
    const FitPrior pr = fit_prior(K, pm, pw);
    const double ku = fit_ku(ge.lg, K);
    const dim3 grid = ge.grid, block(kEvThreads);
    const int M = g.T + 1;
    switch (K) {
    case 1: hipLaunchKernelGGL((k_conditional_fit<1>), grid, block, 0, s, R, S, scale, data, bg, T, pr, ku, theta, nll, mu, status, M, C, ge.lg, Q); break;
    case 2: hipLaunchKernelGGL((k_conditional_fit<2>), grid, block, 0, s, R, S, scale, data, bg, T, pr, ku, theta, nll, mu, status, M, C, ge.lg, Q); break;
    case 3: hipLaunchKernelGGL((k_conditional_fit<3>), grid, block, 0, s, R, S, scale, data, bg, T, pr, ku, theta, nll, mu, status, M, C, ge.lg, Q); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_interval<NC>: profile-likelihood limits on the signal's scale (nusi_plan_response_limit), NC = 1 + K = 1 .. 4, on
// k_detector_fit's block shape: lanes on (c, ONE spectrum), every sum over the bins a det_butterfly over the group's
// lanes, everything after it uniform over the group and done redundantly on its lanes.  Three parts:
//   the best fit   k_detector_fit<NC>'s iteration (NC = 1: k_detector_profile's, one chain a lane): those kernels' text,
//                  by #include (nusi_fit_newton.inc, nusi_profile_chain1.inc), so theta_hat, nll_hat and the word are
//                  those calls' bits;
//   the search     per side asked for, Newton's iteration in a on lambda(a) = delta / 2 (include/nusi.h): each outer step
//                  runs k_conditional_fit's iteration at the held a, started from the step before's theta (K = 0: one
//                  evaluation), with ONE sum more in the round's butterfly, S2_0 = tree(s_c w_c), which is the
//                  derivative g_0 = S1_0 - S2_0 by the envelope theorem; then lambda from ratios, one nm::log_i on the
//                  bin's own lane, and its magnitude in one butterfly of two.  Groups of a wave need different numbers
//                  of outer and inner steps: a stopped chain skips the logic, the wave leaves a loop when none of its
//                  chains runs, every butterfly runs with full exec.  No LDS and no barrier in here.  The text is
//                  nusi_search_setup.inc and, per side, nusi_search_side.inc, which k_toys_limit includes as well;
//   the records    lo, hi and the side words, then the best fit's statistic through LDS as k_detector_fit forms it (mu
//                  and theta_1 .. theta_K per spectrum of the block, one barrier, the serial sum of
//                  nusi_fit_statistic.inc): fit_lds_max(NC) doubles.
// Arrays of the K floated templates are indexed i = j - 1 and sized max(K, 1).
// ---------------------------------------------------------------------------
template <int NC>
__global__ __launch_bounds__(kEvThreads) void k_interval(const double* __restrict__ R, const double* __restrict__ S,
                                                         const double* __restrict__ data, const double* __restrict__ bg,
                                                         const double* __restrict__ T, const FitPrior pr, const double ku,
                                                         const double klu, const double delta, const int which,
                                                         double* __restrict__ lo, double* __restrict__ hi,
                                                         double* __restrict__ theta_hat, double* __restrict__ nll_hat,
                                                         int* __restrict__ status, int M, int C, int lgC, int Q)
{
#pragma clang fp contract(off)
    constexpr int KT = NC - 1, KA = KT > 0 ? KT : 1;
    __shared__ double smu[fit_lds_max(NC)];
    const int tid = (int)threadIdx.x, t = (int)blockIdx.x;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, qb0 = (int)blockIdx.y * QB, q = qb0 + grp;
    const int cc = c < C ? c : C - 1, RS = fit_row(C, NC);
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)(q < Q ? q : Q - 1) * M;
    const bool in = c < C;
    double X[NC];
    {
        double s0 = 0.0;
#pragma unroll 4
        for (int n = 1; n < M; ++n) s0 = s0 + Rt[(size_t)n * C] * Sq[n];
        X[0] = in ? s0 : 0.0;
    }
#pragma unroll
    for (int j = 1; j < NC; ++j) X[j] = in ? T[(size_t)(j - 1) * C + cc] : 0.0;
    const double b = in ? bg[cc] : 0.0, d = in ? data[cc] : 0.0;
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto min = [](double x, double y) { return y < x ? y : x; };
    auto any = [&](bool x) { return (__ballot(x) & gmask) != 0; };

    // ---- the best fit ------------------------------------------------------------------------------------------------
    double thh[NC], S1h[NC], muh;
    int sth;
    if constexpr (NC == 1) {
        double S1[1] = {X[0]};
        det_butterfly(S1, lgC, add);
#include "nusi_profile_chain1.inc"
        thh[0] = a[0];
        S1h[0] = S1[0];
        muh = m;
        sth = st;
    } else {
        constexpr int NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major)
        double S1[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) S1[j] = X[j];
        det_butterfly(S1, lgC, add);
#define FN_NSIG 1
#include "nusi_fit_newton.inc"
#undef FN_NSIG
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            thh[j] = th[j];
            S1h[j] = S1[j];
        }
        muh = m;
        sth = st;
    }

    // ---- the search --------------------------------------------------------------------------------------------------
#include "nusi_search_setup.inc"
#pragma unroll 1
    for (int side = 1; side >= 0; --side) {   // 1: the upper side, 0: the lower
#include "nusi_search_side.inc"
        if (c == 0 && q < Q) {
            double* out = upper ? hi : lo;
            if (out) out[(size_t)t * Q + q] = res;
            if (status) status[((size_t)t * Q + q) * 3 + (upper ? 2 : 1)] = word;
        }
    }

    // ---- the records of the best fit -------------------------------------------------------------------------------------
    if (in) smu[grp * RS + c] = muh;
    if (c == 0) {
#pragma unroll
        for (int j = 1; j < NC; ++j) smu[grp * RS + C + j - 1] = thh[j];
        if (q < Q) {
            if (theta_hat)
#pragma unroll
                for (int j = 0; j < NC; ++j) theta_hat[((size_t)t * Q + q) * NC + j] = thh[j];
            if (status) status[((size_t)t * Q + q) * 3] = sth;
        }
    }
    if (!nll_hat) return;   // (uniform)
    __syncthreads();
    // (a block owns QB <= kEvThreads spectra)
    if (tid < QB && qb0 + tid < Q) {
        constexpr int NP = NC;
#include "nusi_fit_statistic.inc"
        nll_hat[(size_t)t * Q + qb0 + tid] = sum;
    }
}

hipError_t launch_detector_limit(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                                 const double* bg, int C, int K, const double* T, const double* pm, const double* pw,
                                 double delta, int which, double* lo, double* hi, double* theta_hat, double* nll_hat,
                                 int* status, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0) return hipSuccess;
    const DetGeom ge(C, 1, ntab, Q);
    const FitPrior pr = fit_prior(K, pm, pw);
    const double ku = fit_ku(ge.lg, K);
    const double klu = fit_klu(ge.lg, K);
    const dim3 grid = ge.grid, block(kEvThreads);
    const int M = g.T + 1;
    switch (K) {
    case 0: hipLaunchKernelGGL((k_interval<1>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, lo, hi, theta_hat, nll_hat, status, M, C, ge.lg, Q); break;
    case 1: hipLaunchKernelGGL((k_interval<2>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, lo, hi, theta_hat, nll_hat, status, M, C, ge.lg, Q); break;
    case 2: hipLaunchKernelGGL((k_interval<3>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, lo, hi, theta_hat, nll_hat, status, M, C, ge.lg, Q); break;
    case 3: hipLaunchKernelGGL((k_interval<4>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, lo, hi, theta_hat, nll_hat, status, M, C, ge.lg, Q); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_toys_limit<NC>: the limits of P data sets on one front half (nusi_plan_response_ensemble_limit), NC = 1 + K =
// 1 .. 4, on k_interval<NC>'s block shape.  (The names of the two kernels of this call hold neither "k_ensemble" nor
// "k_interval": the resource tests of those kernels count theirs by substring.)  A block takes one unit u = u0 +
// blockIdx.x of the call's chunk -- table t = u / nqb, spectrum block u % nqb -- and the data sets of its p-slice
// (blockIdx.z, ens_share).  Before the loop: the front half, the templates, the background and S1 = tree(X), none of
// which reads the data.  Per data set: k_interval's best fit and search, the same text by #include (as in the
// ensemble kernels), so the record of (p, t, q) has nusi_plan_response_limit's bits; every per-toy value is set
// anew at the top of the loop.  No LDS: the best fit's statistic is not formed.
// A side's limit goes to row[P] + p, row = the spectrum's place in the chunk's scratch ((u - u0) QB + grp; compact) or
// t Q + q in the caller's [ntab][Q][P]; its word to words[t][q][p][side]; a flag among NUSI_LIMIT_AT_ZERO .. _NOT_CONVERGED
// adds one to tally[t][q][side][flag] (integer atomics: the order is free; the caller zeroes the tally).
// ---------------------------------------------------------------------------
struct ToysOut {
    double *lo, *hi;   // a side's values, or nullptr
    int lo_compact, hi_compact;
    int* words;        // [ntab][Q][P][2] or nullptr
    int* tally;        // [ntab][Q][2][4] or nullptr
};

template <int NC>
__global__ __launch_bounds__(kEvThreads) void k_toys_limit(const double* __restrict__ R, const double* __restrict__ S,
                                                           const double* __restrict__ data, const double* __restrict__ bg,
                                                           const double* __restrict__ T, const FitPrior pr, const double ku,
                                                           const double klu, const double delta, const int which,
                                                           const ToysOut o, int u0, int nqb, int M, int C, int lgC, int Q, int P)
{
#pragma clang fp contract(off)
    constexpr int KT = NC - 1, KA = KT > 0 ? KT : 1;
    const int tid = (int)threadIdx.x, u = u0 + (int)blockIdx.x, t = u / nqb;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, qb0 = (u - t * nqb) * QB, q = qb0 + grp;
    const int cc = c < C ? c : C - 1;
    const double* __restrict__ Rt = R + (size_t)t * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)(q < Q ? q : Q - 1) * M;
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
    const size_t rq = (size_t)t * Q + q;                      // the spectrum's row of the call's arrays
    const size_t rc = (size_t)(u - u0) * QB + grp;            // ... and of the chunk's scratch
    const size_t rlo = (o.lo_compact ? rc : rq) * P, rhi = (o.hi_compact ? rc : rq) * P;

#pragma unroll 1
    for (int p = p0; p < p1; ++p) {
        const double d = in ? data[(size_t)p * C + cc] : 0.0;

        // ---- the best fit --------------------------------------------------------------------------------------------
        double thh[NC], muh;
        int sth;
        if constexpr (NC == 1) {
            double S1[1] = {S1h[0]};
#include "nusi_profile_chain1.inc"
            thh[0] = a[0];
            muh = m;
            sth = st;
        } else {
            constexpr int NS = NC + NC * (NC + 1) / 2;   // a round's sums: S2_j, then H_jk (j <= k, row-major)
            double S1[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) S1[j] = S1h[j];
#define FN_NSIG 1
#include "nusi_fit_newton.inc"
#undef FN_NSIG
#pragma unroll
            for (int j = 0; j < NC; ++j) thh[j] = th[j];
            muh = m;
            sth = st;
        }

        // ---- the search ----------------------------------------------------------------------------------------------
#include "nusi_search_setup.inc"
#pragma unroll 1
        for (int side = 1; side >= 0; --side) {   // 1: the upper side, 0: the lower
#include "nusi_search_side.inc"
            if (c == 0 && q < Q) {
                double* out = upper ? o.hi : o.lo;
                if (out) out[(upper ? rhi : rlo) + p] = res;
                if (o.words) o.words[(rq * P + p) * 2 + side] = word;
                if (o.tally) {
                    int* ty = o.tally + (rq * 2 + side) * 4;
                    if (word & NUSI_LIMIT_AT_ZERO) atomicAdd(ty + 0, 1);
                    if (word & NUSI_LIMIT_UNBOUNDED) atomicAdd(ty + 1, 1);
                    if (word & NUSI_LIMIT_NO_FIT) atomicAdd(ty + 2, 1);
                    if (word & NUSI_LIMIT_NOT_CONVERGED) atomicAdd(ty + 3, 1);
                }
            }
        }
    }
}

int toys_limit_block(int C) { return kEvThreads >> ceil_log2(C); }

hipError_t launch_toys_limit(const GridDev& g, const double* R, const double* S, int Q, const double* data, int P,
                             const double* bg, int C, int K, const double* T, const double* pm, const double* pw,
                             double delta, int which, int u0, int nu, int pslices, double* lo, bool lo_compact, double* hi,
                             bool hi_compact, int* words, int* tally, hipStream_t s)
{
    if (nu <= 0 || Q <= 0 || P <= 0) return hipSuccess;
    const int lg = ceil_log2(C), QB = kEvThreads >> lg, nqb = (Q + QB - 1) / QB;
    const FitPrior pr = fit_prior(K, pm, pw);
    const double ku = fit_ku(lg, K);
    const double klu = fit_klu(lg, K);
    const ToysOut o{lo, hi, lo_compact ? 1 : 0, hi_compact ? 1 : 0, words, tally};
    const dim3 grid((unsigned)nu, 1, (unsigned)pslices), block(kEvThreads);
    const int M = g.T + 1;
    switch (K) {
    case 0: hipLaunchKernelGGL((k_toys_limit<1>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, o, u0, nqb, M, C, lg, Q, P); break;
    case 1: hipLaunchKernelGGL((k_toys_limit<2>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, o, u0, nqb, M, C, lg, Q, P); break;
    case 2: hipLaunchKernelGGL((k_toys_limit<3>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, o, u0, nqb, M, C, lg, Q, P); break;
    case 3: hipLaunchKernelGGL((k_toys_limit<4>), grid, block, 0, s, R, S, data, bg, T, pr, ku, klu, delta, which, o, u0, nqb, M, C, lg, Q, P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_toys_band: the order statistics of a spectrum's P limits (the band of nusi_plan_response_ensemble_limit).  A block
// takes one spectrum of the chunk (blockIdx.x: unit u0 + x / QBe, the unit's spectrum x % QBe, QBe = min(QB, Q) -- a
// call of fewer spectra than a block launches no blocks for the rest; past Q: nothing) and one side (blockIdx.y).  A limit is a non-negative double, +inf or NaN, never -0.0, so its bit pattern with NaN mapped to
// all ones is a monotone 64-bit key under (isnan(x), x): the keys are sorted in LDS by a bitonic network over
// npad = 2^ceil(log2 P) slots (the padding: all ones, behind every rank < P) and band[t][q][k] is the key at rank[k],
// all ones read back as NaN; rank [NR] is device memory.  Equal keys are equal bits, so the result does not depend on
// the network.
// A side with src == nullptr (not asked for) writes NaN.
// ---------------------------------------------------------------------------
constexpr int kBandThreads = 256;

__global__ __launch_bounds__(kBandThreads) void k_toys_band(const double* __restrict__ lo, int lo_compact,
                                                            const double* __restrict__ hi, int hi_compact,
                                                            double* __restrict__ band_lo, double* __restrict__ band_hi,
                                                            const int* __restrict__ rank, int NR, int u0, int nqb, int QB,
                                                            int QBe, int Q, int P, int npad)
{
    extern __shared__ unsigned long long skey[];   // [npad]
    const int tid = (int)threadIdx.x, nth = (int)blockDim.x;
    const int x = (int)blockIdx.x, du = x / QBe, g = x - du * QBe, u = u0 + du, t = u / nqb, q = (u - t * nqb) * QB + g;
    const bool upper = blockIdx.y == 1;
    double* __restrict__ band = upper ? band_hi : band_lo;
    if (q >= Q || !band) return;   // (uniform over the block)
    const double* __restrict__ src = upper ? hi : lo;
    const size_t rq = (size_t)t * Q + q;
    if (!src) {
        for (int k = tid; k < NR; k += nth) band[rq * NR + k] = __builtin_nan("");
        return;
    }
    src += ((upper ? hi_compact : lo_compact) ? (size_t)du * QB + g : rq) * P;
    for (int i = tid; i < npad; i += nth) {
        unsigned long long key = ~0ull;
        if (i < P) {
            const double v = src[i];
            key = v != v ? ~0ull : (unsigned long long)__double_as_longlong(v);
        }
        skey[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (npad >> 1); i += nth) {
                const int a = ((i & ~(j - 1)) << 1) | (i & (j - 1)), bb = a | j;   // the pair (a, a + j) of this stage
                const unsigned long long ka = skey[a], kb = skey[bb];
                const bool up = (a & k) == 0;
                if ((ka > kb) == up) {
                    skey[a] = kb;
                    skey[bb] = ka;
                }
            }
            __syncthreads();
        }
    for (int k = tid; k < NR; k += nth) {
        const unsigned long long key = skey[rank[k]];
        band[rq * NR + k] = key == ~0ull ? __builtin_nan("") : __longlong_as_double((long long)key);
    }
}

hipError_t launch_toys_band(int C, int Q, int P, int u0, int nu, const double* lo, bool lo_compact, const double* hi,
                            bool hi_compact, double* band_lo, double* band_hi, const int* rank, int NR, hipStream_t s)
{
    if (nu <= 0 || NR <= 0 || NR > NUSI_BAND_RANKS_MAX || (!band_lo && !band_hi)) return hipSuccess;
    const int lg = ceil_log2(C), QB = kEvThreads >> lg, nqb = (Q + QB - 1) / QB;
    int npad = 1;
    while (npad < P) npad <<= 1;
    int nth = npad >> 1;
    nth = nth < 64 ? 64 : (nth > kBandThreads ? kBandThreads : nth);
    const int QBe = QB < Q ? QB : Q;
    const dim3 grid((unsigned)((long long)nu * QBe), 2), block((unsigned)nth);
    hipLaunchKernelGGL(k_toys_band, grid, block, sizeof(unsigned long long) * (size_t)npad, s, lo, lo_compact ? 1 : 0, hi,
                       hi_compact ? 1 : 0, band_lo, band_hi, rank, NR, u0, nqb, QB, QBe, Q, P, npad);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_poisson_draw: out[row][p][c] = draw::poisson(mu[row][c]) under the identity (seed, stream, row, p, c)
// (nusi_plan_draw_counts): one lane per count, no lane reads another's.  n = rows P C <= NUSI_DRAW_COUNTS_MAX =
// (2^31 - 1) 256: the grid of one launch.
// ---------------------------------------------------------------------------
constexpr int kDrawThreads = 256;

__global__ __launch_bounds__(kDrawThreads) void k_poisson_draw(const double* __restrict__ mu, double* __restrict__ out, int C,
                                                               int P, unsigned long long n, unsigned long long seed,
                                                               unsigned stream)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kDrawThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long rp = i / (unsigned)C;
    const unsigned c = (unsigned)(i - rp * (unsigned)C), row = (unsigned)(rp / (unsigned)P), p = (unsigned)(rp - (unsigned long long)row * (unsigned)P);
    out[i] = draw::poisson(mu[(size_t)row * C + c], draw::ident(seed, stream, row, p, c));
}

hipError_t launch_poisson_draw(const double* mu, int rows, int C, int P, unsigned long long seed, unsigned stream, double* out,
                               hipStream_t s)
{
    if (rows <= 0 || C <= 0 || P <= 0) return hipSuccess;
    const unsigned long long n = (unsigned long long)rows * P * C, nb = (n + kDrawThreads - 1) / kDrawThreads;
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_poisson_draw, dim3((unsigned)nb), dim3(kDrawThreads), 0, s, mu, out, C, P, n, seed, stream);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_normal_draw: out[row][p][j] = draw::normal0(center[row][j], sigma[j]) under the identity (seed, stream, row, p, j)
// (nusi_plan_draw_normals): k_poisson_draw's shape, one lane per variate.  cs = center [rows][J], then sigma [J].
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kDrawThreads) void k_normal_draw(const double* __restrict__ cs, double* __restrict__ out, int rows,
                                                              int J, int P, unsigned long long n, unsigned long long seed,
                                                              unsigned stream)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kDrawThreads + threadIdx.x;
    if (i >= n) return;
    const unsigned long long rp = i / (unsigned)J;
    const unsigned j = (unsigned)(i - rp * (unsigned)J), row = (unsigned)(rp / (unsigned)P), p = (unsigned)(rp - (unsigned long long)row * (unsigned)P);
    out[i] = draw::normal0(cs[(size_t)row * J + j], cs[(size_t)rows * J + j], draw::ident(seed, stream, row, p, j));
}

hipError_t launch_normal_draw(const double* cs, int rows, int J, int P, unsigned long long seed, unsigned stream, double* out,
                              hipStream_t s)
{
    if (rows <= 0 || J <= 0 || P <= 0) return hipSuccess;
    const unsigned long long n = (unsigned long long)rows * P * J, nb = (n + kDrawThreads - 1) / kDrawThreads;
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_normal_draw, dim3((unsigned)nb), dim3(kDrawThreads), 0, s, cs, out, rows, J, P, n, seed, stream);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_inject<NC>: the calibration call (nusi_plan_response_inject), NC = 1 + K = 1 .. 4, on k_toys_limit<NC>'s block
// shape, units and p-slices.  Per (t, q) and toy p the datum of lane c is DRAWN where it is fitted: draw::poisson of
// mu_inj[c] = a_inj[q] s_c + sum_j theta_inj[j] T_jc + B_c (the conditional fit's order for mu) under the identity
// (seed, stream = t, row = q, p, c), which is global -- no chunk, slice or launch shape enters.  Then, against that
// datum: the best fit (k_detector_profile's / k_detector_fit's iteration, the same text by #include as in
// k_toys_limit), ONE conditional fit at a_test[q] from the header's cold start (k_conditional_fit's rounds,
// nusi_conditional_newton.inc, and its word; K = 0: a single evaluation, word 0), lambda as k_interval forms it, and the statistic under `mode`.  No LDS.
// theta_hat_0 goes to row[P] + p of o.theta and the statistic to o.stat (row: the spectrum's place in the chunk's
// scratch, compact, or t Q + q in the caller's [ntab][Q][P]) -- k_toys_band then selects from them, theta_hat_0 on its
// lo side and the statistic on hi --, the two words to words[t][q][p][2], the counts to tally[t][q][4] and exceed[t][q]
// (integer atomics; the caller zeroes both), the drawn counts to data[t][q][p][C].
// ---------------------------------------------------------------------------
struct InjectOut {
    double *theta, *stat;   // theta_hat_0 and the statistic per toy, or nullptr
    int theta_compact, stat_compact;
    int* words;             // [ntab][Q][P][2] or nullptr
    int* tally;             // [ntab][Q][4] or nullptr
    int* exceed;            // [ntab][Q] or nullptr (with qobs)
    double* data;           // [ntab][Q][P][C] or nullptr
};
struct InjectIn {
    const double *a_inj, *a_test, *qobs;   // [Q], [Q], [ntab][Q] (qobs: nullptr without exceed)
    double th_inj[NUSI_FIT_TEMPLATES_MAX + 1];   // [0] unused
    unsigned long long seed;
    int mode;
};

template <int NC>
__global__ __launch_bounds__(kEvThreads) void k_inject(const double* __restrict__ R, const double* __restrict__ S,
                                                       const double* __restrict__ bg, const double* __restrict__ T,
                                                       const FitPrior pr, const double ku, const InjectIn ii, const InjectOut o,
                                                       int u0, int nqb, int M, int C, int lgC, int Q, int P)
{
#pragma clang fp contract(off)
#include "nusi_inject_setup.inc"
#pragma unroll 1
    for (int p = p0; p < p1; ++p) {
        // (the expectation through an opaque copy: the sampler's set-up is formed per toy and not held across the fits)
        double mup = mu_inj;
        asm volatile("" : "+v"(mup));
        const double d = in ? draw::poisson(mup, draw::ident(ii.seed, (unsigned)t, (unsigned)qc, (unsigned)p, (unsigned)c)) : 0.0;
        if (o.data && in && q < Q) o.data[(rq * P + p) * C + c] = d;

#include "nusi_toy_body.inc"
#include "nusi_inject_store.inc"
    }
}

// k_nuis_inject<NC, MODE>: k_inject<NC> under NUSI_OPT_TOY_NUISANCE = MODE, NUSI_TOYS_GLOBAL or NUSI_TOYS_PRIOR, NC = 2 .. 4,
// launched only where a template is constrained (a w_j > 0): the same set-up, toy body and stores by #include, with the
// toy's draws in front.  The toy's prior means (GLOBAL: m*_j) or its nuisances (PRIOR: theta*_j) are draw::normal0 of
// the identity (seed, stream = t, row = q, p, j), j = 0 .. K - 1 the template, formed by every lane of the group --
// uniform over it by construction, like theta.  `pr`, which the included texts read, is the toy's own copy of the plan's
// priors prp: its means are vector values where a draw replaced them.  sg: the widths sigma_j (+inf: no prior).
struct ToySigma {
    double s[NUSI_FIT_TEMPLATES_MAX + 1];   // [0] unused
};

template <int NC, int MODE>
__global__ __launch_bounds__(kEvThreads) void k_nuis_inject(const double* __restrict__ R, const double* __restrict__ S,
                                                            const double* __restrict__ bg, const double* __restrict__ T,
                                                            const FitPrior prp, const ToySigma sg, const double ku,
                                                            const InjectIn ii, const InjectOut o, int u0, int nqb, int M, int C,
                                                            int lgC, int Q, int P)
{
#pragma clang fp contract(off)
    static_assert(NC > 1 && (MODE == NUSI_TOYS_GLOBAL || MODE == NUSI_TOYS_PRIOR), "k_nuis_inject: templates and a randomised ensemble");
#include "nusi_inject_setup.inc"
#pragma unroll 1
    for (int p = p0; p < p1; ++p) {
        FitPrior pr = prp;
        // (the expectation through an opaque copy, as in k_inject)
        double mup = mu_inj;
        if constexpr (MODE == NUSI_TOYS_GLOBAL) {
#pragma unroll
            for (int j = 1; j < NC; ++j)
                if (prp.w[j] > 0.0)
                    pr.m[j] = draw::normal0(ii.th_inj[j], sg.s[j], draw::ident(ii.seed, (unsigned)t, (unsigned)qc, (unsigned)p, (unsigned)(j - 1)));
        } else {
            mup = ii.a_inj[qc] * X[0];
#pragma unroll
            for (int j = 1; j < NC; ++j) {
                double thj = ii.th_inj[j];
                if (prp.w[j] > 0.0)
                    thj = draw::normal0(prp.m[j], sg.s[j], draw::ident(ii.seed, (unsigned)t, (unsigned)qc, (unsigned)p, (unsigned)(j - 1)));
                mup = mup + thj * X[j];
            }
            mup = mup + b;
        }
        asm volatile("" : "+v"(mup));
        const double d = in ? draw::poisson(mup, draw::ident(ii.seed, (unsigned)t, (unsigned)qc, (unsigned)p, (unsigned)c)) : 0.0;
        if (o.data && in && q < Q) o.data[(rq * P + p) * C + c] = d;

#include "nusi_toy_body.inc"
#include "nusi_inject_store.inc"
    }
}

// a call's widths as the kernels take them (fit_prior's slots)
static ToySigma toy_sigma(int K, const double* ps)
{
    ToySigma sg;
    for (int j = 0; j <= NUSI_FIT_TEMPLATES_MAX; ++j) sg.s[j] = (j >= 1 && j <= K) ? ps[j - 1] : __builtin_inf();
    return sg;
}
// does the ensemble `toys` differ from NUSI_TOYS_FIXED on these priors?  (K = 0, or no constrained template: no)
static bool toy_randomised(int toys, int K, const double* pw)
{
    bool any = false;
    for (int j = 0; j < K; ++j) any = any || pw[j] > 0.0;
    return toys != NUSI_TOYS_FIXED && any;
}

hipError_t launch_inject(const GridDev& g, const double* R, const double* S, int Q, const double* a_inj, const double* a_test,
                         const double* th_inj, const double* qobs, int P, unsigned long long seed, int mode, const double* bg,
                         int C, int K, const double* T, const double* pm, const double* pw, const double* ps, int toys, int u0,
                         int nu, int pslices, double* theta, bool theta_compact, double* stat, bool stat_compact, int* words,
                         int* tally, int* exceed, double* data, hipStream_t s)
{
    if (nu <= 0 || Q <= 0 || P <= 0) return hipSuccess;
    const int lg = ceil_log2(C), QB = kEvThreads >> lg, nqb = (Q + QB - 1) / QB;
    const FitPrior pr = fit_prior(K, pm, pw);
    InjectIn ii{a_inj, a_test, qobs, {}, seed, mode};
    for (int j = 0; j <= NUSI_FIT_TEMPLATES_MAX; ++j) ii.th_inj[j] = (j >= 1 && j <= K) ? th_inj[j - 1] : 0.0;
    const double ku = fit_ku(lg, K);
    const InjectOut o{theta, stat, theta_compact ? 1 : 0, stat_compact ? 1 : 0, words, tally, exceed, data};
    const dim3 grid((unsigned)nu, 1, (unsigned)pslices), block(kEvThreads);
    const int M = g.T + 1;
    if (toy_randomised(toys, K, pw)) {
        const ToySigma sg = toy_sigma(K, ps);
#define NUSI_NUIS_INJECT(NC, MODE) \
    hipLaunchKernelGGL((k_nuis_inject<NC, MODE>), grid, block, 0, s, R, S, bg, T, pr, sg, ku, ii, o, u0, nqb, M, C, lg, Q, P)
        switch (K * 4 + toys) {
        case 1 * 4 + NUSI_TOYS_GLOBAL: NUSI_NUIS_INJECT(2, NUSI_TOYS_GLOBAL); break;
        case 2 * 4 + NUSI_TOYS_GLOBAL: NUSI_NUIS_INJECT(3, NUSI_TOYS_GLOBAL); break;
        case 3 * 4 + NUSI_TOYS_GLOBAL: NUSI_NUIS_INJECT(4, NUSI_TOYS_GLOBAL); break;
        case 1 * 4 + NUSI_TOYS_PRIOR: NUSI_NUIS_INJECT(2, NUSI_TOYS_PRIOR); break;
        case 2 * 4 + NUSI_TOYS_PRIOR: NUSI_NUIS_INJECT(3, NUSI_TOYS_PRIOR); break;
        case 3 * 4 + NUSI_TOYS_PRIOR: NUSI_NUIS_INJECT(4, NUSI_TOYS_PRIOR); break;
        default: return hipErrorInvalidValue;
        }
#undef NUSI_NUIS_INJECT
        return hipGetLastError();
    }
    switch (K) {
    case 0: hipLaunchKernelGGL((k_inject<1>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nqb, M, C, lg, Q, P); break;
    case 1: hipLaunchKernelGGL((k_inject<2>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nqb, M, C, lg, Q, P); break;
    case 2: hipLaunchKernelGGL((k_inject<3>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nqb, M, C, lg, Q, P); break;
    case 3: hipLaunchKernelGGL((k_inject<4>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nqb, M, C, lg, Q, P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_belt<NC>: the toy-calibrated interval's records (nusi_plan_response_belt), NC = 1 + K = 1 .. 4, on k_inject<NC>'s
// block shape.  A record is (t, q, g) with row r = q G + g of the table's Q G rows; unit u is table u / nrb and row block
// u % nrb, nrb = ceil(Q G / QB); a group of the block takes one row.  The test scale is a = frac[g] ref[t][q], agood =
// ref >= 0 && a < inf, at = agood ? a : 0.  The loop over the toys has one pass in front, against the staged data d[c]
// (nusi_toy_body.inc, the text of the toys' own pass): it gives the record's observed side, q_obs, and mu_inj, the
// conditional fit's own mu -- then toy p of lane c is draw::poisson(mu_inj[c]; seed, stream = t, row = r, p, c).  Every
// p-slice runs the observed pass and slice 0 stores it.  A record that is invalid (!agood, or NOT_CONVERGED | SINGULAR
// in either observed word) stays in the loop with mu_inj = 0, which draws nothing: it adds to no count, and what it
// stores to the raw arrays is their NaN / 0.  A row outside the table (r >= Q G) or outside the launch's pairs
// pr0 <= t Q + q < pr1 stores nothing; every load index is clamped (cc, rc and with it q and g).
// exceed [.][G], tally [.][G][4] and words_obs [.][1 + G] are indexed by the pair t Q + q, or by t Q + q - pr0 where the
// array is the chunk's scratch (compact); the caller zeroes exceed and tally.
// ---------------------------------------------------------------------------
struct BeltOut {
    int *exceed, *tally, *wobs;            // or nullptr
    int exceed_compact, tally_compact, wobs_compact;
    double *qobs, *thobs;                  // [ntab][Q][G], [ntab][Q][1 + G][NC] or nullptr
    double *theta, *stat;                  // [ntab][Q][G][P] or nullptr
    int* words;                            // [ntab][Q][G][P][2] or nullptr
    double* data;                          // [ntab][Q][G][P][C] or nullptr
};
struct BeltIn {
    const double *data, *frac, *ref;       // [C], [G], [ntab][Q] (ref: nullptr = 1)
    unsigned long long seed;
    int mode, G, pr0, pr1;
};

template <int NC>
__global__ __launch_bounds__(kEvThreads) __attribute__((amdgpu_waves_per_eu(NC == 1 ? 4 : NC == 4 ? 2 : 3)))
void k_belt(const double* __restrict__ R, const double* __restrict__ S, const double* __restrict__ bg,
            const double* __restrict__ T, const FitPrior pr, const double ku, const BeltIn ii, const BeltOut o, int u0, int nrb,
            int M, int C, int lgC, int Q, int P)
{
#pragma clang fp contract(off)
#include "nusi_belt_setup.inc"
#pragma unroll 1
    for (int p = p0 - 1; p < p1; ++p) {
        const bool obs = p < p0;   // (uniform over the block: the pass against the data)
        double d;
        if (obs) {
            d = in ? ii.data[cc] : 0.0;
        } else {
            // (the expectation through an opaque copy, as in k_inject)
            double mup = mu_inj;
            asm volatile("" : "+v"(mup));
            d = in ? draw::poisson(mup, draw::ident(ii.seed, (unsigned)t, (unsigned)rc, (unsigned)p, (unsigned)c)) : 0.0;
            if (o.data && in && mine) o.data[(rg * P + p) * C + c] = valid ? d : 0.0;
        }

#include "nusi_toy_body.inc"
#include "nusi_belt_store.inc"
    }
}

// k_nuis_belt<NC>: k_belt<NC> under NUSI_TOYS_GLOBAL, NC = 2 .. 4, as k_nuis_inject<NC, NUSI_TOYS_GLOBAL> is k_inject<NC>'s.
// The centre of a toy's m*_j is the observed conditional fit's theta_j(a) of the record, kept from the observed pass,
// which itself reads the plan's means; the identity is (seed, stream = t, row = q G + g, p, j).
template <int NC>
__global__ __launch_bounds__(kEvThreads) __attribute__((amdgpu_waves_per_eu(NC == 4 ? 2 : 3)))
void k_nuis_belt(const double* __restrict__ R, const double* __restrict__ S, const double* __restrict__ bg,
                 const double* __restrict__ T, const FitPrior prp, const ToySigma sg, const double ku, const BeltIn ii,
                 const BeltOut o, int u0, int nrb, int M, int C, int lgC, int Q, int P)
{
#pragma clang fp contract(off)
    static_assert(NC > 1, "k_nuis_belt: templates");
#include "nusi_belt_setup.inc"
    double cen[KT];   // the centres: set by the observed pass (an invalid record has no toys to store: 0)
#pragma unroll
    for (int j = 0; j < KT; ++j) cen[j] = 0.0;

#pragma unroll 1
    for (int p = p0 - 1; p < p1; ++p) {
        const bool obs = p < p0;   // (uniform over the block: the pass against the data)
        FitPrior pr = prp;
        double d;
        if (obs) {
            d = in ? ii.data[cc] : 0.0;
        } else {
#pragma unroll
            for (int j = 1; j < NC; ++j)
                if (prp.w[j] > 0.0)
                    pr.m[j] = draw::normal0(cen[j - 1], sg.s[j], draw::ident(ii.seed, (unsigned)t, (unsigned)rc, (unsigned)p, (unsigned)(j - 1)));
            // (the expectation through an opaque copy, as in k_inject)
            double mup = mu_inj;
            asm volatile("" : "+v"(mup));
            d = in ? draw::poisson(mup, draw::ident(ii.seed, (unsigned)t, (unsigned)rc, (unsigned)p, (unsigned)c)) : 0.0;
            if (o.data && in && mine) o.data[(rg * P + p) * C + c] = valid ? d : 0.0;
        }

#include "nusi_toy_body.inc"
#include "nusi_belt_store.inc"
        if (obs)
#pragma unroll
            for (int j = 0; j < KT; ++j) cen[j] = valid ? th[j] : 0.0;
    }
}

// k_belt_accept: per pair (t, q) of pr0 .. pr1 - 1 the acceptance rule over the G points, g ascending, from the counts and
// the observed words (detector.belt_accept with belt_host's valid and flags): a = frac[g] ref[t][q]; valid = agood and
// neither word[0] nor word[1 + g] flagged; nv = P - tally[0] - tally[1]; accepted iff valid, nv > 0 and (double)exceed >
// alpha (double)nv.  lo, hi [ntab][Q], idx [ntab][Q][2], status [ntab][Q]; any may be nullptr.
constexpr int kBeltAcceptThreads = 256;

__global__ __launch_bounds__(kBeltAcceptThreads) void k_belt_accept(const BeltIn ii, const int* __restrict__ exceed,
                                                                    int exceed_compact, const int* __restrict__ tally,
                                                                    int tally_compact, const int* __restrict__ wobs,
                                                                    int wobs_compact, int P, double alpha,
                                                                    double* __restrict__ lo, double* __restrict__ hi,
                                                                    int* __restrict__ idx, int* __restrict__ status)
{
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kBeltAcceptThreads + threadIdx.x + ii.pr0;
    if (i >= ii.pr1) return;
    const int pair = (int)i, G = ii.G, fail = NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR;
    const int* ex = exceed + (size_t)(pair - (exceed_compact ? ii.pr0 : 0)) * G;
    const int* ty = tally + (size_t)(pair - (tally_compact ? ii.pr0 : 0)) * G * 4;
    const int* wo = wobs + (size_t)(pair - (wobs_compact ? ii.pr0 : 0)) * (1 + G);
    const double rf = ii.ref ? ii.ref[pair] : 1.0;
    const bool nofit = (wo[0] & fail) != 0;
    int st = nofit ? NUSI_BELT_NO_FIT : 0, first = -1, last = -1, nacc = 0;
    for (int g = 0; g < G; ++g) {
        const double a = ii.frac[g] * rf;
        const bool agood = rf >= 0.0 && a < __builtin_inf();
        const bool nocond = (wo[1 + g] & fail) != 0;
        if (!agood) st |= NUSI_BELT_NO_GRID;
        if (agood && !nofit && nocond) st |= NUSI_BELT_BAD_POINT;
        const int nv = P - ty[g * 4] - ty[g * 4 + 1];
        if (nv <= 0) st |= NUSI_BELT_BAD_POINT;
        const double lim = alpha * (double)nv;
        if (agood && !nofit && !nocond && nv > 0 && (double)ex[g] > lim) {
            if (first < 0) first = g;
            last = g;
            ++nacc;
        }
    }
    if (nacc == 0) st |= NUSI_BELT_EMPTY;
    if (first == 0) st |= NUSI_BELT_LO_EDGE;
    if (last == G - 1) st |= NUSI_BELT_HI_EDGE;
    if (nacc > 0 && nacc != last - first + 1) st |= NUSI_BELT_GAPS;
    if (lo) lo[pair] = nacc > 0 ? ii.frac[first] * rf : __builtin_nan("");
    if (hi) hi[pair] = nacc > 0 ? ii.frac[last] * rf : __builtin_nan("");
    if (idx) {
        idx[(size_t)pair * 2] = first;
        idx[(size_t)pair * 2 + 1] = last;
    }
    if (status) status[pair] = st;
}

int belt_block(int C) { return kEvThreads >> ceil_log2(C); }

hipError_t launch_belt(const GridDev& g, const double* R, const double* S, int Q, const double* data, const double* frac,
                       int G, const double* ref, int P, unsigned long long seed, int mode, const double* bg, int C, int K,
                       const double* T, const double* pm, const double* pw, const double* ps, int toys, int pr0, int pr1,
                       int pslices, int* exceed, bool exceed_compact, int* tally, bool tally_compact, int* wobs,
                       bool wobs_compact, double* qobs, double* thobs, double* theta, double* stat, int* words, double* data_all,
                       hipStream_t s)
{
    if (pr1 <= pr0 || Q <= 0 || G <= 0 || P <= 0) return hipSuccess;
    const int lg = ceil_log2(C), QB = kEvThreads >> lg, nrb = (int)(((long long)Q * G + QB - 1) / QB);
    // the units that hold the rows of the pairs pr0 .. pr1 - 1 (a unit at the chunk's edge may hold other pairs' rows too)
    const int t0 = pr0 / Q, q0 = pr0 - t0 * Q, t1 = (pr1 - 1) / Q, q1 = (pr1 - 1) - t1 * Q;
    const long long ua = (long long)t0 * nrb + ((long long)q0 * G) / QB, ub = (long long)t1 * nrb + ((long long)q1 * G + G - 1) / QB;
    if (ub - ua + 1 > 0x7fffffffll) return hipErrorInvalidValue;
    const FitPrior pr = fit_prior(K, pm, pw);
    const BeltIn ii{data, frac, ref, seed, mode, G, pr0, pr1};
    const BeltOut o{exceed, tally, wobs, exceed_compact ? 1 : 0, tally_compact ? 1 : 0, wobs_compact ? 1 : 0,
                    qobs, thobs, theta, stat, words, data_all};
    const double ku = fit_ku(lg, K);
    const dim3 grid((unsigned)(ub - ua + 1), 1, (unsigned)pslices), block(kEvThreads);
    const int M = g.T + 1, u0 = (int)ua;
    if (toy_randomised(toys, K, pw)) {
        if (toys != NUSI_TOYS_GLOBAL) return hipErrorInvalidValue;
        const ToySigma sg = toy_sigma(K, ps);
        switch (K) {
        case 1: hipLaunchKernelGGL((k_nuis_belt<2>), grid, block, 0, s, R, S, bg, T, pr, sg, ku, ii, o, u0, nrb, M, C, lg, Q, P); break;
        case 2: hipLaunchKernelGGL((k_nuis_belt<3>), grid, block, 0, s, R, S, bg, T, pr, sg, ku, ii, o, u0, nrb, M, C, lg, Q, P); break;
        case 3: hipLaunchKernelGGL((k_nuis_belt<4>), grid, block, 0, s, R, S, bg, T, pr, sg, ku, ii, o, u0, nrb, M, C, lg, Q, P); break;
        default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (K) {
    case 0: hipLaunchKernelGGL((k_belt<1>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nrb, M, C, lg, Q, P); break;
    case 1: hipLaunchKernelGGL((k_belt<2>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nrb, M, C, lg, Q, P); break;
    case 2: hipLaunchKernelGGL((k_belt<3>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nrb, M, C, lg, Q, P); break;
    case 3: hipLaunchKernelGGL((k_belt<4>), grid, block, 0, s, R, S, bg, T, pr, ku, ii, o, u0, nrb, M, C, lg, Q, P); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_belt_accept(const double* frac, int G, const double* ref, int P, double alpha, int pr0, int pr1,
                              const int* exceed, bool exceed_compact, const int* tally, bool tally_compact, const int* wobs,
                              bool wobs_compact, double* lo, double* hi, int* idx, int* status, hipStream_t s)
{
    if (pr1 <= pr0) return hipSuccess;
    const BeltIn ii{nullptr, frac, ref, 0ull, 0, G, pr0, pr1};
    const unsigned nb = (unsigned)(((long long)(pr1 - pr0) + kBeltAcceptThreads - 1) / kBeltAcceptThreads);
    hipLaunchKernelGGL(k_belt_accept, dim3(nb), dim3(kBeltAcceptThreads), 0, s, ii, exceed, exceed_compact ? 1 : 0, tally,
                       tally_compact ? 1 : 0, wobs, wobs_compact ? 1 : 0, P, alpha, lo, hi, idx, status);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_composition_belt<NCF>: the toy-calibrated region of the flavour composition (nusi_plan_response_composition_belt),
// NCF = 3 + K = 3 .. 6, on k_belt's block shape: a record is (t, q, g) with row r = q G + g of the table's Q G rows, unit
// u is table u / nrb and row block u % nrb, a group of the block takes one row, p-slices on the grid's z.  g is a point
// phi[g] (or phi[t][g]) of the composition grid.  The front half runs once per row with FOUR accumulators, each in
// events' order: the three components s_j of k_components_fit<3, .> and the held signal s_phi, the composed row
// r = (phi_0 R3[t][0][n][c] + phi_1 R3[t][1][n][c]) + phi_2 R3[t][2][n][c] in k_response_compose's expression -- what
// nusi_plan_response_fit / _profile accumulate on the composed matrix, to the bit.  Then one pass against the staged data
// and one per toy, each nusi_composition_body.inc: the free fit, the held fit, lambda.  The observed pass gives the
// record's observed side, q_obs and mu_inj, the held fit's own mu; toy p of lane c is draw::poisson(mu_inj[c]; seed,
// stream = t, row = r, p, c).  Every p-slice runs the observed pass and slice 0 stores it.  An invalid record
// (NOT_CONVERGED | SINGULAR in either observed word) stays in the loop with mu_inj = 0, which draws nothing: it adds to
// no count and stores the raw arrays' NaN / 0.  A row outside the table (r >= Q G) stores nothing; every load index is
// clamped (cc, rc and with it q and g).  No LDS.
// Both fits' registers are live across the toy loop with XF, S1F, s_phi, mu_inj and q_obs: the instances ask for as few
// waves per SIMD as that takes (comp_belt_waves; DESIGN.md sec. 4, "The composition region").
// ---------------------------------------------------------------------------
struct CompBeltOut {
    int *exceed, *tally, *wobs;            // [ntab][Q][G], [ntab][Q][G][4], [ntab][Q][1 + G] or nullptr
    double *qobs, *thobs;                  // [ntab][Q][G], [ntab][Q][1 + G][NCF] or nullptr
    double *theta, *stat;                  // [ntab][Q][G][P][NCF], [ntab][Q][G][P] or nullptr
    int* words;                            // [ntab][Q][G][P][2] or nullptr
    double* data;                          // [ntab][Q][G][P][C] or nullptr
};
struct CompBeltIn {
    const double *data, *phi;              // [C], [G][3] or [ntab][G][3]
    unsigned long long seed;
    int G, phi_tables;
};

constexpr int comp_belt_waves(int NCF) { return NCF == 3 ? 3 : NCF <= 5 ? 2 : 1; }

template <int NCF>
__global__ __launch_bounds__(kEvThreads) __attribute__((amdgpu_waves_per_eu(comp_belt_waves(NCF))))
void k_composition_belt(const double* __restrict__ R3, const double* __restrict__ S, const double* __restrict__ bg,
                        const double* __restrict__ T, const FitPrior tp, const double kuf, const double kuh,
                        const CompBeltIn ii, const CompBeltOut o, int u0, int nrb, int M, int C, int lgC, int Q, int P)
{
#pragma clang fp contract(off)
    static_assert(NCF >= 3 && NCF - 3 <= NUSI_FIT_TEMPLATES_MAX, "k_composition_belt: three signal components and NCF - 3 templates");
    constexpr int KT = NCF - 3;
    const int G = ii.G, QG = Q * G;
    const int tid = (int)threadIdx.x, u = u0 + (int)blockIdx.x, t = u / nrb;
    const int c = tid & ((1 << lgC) - 1), grp = tid >> lgC;
    const int QB = kEvThreads >> lgC, row = (u - t * nrb) * QB + grp;
    const int cc = c < C ? c : C - 1, rc = row < QG ? row : QG - 1, q = rc / G, gp = rc - q * G;   // q < Q, gp < G
    const int pair = t * Q + q;
    const double* __restrict__ Rt = R3 + (size_t)t * 3 * M * C + cc;
    const double* __restrict__ Sq = S + (size_t)q * M;
    const double* __restrict__ ph = ii.phi + ((size_t)(ii.phi_tables ? t : 0) * G + gp) * 3;
    const bool in = c < C;
    const bool mine = row < QG;   // the record is this block's to store
    int p0, p1;
    ens_share(P, (int)blockIdx.z, (int)gridDim.z, p0, p1);
    double XF[NCF], sphi;
    {
        const double f0 = ph[0], f1 = ph[1], f2 = ph[2];
        double s0[3], sp = 0.0;
#pragma unroll
        for (int j = 0; j < 3; ++j) s0[j] = 0.0;
#pragma unroll 4
        for (int n = 1; n < M; ++n) {
            const double sv = Sq[n];
            double rv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                rv[j] = Rt[((size_t)j * M + n) * C];
                s0[j] = s0[j] + rv[j] * sv;
            }
            const double r = (f0 * rv[0] + f1 * rv[1]) + f2 * rv[2];
            sp = sp + r * sv;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) XF[j] = in ? s0[j] : 0.0;
        sphi = in ? sp : 0.0;
    }
#pragma unroll
    for (int j = 3; j < NCF; ++j) XF[j] = in ? T[(size_t)(j - 3) * C + cc] : 0.0;
    struct {
        double m[NCF], w[NCF];
    } prf;   // the free fit's priors: template i's behind the signal components' zeros
#pragma unroll
    for (int j = 0; j < NCF; ++j) {
        prf.m[j] = j < 3 ? 0.0 : tp.m[j < 3 ? 0 : j - 2];
        prf.w[j] = j < 3 ? 0.0 : tp.w[j < 3 ? 0 : j - 2];
    }
    const double b = in ? bg[cc] : 0.0;
    const unsigned long long gmask = (lgC == 6 ? ~0ull : (1ull << (1 << lgC)) - 1) << ((tid & 63) & ~((1 << lgC) - 1));
    auto add = [](double x, double y) { return x + y; };
    auto min = [](double x, double y) { return y < x ? y : x; };
    auto any = [&](bool x) { return (__ballot(x) & gmask) != 0; };
    double S1F[NCF], S1p;   // tree(XF_j), tree(s_phi): the data do not enter
    {
        double sv[NCF + 1];
#pragma unroll
        for (int j = 0; j < NCF; ++j) sv[j] = XF[j];
        sv[NCF] = sphi;
        det_butterfly(sv, lgC, add);
#pragma unroll
        for (int j = 0; j < NCF; ++j) S1F[j] = sv[j];
        S1p = sv[NCF];
    }
    const size_t rg = (size_t)pair * G + gp;   // the record's row of the call's [ntab][Q][G] arrays
    double mu_inj = 0.0, qobs = __builtin_nan("");   // both set by the observed pass
    bool valid = false;

#pragma unroll 1
    for (int p = p0 - 1; p < p1; ++p) {
        const bool obs = p < p0;   // (uniform over the block: the pass against the data)
        double d;
        if (obs) {
            d = in ? ii.data[cc] : 0.0;
        } else {
            // (the expectation through an opaque copy, as in k_inject)
            double mup = mu_inj;
            asm volatile("" : "+v"(mup));
            d = in ? draw::poisson(mup, draw::ident(ii.seed, (unsigned)t, (unsigned)rc, (unsigned)p, (unsigned)c)) : 0.0;
            if (o.data && in && mine) o.data[(rg * P + p) * C + c] = valid ? d : 0.0;
        }

#include "nusi_composition_body.inc"

        if (obs) {
            valid = !nofit && !nocond;
            qobs = valid ? stat : __builtin_nan("");
            mu_inj = valid ? mu : 0.0;
            if (c == 0 && mine && blockIdx.z == 0) {
                const size_t ro = (size_t)pair * (1 + G);
                if (gp == 0) {
                    if (o.thobs) {
#pragma unroll
                        for (int j = 0; j < NCF; ++j) o.thobs[ro * NCF + j] = thh[j];
                    }
                    if (o.wobs) o.wobs[ro] = sth;
                }
                if (o.thobs) {
#pragma unroll
                    for (int j = 0; j < NCF; ++j) o.thobs[(ro + 1 + gp) * NCF + j] = j <= KT ? thc[j <= KT ? j : 0] : 0.0;
                }
                if (o.wobs) o.wobs[ro + 1 + gp] = stc;
                if (o.qobs) o.qobs[rg] = qobs;
            }
        } else if (c == 0 && mine) {
            if (o.theta) {
#pragma unroll
                for (int j = 0; j < NCF; ++j) o.theta[(rg * P + p) * NCF + j] = (valid && !nofit) ? thh[j] : __builtin_nan("");
            }
            if (o.stat) o.stat[rg * P + p] = valid ? stat : __builtin_nan("");
            if (o.words) {
                o.words[(rg * P + p) * 2] = valid ? sth : 0;
                o.words[(rg * P + p) * 2 + 1] = valid ? stc : 0;
            }
            if (o.tally && valid) {
                int* ty = o.tally + rg * 4;
                if (nofit) atomicAdd(ty + 0, 1);
                if (nocond && !nofit) atomicAdd(ty + 1, 1);
                if (sth & (NUSI_FIT_ZERO * 7 | NUSI_FIT_BOUNDARY | NUSI_FIT_FLAT)) atomicAdd(ty + 2, 1);
                if (sth & NUSI_FIT_INFINITE) atomicAdd(ty + 3, 1);
            }
            if (o.exceed && valid && stat >= qobs) atomicAdd(o.exceed + rg, 1);
        }
    }
}

// k_composition_accept: per pair (t, q) the acceptance rule over the G points, g ascending, from the counts, the observed
// words and q_obs (detector.composition_accept): valid = neither word[0] nor word[1 + g] flagged; nv = P - tally[0] -
// tally[1]; accepted iff valid, nv > 0 and (double)exceed > alpha (double)nv.  accept [ntab][Q][G], status and best
// [ntab][Q]; any may be nullptr.
__global__ __launch_bounds__(kBeltAcceptThreads) void k_composition_accept(const int* __restrict__ exceed,
                                                                           const int* __restrict__ tally,
                                                                           const int* __restrict__ wobs,
                                                                           const double* __restrict__ qobs, int G, int P,
                                                                           double alpha, int npairs, int* __restrict__ accept,
                                                                           int* __restrict__ status, int* __restrict__ best)
{
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kBeltAcceptThreads + threadIdx.x;
    if (i >= npairs) return;
    const size_t pair = (size_t)i;
    const int fail = NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR;
    const int* ex = exceed + pair * G;
    const int* ty = tally + pair * G * 4;
    const int* wo = wobs + pair * (1 + G);
    const double* qo = qobs + pair * G;
    const bool nofit = (wo[0] & fail) != 0;
    int st = nofit ? NUSI_REGION_NO_FIT : 0, nacc = 0, nvalid = 0, bg = -1;
    double bq = 0.0;
    for (int g = 0; g < G; ++g) {
        const bool nocond = (wo[1 + g] & fail) != 0, valid = !nofit && !nocond;
        if (!nofit && nocond) st |= NUSI_REGION_BAD_POINT;
        const int nv = P - ty[g * 4] - ty[g * 4 + 1];
        if (valid && nv <= 0) st |= NUSI_REGION_BAD_POINT;
        const double lim = alpha * (double)nv;
        const bool acc = valid && nv > 0 && (double)ex[g] > lim;
        if (accept) accept[pair * G + g] = acc ? 1 : 0;
        nvalid += valid ? 1 : 0;
        nacc += acc ? 1 : 0;
        if (valid && (bg < 0 || qo[g] < bq)) {
            bg = g;
            bq = qo[g];
        }
    }
    if (nacc == 0) st |= NUSI_REGION_EMPTY;
    if (nvalid > 0 && nacc == nvalid) st |= NUSI_REGION_ALL;
    if (status) status[pair] = st;
    if (best) best[pair] = bg;
}

int composition_belt_block(int C) { return kEvThreads >> ceil_log2(C); }

hipError_t launch_composition_belt(const GridDev& g, const double* R3, int ntab, const double* S, int Q, const double* data,
                                   const double* phi, bool phi_tables, int G, int P, unsigned long long seed, const double* bg,
                                   int C, int K, const double* T, const double* pm, const double* pw, int pslices,
                                   int* exceed, int* tally, int* wobs, double* qobs, double* thobs, double* theta, double* stat,
                                   int* words, double* data_all, hipStream_t s)
{
    if (ntab <= 0 || Q <= 0 || G <= 0 || P <= 0) return hipSuccess;
    const int lg = ceil_log2(C), QB = kEvThreads >> lg, nrb = (int)(((long long)Q * G + QB - 1) / QB);
    const long long units = (long long)ntab * nrb;
    if (units > 0x7fffffffll) return hipErrorInvalidValue;
    const FitPrior pr = fit_prior(K, pm, pw);
    const CompBeltIn ii{data, phi, seed, G, phi_tables ? 1 : 0};
    const CompBeltOut o{exceed, tally, wobs, qobs, thobs, theta, stat, words, data_all};
    const double kuf = fit_ku(lg, 2 + K), kuh = fit_ku(lg, K);
    const dim3 block(kEvThreads);
    const int M = g.T + 1;
    constexpr long long kRange = 1ll << 22;   // units a launch: 2^22 blocks of 256 threads stay below 2^32 threads on x
    for (long long ua = 0; ua < units; ua += kRange) {
        const dim3 grid((unsigned)(units - ua < kRange ? units - ua : kRange), 1, (unsigned)pslices);
        const int u0 = (int)ua;
        switch (K) {
        case 0: hipLaunchKernelGGL((k_composition_belt<3>), grid, block, 0, s, R3, S, bg, T, pr, kuf, kuh, ii, o, u0, nrb, M, C, lg, Q, P); break;
        case 1: hipLaunchKernelGGL((k_composition_belt<4>), grid, block, 0, s, R3, S, bg, T, pr, kuf, kuh, ii, o, u0, nrb, M, C, lg, Q, P); break;
        case 2: hipLaunchKernelGGL((k_composition_belt<5>), grid, block, 0, s, R3, S, bg, T, pr, kuf, kuh, ii, o, u0, nrb, M, C, lg, Q, P); break;
        case 3: hipLaunchKernelGGL((k_composition_belt<6>), grid, block, 0, s, R3, S, bg, T, pr, kuf, kuh, ii, o, u0, nrb, M, C, lg, Q, P); break;
        default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_composition_accept(int npairs, int G, int P, double alpha, const int* exceed, const int* tally,
                                     const int* wobs, const double* qobs, int* accept, int* status, int* best, hipStream_t s)
{
    if (npairs <= 0) return hipSuccess;
    const unsigned nb = (unsigned)(((long long)npairs + kBeltAcceptThreads - 1) / kBeltAcceptThreads);
    hipLaunchKernelGGL(k_composition_accept, dim3(nb), dim3(kBeltAcceptThreads), 0, s, exceed, tally, wobs, qobs, G, P, alpha,
                       npairs, accept, status, best);
    return hipGetLastError();
}

}  // namespace nusi
