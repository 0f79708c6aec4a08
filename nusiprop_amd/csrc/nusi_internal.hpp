// nuSIprop MI355X -- internal interfaces between the C-ABI host layer and the kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "nusi.h"
#include "nusi_physics.hpp"

namespace nusi {

// Grid shared by every point of a batch (constructor, nuSIprop.hpp:113-128, and
// the table axis of evolve(), nuSIprop.hpp:224-233).  Device pointers.
struct GridDev {
    int N, Nz, T;
    long long PT;          // alpha entries per point = T(T-1)/2
    const double* Emin;    // [N]
    const double* Emax;    // [N]
    const double* lo;      // [T] table-axis bin edges
    const double* hi;      // [T]
    const double* z;       // [Nz]
    const double* step_c;  // [Nz] c_i = (1+z[i-1]) dlogz / H(z[i-1]), index i (0 unused)
    const double* step_s;  // [Nz] s_i = n_nu(z[i-1]) / (1+z[i-1])^2
    const double* sfr;     // [Nz] get_SFR(z[i])
};

// Device tables of one batch.  alpha is stored transposed and packed:
// alpha(n, m), n < m, lives at m(m-1)/2 + n, so that the cascade's column
// reads (all n < m for one m) are contiguous.
struct TablesDev {
    double* G;    // [npts][T]
    double* At;   // [npts][T]
    double* A;    // [npts][PT]
    double* Med;  // [npts][3][kMedFields T]: member edge leaves of every bin edge (k_alpha_medge)
    double* Src;  // [npts][T (Nz-1)]: the source terms c_i Lum of every point that is not the power law (k_source_dsnb,
                  // k_source_tab; diagonal layout), or nullptr
    int* Wmin;    // [npts][4][T] or nullptr (only the base plan of NUSI_OPT_SHIFT_REUSE): per warning bit b and table
                  // row n, the smallest column m of an entry (n, m) that raised it (Gamma / alphaTilde: m = n), so
                  // that k_table_shift passes on exactly the warnings of the rows a shifted slot reads
    double* Kt = nullptr;   // [npts][3][PT][8] or nullptr: the k-split alpha path of calls of few tables
                            // (launch_alpha): each mass state's terms of every entry, summed in order by k_alpha_ksum
    double* Gpre = nullptr;   // [npts][3][kGaPreFields][T] or nullptr: the reference order's Gamma / alphaTilde
                              // dilogarithms of calls of few tables (k_ga_dilogs, launch_gamma_alphat)
};

// Tiles of the alpha table for k_alpha_tile: kAlphaTile x kAlphaTile (n, m) bin blocks with
// tn <= tm, in three launch classes by how many distinct bin edges a side has
// (bins of the first N share edges, redshift-extended bins do not), which sets
// each class's LDS footprint.  tiles[]: kTileWords words per tile (alpha_tile_decode, nusi_alpha_tiles.hpp).
struct AlphaTilesDev {
    int* tiles = nullptr;   // device [ncore + nmixed + nfull][kTileWords]
    int ncls[3] = {0, 0, 0};
    int cs_max[3] = {0, 0, 0}, ct_max[3] = {0, 0, 0};
};
// Classify the tiles of a grid on the host; `shared[n]` = (hi[n] == lo[n+1]) bitwise.
hipError_t alpha_tiles_create(int T, const unsigned char* shared, AlphaTilesDev* out);
void alpha_tiles_destroy(AlphaTilesDev* t);

// NUSI_OPT_REFERENCE_ORDER on the big-batch kernel: the member corners (Dc, A of alpha_member_ref) of every table, mass
// state and corner, evaluated by k_alpha_mcorner before k_alpha_batch reads them.  A corner is a pair of distinct bin
// edges (S' edge us, t edge ut <= us; the edges numbered 0 .. U-1 along the table axis, an edge two neighbouring bins
// share counted once): c = us (us + 1) / 2 + ut, NC = U (U + 1) / 2.  The block of a batch of nb tables starting at
// slot p0 is buf + (p0 - pc0) 6 NC, laid out [k][q][c][Dcr, Dci] (a tile's corner rows contiguous; A = carg(..) is
// formed by the batch kernel); a launch chunk of batches whose tables fit cap_tables starts at table pc0.
struct MCornerDev {
    double* buf = nullptr;   // [cap_tables][3][NC][2]
    int* eu = nullptr;       // [2 T]: edge number of bin edge 2 b + side (side 0: lo[b], 1: hi[b])
    double* ue = nullptr;    // [U]: the energy of each edge
    long long NC = 0;
    int U = 0, cap_tables = 0;
    int* ub = nullptr;       // [2 U]: the bins an edge bounds (ga_batch_edge_bins; k_ga_dilogs_batch)
};
// Scans in the reference order: Gamma / alphaTilde's dilogarithms per alpha batch (k_ga_dilogs_batch) in one
// plan-owned block buf of `bytes`, laid out per launch chunk of whole batches (nt tables, nk batches; ga_batch_bytes):
// [nt][3][ga_gdep_doubles] the values that read gr, [nk][3][ga_shared_doubles] the batch's shared ones, [nt] ints: the
// batch of each table.  eu, ue, ub, U: the plan's distinct edges (MCornerDev's).
struct GaBatchDev {
    char* buf = nullptr;
    size_t bytes = 0;
    const int* eu = nullptr;
    const double* ue = nullptr;
    const int* ub = nullptr;
    int U = 0;
};
struct GaBatchView {   // one chunk's blocks as k_gamma_alphat<true, 1, true> reads them (pc0: its first table)
    const double* gd = nullptr;
    const double* sh = nullptr;
    const int* tb = nullptr;
    const int* eu = nullptr;
    int U = 0, pc0 = 0;
};
size_t ga_batch_bytes(int T, int U, int ntab, int nbatch);
void ga_batch_edge_bins(int T, const std::vector<int>& eu, int U, std::vector<int>& ub);
// ref: NUSI_OPT_REFERENCE_ORDER (the kernels' kRef instances: the reference's own operation order for the complex
// dilogarithms and the s-t interference member leaves, bit-identical to the oracle's ora_set_reference_order(1))
size_t gamma_alphat_pre_doubles(int T, int npts);   // TablesDev::Gpre's size
// gb != nullptr (ref only): the batch path -- k_ga_dilogs_batch over the call's alpha batches (device `batches`, the
// same in host memory h_batches; they cover the tables 0 .. npts - 1 in order), then k_gamma_alphat<true, 1, true>,
// in chunks of whole batches that fit gb->bytes (one chunk, and one dispatch of each kernel, where the call fits)
hipError_t launch_gamma_alphat(const GridDev& g, const Point* pts, int npts, const SplineSet* spl, TablesDev t,
                               int* warn, hipStream_t s, bool ref, const GaBatchDev* gb = nullptr,
                               const int* batches = nullptr, const int* h_batches = nullptr, int nbatches = 0);
const char* last_ga_kernel();   // what the latest launch_gamma_alphat on this thread ran (nusi_plan_ga_kernel)
// batches: device [nbatches] of first table | count << 24 (count <= gmax), tables of a batch sharing
// m_phi, the masses and the channel flags (nullptr: every table alone).  kernel = NUSI_OPT_ALPHA_KERNEL:
// 0 -- core tiles on the big-batch kernel k_alpha_batch (any count < 256; the first nb_plain batches without
// the phi-phi channel, the rest with it); 1 -- k_alpha_tile<G> batches (count <= 4); 2 -- one entry per
// work-item (k_alpha).  h_batches: the same batches in host memory, and mc the member-corner block (both read
// only by kernel 0 with ref: k_alpha_mcorner + k_alpha_batch in chunks of batches of <= mc->cap_tables tables)
hipError_t launch_alpha(const GridDev& g, const Point* pts, int npts, const SplineSet* spl, const AlphaTilesDev& tiles,
                        TablesDev t, int* warn, hipStream_t s, const int* batches, int nbatches, int gmax,
                        int kernel, int nb_plain, bool ref, const int* h_batches = nullptr,
                        const MCornerDev* mc = nullptr);
// the edge numbering of MCornerDev for a table axis (hi[n] == lo[n + 1] bitwise: one edge): eu [2 T], ue [U]
void mcorner_edges(int T, const double* lo, const double* hi, std::vector<int>& eu, std::vector<double>& ue);
// NUSI_OPT_SHIFT_REUSE: tables s0 .. s0 + nshift - 1 of t (grid g) <- base tables map[q].x of tb (grid gb, the
// axis extended on top), read map[q].y bins higher; warn[s] |= the warning bits of the base rows the slot reads
// (tb.Wmin, required)
hipError_t launch_table_shift(const GridDev& g, const GridDev& gb, const int2* map, int s0, int nshift, TablesDev tb,
                              TablesDev t, int* warn, hipStream_t s);
// The block-synchronous MFMA cascade (k_cascade_bs, round 4): workgroup k takes the grp[k].y <= P points gidx[grp[k].x
// ..] that share one table slot (gidx == grp == nullptr: P = 1, point k), P = 1, 2 or 16 (the gamma batch), any source
// and scattering mode, step passes on any grid that fits; fh: a FIFO of cascade_bs_scratch_doubles per workgroup
// (used when the steps take more than one pass).  cascade_bs_config: 0 = the grid does not fit P.
// force_passes (NUSI_OPT_STEP_PASSES = 1, P = 1): the step-pass instance even where one pass fits.
int cascade_bs_config(const GridDev& g, int P, bool force_passes);
size_t cascade_bs_scratch_doubles(const GridDev& g, int P);
hipError_t launch_cascade_bs(const GridDev& g, const Point* pts, int P, const int* gidx, const int2* grp, int nwg,
                             TablesDev t, double* fh, double* flux, double* flux_fla, hipStream_t s, bool all_nr,
                             bool force_passes);
// The impulse cascade k_cascade_bs_impulse (nusi_plan_response): the response matrix G[p][n][3][N] of the points
// pts[p0 .. p0 + npts) -- column n the fluxes of a unit source in source-axis bin n (S = e_n, norm = 1, redshift
// weights w [Nz], device) -- written at G / G_fla + ((p (T + 1) + n) 3 N) for n = 1 .. T (column 0 is the caller's
// memset; either output may be nullptr).  cascade_impulse_groups workgroups per point, 16 bins each; fh: a FIFO of
// cascade_impulse_scratch_doubles per point of the launch (step passes).  cascade_impulse_fits: the grid fits.
bool cascade_impulse_fits(const GridDev& g);
int cascade_impulse_groups(const GridDev& g);
size_t cascade_impulse_scratch_doubles(const GridDev& g);
hipError_t launch_cascade_impulse(const GridDev& g, const Point* pts, int p0, int npts, const double* w, TablesDev t,
                                  double* fh, double* G, double* G_fla, hipStream_t s, bool all_nr);
// k_response_apply: out[t][q][r] = scale[q] sum_n G[t][n][r] S[q][n] (n ascending from 1, no fma) over the 3 N rows
// of ntab resident response matrices; S [Q][T + 1], scale [Q] (or nullptr), G and out in device memory
hipError_t launch_response_apply(const GridDev& g, const double* G, int ntab, const double* S, int Q, const double* scale,
                                 double* out, hipStream_t s);
// The detector of a plan (nusi_detector.hip).  k_detector_fold: out[t][n][c] = sum_r X[t][n][r] D[c][r] (+ bg[c] where
// bg != nullptr) over the 3 N entries of ntab x rows rows, on the fp64 matrix cores; Dt is the plan's K-major copy of
// D, [3 N][detector_ld(C)] with zero-padded columns; tri: X is a response matrix (rows = T + 1), whose entries of
// bins b >= n are +0.0 and are not read.  k_detector_events: mu[t][q][c] = scale[q] (sum_n R[t][n][c] S[q][n]) + bg[c]
// (n ascending from 1, no fma) and nll[t][q] = sum_c mu - data log mu; S [Q][T + 1], scale [Q] (or nullptr), data [C]
// (with nll), bg [C], all in device memory; mu or nll may be nullptr.
int detector_ld(int C);
hipError_t launch_detector_fold(const GridDev& g, const double* X, int ntab, int rows, bool tri, const double* Dt, int C,
                                const double* bg, double* out, hipStream_t s);
hipError_t launch_detector_events(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* scale,
                                  const double* data, const double* bg, int C, double* mu, double* nll, hipStream_t s);
// k_detector_profile: per (t, q) the a >= 0 minimising the statistic of a s + bg (include/nusi.h); ahat, nll [ntab][Q],
// mu [ntab][Q][C], status [ntab][Q] in device memory, all but ahat may be nullptr
hipError_t launch_detector_profile(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                                   const double* bg, int C, double* ahat, double* nll, double* mu, int* status,
                                   hipStream_t s);
// k_detector_fit: per (t, q) the theta >= 0 [1 + K] minimising the statistic of theta_0 s + sum_j theta_j T_j + bg with
// the priors' penalties (include/nusi.h); T [K][C] in device memory, pm and pw [K] the priors' means and weights on
// the host; theta [ntab][Q][1 + K], nll, mu, status as the profile's, all but theta may be nullptr
hipError_t launch_detector_fit(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                               const double* bg, int C, int K, const double* T, const double* pm, const double* pw,
                               double* theta, double* nll, double* mu, int* status, hipStream_t s);
// k_components_fit<J, J + K>: the fit with J = 2 .. 3 signal components per (table, spectrum), R3 [ntab][J][M][C], and
// K = 0 .. 3 templates (T, pm, pw: unread at K = 0); theta [ntab][Q][J + K]
hipError_t launch_components_fit(const GridDev& g, const double* R3, int ntab, int J, const double* S, int Q,
                                 const double* data, const double* bg, int C, int K, const double* T, const double* pm,
                                 const double* pw, double* theta, double* nll, double* mu, int* status, hipStream_t s);
// k_ensemble_profile (K = 0) / k_ensemble_fit<1 + K>: P data sets data [P][C] (device memory), per (p, t) the best
// spectrum's record under the key of include/nusi.h: q, nll, status [P][ntab], theta [P][ntab][1 + K] in device memory,
// theta and status may be nullptr.  Grid (ntab, qslices, pslices): 1 <= qslices <= ensemble_blocks(C, K, Q) (the
// spectrum blocks per table), 1 <= pslices <= P.  With qslices > 1 the slices' records go to scratch --
// qslices P ntab ensemble_record_bytes(K) bytes of device memory -- and k_ensemble_best merges them.
size_t ensemble_record_bytes(int K);
int ensemble_blocks(int C, int K, int Q);
hipError_t launch_detector_ensemble(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                                    int P, const double* bg, int C, int K, const double* T, const double* pm,
                                    const double* pw, int qslices, int pslices, void* scratch, int* oq, double* onll,
                                    double* otheta, int* ostatus, hipStream_t s);
// k_conditional_fit<K>: the fit's iteration on the K templates alone with the signal's scale held at scale [Q] (device
// memory, entries >= 0): theta [ntab][Q][1 + K] (theta_0 = the scale, copied), nll, mu, status as the fit's
hipError_t launch_conditional_fit(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* scale,
                                  const double* data, const double* bg, int C, int K, const double* T, const double* pm,
                                  const double* pw, double* theta, double* nll, double* mu, int* status, hipStream_t s);
// k_interval<1 + K>: the best fit (the profile's at K = 0, the fit's else) and the roots of lambda(a) = delta / 2 on the
// sides `which` asks for (include/nusi.h): lo, hi, nll_hat [ntab][Q], theta_hat [ntab][Q][1 + K], status [ntab][Q][3] in
// device memory; any may be nullptr (a side asked for must not be: the caller checks)
hipError_t launch_detector_limit(const GridDev& g, const double* R, int ntab, const double* S, int Q, const double* data,
                                 const double* bg, int C, int K, const double* T, const double* pm, const double* pw,
                                 double delta, int which, double* lo, double* hi, double* theta_hat, double* nll_hat,
                                 int* status, hipStream_t s);
// k_toys_limit<1 + K> and k_toys_band (nusi_plan_response_ensemble_limit).  The work of a call is cut into units: unit u
// is table u / nqb and spectrum block u % nqb, nqb = ceil(Q / QB), QB = toys_limit_block(C) spectra.  launch_toys_limit
// runs units u0 .. u0 + nu - 1 against the P data sets data [P][C] (device memory) in `pslices` slices: a side's limits
// go to lo / hi (nullptr: not kept) -- compact: the chunk's scratch [nu QB][P], else the call's [ntab][Q][P] --, the
// side words to words [ntab][Q][P][2] and the counted flags are ADDED to tally [ntab][Q][2][4] (either may be nullptr).
// launch_toys_band selects the NR ranks rank [NR] (device memory, 0 <= r < P) of those units' limits into band_lo,
// band_hi [ntab][Q][NR] (nullptr: skipped; a side without values, lo / hi == nullptr: NaN).
int toys_limit_block(int C);
hipError_t launch_toys_limit(const GridDev& g, const double* R, const double* S, int Q, const double* data, int P,
                             const double* bg, int C, int K, const double* T, const double* pm, const double* pw,
                             double delta, int which, int u0, int nu, int pslices, double* lo, bool lo_compact, double* hi,
                             bool hi_compact, int* words, int* tally, hipStream_t s);
hipError_t launch_toys_band(int C, int Q, int P, int u0, int nu, const double* lo, bool lo_compact, const double* hi,
                            bool hi_compact, double* band_lo, double* band_hi, const int* rank, int NR, hipStream_t s);
// k_poisson_draw: out[row][p][c] = a Poisson count around mu[row][c] under the identity (seed, stream, row, p, c) of
// include/nusi.h ("Drawing counts"); mu [rows][C] and out [rows][P][C] in device memory, rows P C <= NUSI_DRAW_COUNTS_MAX
hipError_t launch_poisson_draw(const double* mu, int rows, int C, int P, unsigned long long seed, unsigned stream, double* out,
                               hipStream_t s);
// k_normal_draw: out[row][p][j] = draw::normal0(center[row][j], sigma[j]) under the identity (seed, stream, row, p, j) of
// include/nusi.h ("Drawing normals"); cs = center [rows][J] then sigma [J], and out [rows][P][J], in device memory
hipError_t launch_normal_draw(const double* cs, int rows, int J, int P, unsigned long long seed, unsigned stream, double* out,
                              hipStream_t s);
// (launch_inject, launch_belt: ps [K] the priors' widths, +inf = none, and toys = NUSI_TOYS_*, the toys' ensemble; where
// it randomises nothing -- NUSI_TOYS_FIXED, K = 0, no pw > 0 -- the FIXED instance runs)
// k_inject<1 + K>: the calibration call (include/nusi.h nusi_plan_response_inject) on launch_toys_limit's units u0 ..
// u0 + nu - 1 and p-slices: per (t, q, p) a toy drawn from a_inj[q] s + sum_j th_inj[j] T_j + bg under (seed, stream = t,
// row = q, p, c), its best fit, the conditional fit at a_test[q] and the statistic under `mode`.  a_inj, a_test [Q] and
// qobs [ntab][Q] (or nullptr) in device memory, th_inj [K] on the host.  theta_hat_0 and the statistic per toy go to
// theta / stat (nullptr: not kept; compact: the chunk's scratch [nu QB][P], else the call's [ntab][Q][P]) -- the layout
// launch_toys_band selects from --, the words to words [ntab][Q][P][2], the drawn counts to data [ntab][Q][P][C], and the
// counts are ADDED to tally [ntab][Q][4] and exceed [ntab][Q] (any may be nullptr).
hipError_t launch_inject(const GridDev& g, const double* R, const double* S, int Q, const double* a_inj, const double* a_test,
                         const double* th_inj, const double* qobs, int P, unsigned long long seed, int mode, const double* bg,
                         int C, int K, const double* T, const double* pm, const double* pw, const double* ps, int toys, int u0,
                         int nu, int pslices, double* theta, bool theta_compact, double* stat, bool stat_compact, int* words,
                         int* tally, int* exceed, double* data, hipStream_t s);
// k_belt<1 + K> and k_belt_accept (include/nusi.h nusi_plan_response_belt).  A record is (t, q, g) with row q G + g of a
// table's Q G rows; a unit is one table and belt_block(C) rows.  launch_belt runs the units that hold the rows of the
// pairs t Q + q = pr0 .. pr1 - 1 and stores those pairs' records alone: the observed side to qobs [ntab][Q][G], thobs
// [ntab][Q][1 + G][1 + K] and wobs [.][1 + G]; the toys' records to theta, stat [ntab][Q][G][P], words [..][P][2] and
// data_all [..][P][C]; the counts are ADDED to exceed [.][G] and tally [.][G][4].  exceed, tally and wobs are indexed by
// the pair, or by pair - pr0 where compact (the chunk's scratch).  data [C], frac [G] and ref [ntab][Q] (nullptr: 1) in
// device memory.  launch_belt_accept forms lo, hi [ntab][Q], idx [ntab][Q][2] and status [ntab][Q] of those pairs from
// exceed, tally and wobs.  Any output may be nullptr.
int belt_block(int C);
hipError_t launch_belt(const GridDev& g, const double* R, const double* S, int Q, const double* data, const double* frac,
                       int G, const double* ref, int P, unsigned long long seed, int mode, const double* bg, int C, int K,
                       const double* T, const double* pm, const double* pw, const double* ps, int toys, int pr0, int pr1,
                       int pslices, int* exceed, bool exceed_compact, int* tally, bool tally_compact, int* wobs,
                       bool wobs_compact, double* qobs, double* thobs, double* theta, double* stat, int* words, double* data_all,
                       hipStream_t s);
hipError_t launch_belt_accept(const double* frac, int G, const double* ref, int P, double alpha, int pr0, int pr1,
                              const int* exceed, bool exceed_compact, const int* tally, bool tally_compact, const int* wobs,
                              bool wobs_compact, double* lo, double* hi, int* idx, int* status, hipStream_t s);
// k_composition_belt<3 + K>, k_composition_accept (include/nusi.h nusi_plan_response_composition_belt): R3
// [ntab][3][M][C], S [Q][M], data [C] and phi [G][3] (phi_tables: [ntab][G][3]) in device memory; a unit is one table
// and composition_belt_block(C) of its Q G rows, and the launcher cuts the units into ranges a grid can hold.  The
// observed side goes to qobs [ntab][Q][G], thobs [ntab][Q][1 + G][3 + K] and wobs [ntab][Q][1 + G]; the toys' records to
// theta [ntab][Q][G][P][3 + K], stat [..][P], words [..][P][2] and data_all [..][P][C]; the counts are ADDED to exceed
// [ntab][Q][G] and tally [..][4].  launch_composition_accept forms accept [ntab][Q][G], status and best [ntab][Q] from
// exceed, tally, wobs and qobs.  Any output may be nullptr.
int composition_belt_block(int C);
hipError_t launch_composition_belt(const GridDev& g, const double* R3, int ntab, const double* S, int Q, const double* data,
                                   const double* phi, bool phi_tables, int G, int P, unsigned long long seed, const double* bg,
                                   int C, int K, const double* T, const double* pm, const double* pw, int pslices,
                                   int* exceed, int* tally, int* wobs, double* qobs, double* thobs, double* theta, double* stat,
                                   int* words, double* data_all, hipStream_t s);
hipError_t launch_composition_accept(int npairs, int G, int P, double alpha, const int* exceed, const int* tally,
                                     const int* wobs, const double* qobs, int* accept, int* status, int* best, hipStream_t s);
size_t cascade_src_doubles(const GridDev& g);   // t.Src doubles per point
hipError_t launch_source_dsnb(const GridDev& g, const Point* pts, int npts, double* src, hipStream_t s);
// Tabulated sources (NUSI_SOURCE_TABULATED + slot): `slots` is the plan's slot storage in device memory,
// cascade_slot_doubles per slot (S [T + 1], then w [Nz]), passed by pointer (an indexed by-value aggregate ends up in
// scratch).  launch_source_tab fills the t.Src rows of the call's tabulated points for the MFMA cascade.
size_t cascade_slot_doubles(const GridDev& g);
hipError_t launch_source_tab(const GridDev& g, const Point* pts, int npts, const double* slots, double* src,
                             hipStream_t s);
// The bit-exact scalar cascade k_cascade (NUSI_CASCADE_WAVEFRONT / REG / LDS all select it): one wavefront per
// point, any N.  It reads no t.Src: a tabulated point's source comes straight from `slots` (nullptr where the call
// has no such point), through the expression k_source_tab uses.
hipError_t launch_cascade_exact(const GridDev& g, const Point* pts, int npts, TablesDev t, const double* slots,
                                double* flux, double* flux_fla, hipStream_t s);

// The mass-resolved response (nusi_plan_response_mass; include/nusi.h): G3[p][j][n][3][N], the response to a unit source
// in mass state j alone.  k_cascade_mass_impulse is the impulse cascade with the source in one row (three times its
// workgroups and FIFO per table; p0, npts, w, fh as launch_cascade_impulse); k_cascade_mass is the scalar cascade with
// the source per row, on the columns col0 .. col0 + npts - 1 of the call in the order [p][j][n] (pts[c]: the column's
// tabulated point record on the unit-vector slot n, norm = 3).
hipError_t launch_cascade_mass_impulse(const GridDev& g, const Point* pts, int p0, int npts, const double* w, TablesDev t,
                                       double* fh, double* G3, double* G3_fla, hipStream_t s, bool all_nr);
hipError_t launch_cascade_mass_exact(const GridDev& g, const Point* pts, int npts, TablesDev t, const double* slots,
                                     double* flux, double* flux_fla, long long col0, hipStream_t s);
// k_response_compose: out[t][c][x] = (kappa[t][c][0] A[t][0][x] + kappa[t][c][1] A[t][1][x]) + kappa[t][c][2] A[t][2][x],
// no fma; A [ntab][3][X], kappa [ntab][Qc][3] and out [ntab][Qc][X] in device memory, ntab ceil(X / 256) < 2^31
hipError_t launch_response_compose(const double* A, int ntab, size_t X, const double* kappa, int Qc, double* out,
                                   hipStream_t s);

// 4 x 4 windows of a 3-D spline table f [n0][n1][n2] into fw [n0 n1 n2][16] (synchronous)
hipError_t spline_windows_build(const float* f, int n0, int n1, int n2, float* fw);

// names of the main alpha-table / cascade kernels the latest launch_alpha / launch_cascade_* on this
// thread chose (static strings; nusi_plan_kernels)
const char* last_alpha_kernel();
const char* last_cascade_kernel();

}  // namespace nusi
