/*
 * nusi.h -- C ABI of the MI355X-native nuSIprop cascade solver (libnusi.so).
 *
 * Drop-in boundary for the reference's calculate_flux / pyprop surface
 * (quarkquartet/nuSIprop @ 2025-02-13).  Plain C types only: pointers, sizes,
 * ints and doubles.  Every function returns 0 on success or a negative
 * NUSI_E* code; nusi_last_error() gives the message (thread-local).  Nothing
 * in the library calls exit(): the C++ facade (include/nuSIprop.hpp) maps
 * errors back to the reference's stderr text + exit(1).
 *
 * Two levels:
 *   1. object API -- one parameter point, host-side results, the exact
 *      semantics of nuSIprop::calculate_flux (each entry cites the member it
 *      replaces, nuSIprop.hpp:line);
 *   2. plan API   -- a batch of parameter points sharing one energy/redshift
 *      grid, evolved on one GPU with device-resident inputs/outputs (the
 *      MI355X throughput path; multi-GPU = one plan per device, no
 *      collectives).
 * All arithmetic is IEEE fp64.  The table build and the cascade run as HIP
 * kernels on the GPU; there is no CPU fallback -- without a usable GPU the
 * calls fail with NUSI_EHIP.
 */
#ifndef NUSI_H
#define NUSI_H

#ifdef __cplusplus
extern "C" {
#endif

/* error codes */
#define NUSI_OK 0
#define NUSI_EPARAM -1        /* bad parameters / range                          */
#define NUSI_ENOSPECTRUM -2   /* no neutrino mass spectrum (aux.hpp:48-49)       */
#define NUSI_ETABLE -3        /* phi-phi table missing (interp.hpp:251-254)      */
#define NUSI_EINTERP -4       /* phi-phi lookup out of bounds (interp.hpp:355-361) */
#define NUSI_EHIP -5          /* HIP runtime error / no GPU                      */
#define NUSI_ESTATE -6        /* call order (e.g. results before evolve)         */

/* source models.  DSNB is the reference's active Lum (nuSIprop.hpp:659-662);
 * POWER_LAW is its commented-out power law (nuSIprop.hpp:656) used by the
 * BASELINE workloads. */
#define NUSI_SOURCE_DSNB 0
#define NUSI_SOURCE_POWER_LAW 1
/* Extension (the reference fixes its source at compile time, Lum() of
 * nuSIprop.hpp:648-662): source_model = NUSI_SOURCE_TABULATED + slot selects
 * the user-tabulated source phi(E') W(z) registered in that slot of the plan
 * (nusi_plan_set_source / nusi_set_source below).  For such a point `norm` is
 * absolute (no flux_FS_E0 division) and `si` is ignored; like both built-in
 * sources, the three mass states get equal thirds.  The source term of bin b
 * at redshift step i is, for each mass state,
 *     step_c[i] * ((norm / 3.0) * (w[i] / (1 + z[i])) * S[b + i]). */
#define NUSI_SOURCE_TABULATED 2

/* warning bits (negative cross sections, nuSIprop.hpp:909-918, 1215-1231, 1505-1516) */
#define NUSI_WARN_GAMMA 1
#define NUSI_WARN_ALPHATILDE 2
#define NUSI_WARN_ALPHA 4

/* All constructor arguments of calculate_flux (nuSIprop.hpp:61-65), in order,
 * plus the source model.  Defaults of the reference C++ constructor:
 * norm=1, majorana=1, non_resonant=1, normal_ordering=1, N_bins_E=300,
 * lEmin=12, lEmax=17, zmax=5, flav=2, phiphi=0 (see nusi_params_default). */
typedef struct nusi_params {
    double mphi;        /* mediator mass [eV]                      */
    double g;           /* coupling                                */
    double mntot;       /* sum of neutrino masses [eV]             */
    double si;          /* spectral index                          */
    double norm;        /* free-streaming normalisation at 100 TeV */
    int majorana;
    int non_resonant;
    int normal_ordering;
    int N_bins_E;
    double lEmin;
    double lEmax;
    double zmax;
    int flav;           /* 0=e 1=mu 2=tau */
    int phiphi;
    int source_model;   /* NUSI_SOURCE_*; NUSI_SOURCE_TABULATED + slot */
} nusi_params;

/* Fills the reference C++ constructor defaults (nuSIprop.hpp:61-65) around
 * the four mandatory parameters; source_model = NUSI_SOURCE_DSNB. */
void nusi_params_default(nusi_params *p, double mphi, double g, double mntot, double si);

const char *nusi_last_error(void);
int nusi_device_count(void);

/* ---------------------------------------------------------------------------
 * 1. object API  (nuSIprop::calculate_flux)
 * ------------------------------------------------------------------------- */
typedef struct nusi_handle nusi_handle;

/* calculate_flux(mphi, g, mntot, si, norm, ...)   nuSIprop.hpp:61-171.
 * Builds the energy/redshift grid and the mixing matrix.  With
 * non_resonant && phiphi the phi-phi tables are loaded like the reference,
 * from xsec/alphatilde_phiphi.bin and xsec/alpha_phiphi.bin relative to the
 * current directory (or $NUSI_XSEC_DIR), -> NUSI_ETABLE if missing.
 * The object evolves on GPU `$NUSI_DEVICE` (default 0) with the default
 * (NUSI_CASCADE_AUTO) kernels. */
int nusi_create(const nusi_params *p, nusi_handle **out);
/* copy constructor / operator=  (nuSIprop.hpp:434-525) */
int nusi_copy(const nusi_handle *src, nusi_handle **out);
void nusi_destroy(nusi_handle *h);
/* the public members mphi, g, mntot, si, norm  (nuSIprop.hpp:174) */
int nusi_set_params(nusi_handle *h, double mphi, double g, double mntot, double si, double norm);
int nusi_get_params(const nusi_handle *h, double *mphi_g_mntot_si_norm /* [5] */);
/* evolve()  (nuSIprop.hpp:176-337) */
int nusi_evolve(nusi_handle *h);
/* check_energy_conservation()  (nuSIprop.hpp:339-357): calls evolve() */
int nusi_check_energy_conservation(nusi_handle *h, double *out);
/* Tabulated source of one object (no reference counterpart).  nusi_source_axis
 * is nusi_plan_source_axis on the object's grid.  nusi_set_source registers S
 * (and w, or NULL) in slot 0 of the object's plan and switches the object to
 * it; S == NULL returns the object to its constructor's source_model.
 * nusi_copy keeps the source.  nusi_check_energy_conservation on an object
 * with a tabulated source returns NUSI_EPARAM: its free-streaming energy is
 * defined for the power law only, and bin integrals do not determine the
 * spectrum's energy integral. */
int nusi_source_axis(const nusi_handle *h, int *M, double *lo, double *hi, double *z);
int nusi_set_source(nusi_handle *h, const double *S, const double *w);
/* The response matrix of the object's parameter point (no reference
 * counterpart): nusi_plan_response_host on the object's plan, G / G_fla
 * [M][3][N] host arrays (either may be NULL), w [Nz] or NULL.  The object's
 * fluxes, its source (nusi_set_source) and the plan's slots are not involved. */
int nusi_response(nusi_handle *h, const double *w, double *G, double *G_fla);
/* ... and its mass-resolved response (nusi_plan_response_mass_host, below):
 * G3 / G3_fla [3][M][3][N] host arrays, either may be NULL. */
int nusi_response_mass(nusi_handle *h, const double *w, double *G3, double *G3_fla);
/* results of the last evolve(), row-major [k][b] (mass basis) / [f][b] (flavour) */
int nusi_get_flux(const nusi_handle *h, double *out_3xN);      /* get_flux(i,j)     :359-381 */
int nusi_get_flux_fla(const nusi_handle *h, double *out_3xN);  /* get_flux_fla(i,j) :383-405 */
int nusi_get_energies(const nusi_handle *h, double *out_N);    /* get_energy(i)     :412-429 */
int nusi_get_N_bins_E(const nusi_handle *h);                   /* get_N_bins_E()    :407-410 */
int nusi_get_N_steps_z(const nusi_handle *h);
int nusi_get_warnings(const nusi_handle *h);                   /* NUSI_WARN_* of the last evolve */
/* names of the alpha-table and cascade kernels this object's last evolve() launched (strings owned by the object,
 * valid until its next evolve() or nusi_destroy; a nusi_copy keeps its source's names); no reference
 * counterpart -- reports and tests) */
int nusi_get_kernels(const nusi_handle *h, const char **alpha, const char **cascade);
/* nusi_plan_set_option on the object's plan (NUSI_OPT_*; kept by nusi_copy).  No reference counterpart. */
int nusi_set_option(nusi_handle *h, int option, int value);

/* ---------------------------------------------------------------------------
 * 2. plan API -- batched parameter scans on one GPU
 * ------------------------------------------------------------------------- */
typedef struct nusi_plan nusi_plan;

/* One plan = one device, one grid (N_bins_E, lEmin, lEmax, zmax), room for
 * max_points points per call (tables for all of them stay in HBM). */
int nusi_plan_create(int device, int N_bins_E, double lEmin, double lEmax, double zmax, int max_points,
                     nusi_plan **out);
void nusi_plan_destroy(nusi_plan *plan);
/* Load the phi-phi tables (float32 records {x0..x_{d-1}, f}, last index
 * fastest; interp.hpp:249-291).  dims == NULL -> the reference's
 * {5000,100} and {1000,1000,100} (nuSIprop.hpp:168-169). */
int nusi_plan_load_phiphi(nusi_plan *plan, const char *alphatilde_path, const int *alphatilde_dims,
                          const char *alpha_path, const int *alpha_dims);
int nusi_plan_grid(const nusi_plan *plan, int *N, int *Nz, double *Enu /* [N] or NULL */);
/* Tabulated sources (no reference counterpart).  A plan holds numbered source
 * slots; a point with source_model = NUSI_SOURCE_TABULATED + slot reads its
 * source from that slot.
 * The SOURCE AXIS has M = N + Nz - 1 bins: bins 0 .. N-1 are the energy bins,
 * bin N-1+j is [Emin[N-1] (1 + z_j), Emax[N-1] (1 + z_j)] for j = 1 .. Nz-1 --
 * the bins a redshifted energy bin can come from.  nusi_plan_source_axis
 * returns M, the bin edges lo / hi [M] and the redshift grid z [Nz]; any
 * pointer may be NULL.
 * nusi_plan_set_source fills `slot` (0 .. NUSI_SOURCE_SLOTS_MAX - 1; storage
 * grows on demand) with
 *   S [M]   the spectrum's integral over each source-axis bin, in the
 *           source's frame (bin 0 is never read: there is no source at
 *           redshift step 0);
 *   w [Nz]  the redshift weight W(z_i) in place of the star-formation rate
 *           get_SFR(z_i) (nuSIprop.hpp:591-605); NULL = get_SFR.
 * The vectors are copied (the caller may free them).  The call is ordered
 * with the plan's calls: earlier evolves finish with the old contents, later
 * ones see the new.  S == NULL clears the slot.  NUSI_EPARAM for a slot out
 * of range or a non-finite or negative entry (the cascade relies on every
 * summed term being non-negative), and -- from the evolve calls -- for a point
 * whose slot is empty. */
#define NUSI_SOURCE_SLOTS_MAX 65536
int nusi_plan_source_axis(const nusi_plan *plan, int *M, double *lo /* [M] */, double *hi /* [M] */,
                          double *z /* [Nz] */);
int nusi_plan_set_source(nusi_plan *plan, int slot, const double *S /* [M] */, const double *w /* [Nz] or NULL */);
/* Evolve n points (their grid fields must equal the plan's).  d_flux /
 * d_flux_fla are DEVICE pointers of n*3*N doubles ([point][k][b]); either may
 * be NULL.  stream is a hipStream_t (NULL = the plan's own stream).  The call
 * is asynchronous w.r.t. the host except for the small host->device copy of
 * the per-point constants; results are ready when the stream is. */
int nusi_plan_evolve(nusi_plan *plan, const nusi_params *pts, int n, double *d_flux, double *d_flux_fla, void *stream);
/* Same with host result buffers; synchronous. */
int nusi_plan_evolve_host(nusi_plan *plan, const nusi_params *pts, int n, double *flux, double *flux_fla);
/* Response matrices (no reference counterpart).  Every flux is linear in the
 * source, and a separable source is S [M] on the source axis and w [Nz]
 * (nusi_plan_set_source).  For point p (every field that enters its Stage-A
 * tables; si, norm and source_model are ignored), redshift weights w (NULL =
 * get_SFR) and source-axis bin n,
 *     G[p][n][k][b]
 * is the mass-basis flux nusi_plan_evolve gives a point whose tabulated slot
 * holds S = e_n (the unit vector) with weights w and norm = 1, and
 * G_fla[p][n][f][b] the same in the flavour basis: n-major arrays
 * [p][n][3][N] of n * M * 3 * N doubles, so that for a spectrum S and norm c
 *     flux = c * sum_n G[n] * S[n].
 * From the cascade's direction, exactly: G[p][0] is all zero (bin 0 is never
 * read) and G[p][n][.][b] = +0.0 for b >= n.
 * nusi_plan_response evolves the n points' response matrices into the DEVICE
 * arrays d_G / d_G_fla (either may be NULL); Stage A is nusi_plan_evolve's
 * (deduplication, batches, every NUSI_OPT_*), and afterwards
 * nusi_plan_tables, nusi_plan_warnings, nusi_plan_stage_ms and
 * nusi_plan_kernels refer to this call.  The cascade is the impulse-source
 * instance of the block-synchronous kernel (k_cascade_bs_impulse: 16 source
 * bins of one table per workgroup), launched in chunks of whole tables under
 * NUSI_OPT_RESPONSE_FIFO_KB; grids it does not fit, and plans set to
 * NUSI_CASCADE_WAVEFRONT / REG / LDS, run the impulses through the scalar
 * k_cascade.  n <= max_points bounds the tables of a call, not tables x M.
 * nusi_plan_set_source and the plan's slots are not involved: a response
 * neither reads nor changes them.  NUSI_EPARAM for a negative or non-finite
 * weight.  nusi_plan_response_host: the same into host arrays, synchronous.
 *
 * nusi_plan_response_apply: Q spectra on ntab resident response matrices,
 *     out[t][q][r] = scale[q] * acc,   acc = 0.0, and for n = 1 .. M-1
 *     ascending  acc = acc + G[t][n][r] * S[q][n]
 * (the product and the sum rounded separately, no fma; rows whose bin b >= n
 * are skipped, which changes no bit of a G as above), r over the 3 N rows of
 * G or of G_fla -- call it once for each array.  d_G [ntab][M][3][N] and
 * d_out [ntab][Q][3][N] are DEVICE pointers; S [Q][M] and scale [Q] (NULL =
 * 1) are host vectors and are copied.  NUSI_EPARAM for a negative or
 * non-finite S (nusi_plan_set_source's rule) or a non-finite scale.  The call
 * is ordered on `stream` (NULL = the plan's own, where a response with
 * stream = NULL ran).  nusi_plan_response_apply_host: host G and out. */
int nusi_plan_response(nusi_plan *plan, const nusi_params *pts, int n, const double *w /* [Nz] or NULL */,
                       double *d_G, double *d_G_fla, void *stream);
int nusi_plan_response_host(nusi_plan *plan, const nusi_params *pts, int n, const double *w, double *G, double *G_fla);
int nusi_plan_response_apply(nusi_plan *plan, const double *d_G, int ntab, const double *S /* [Q][M] */, int Q,
                             const double *scale /* [Q] or NULL */, double *d_out, void *stream);
int nusi_plan_response_apply_host(nusi_plan *plan, const double *G, int ntab, const double *S, int Q,
                                  const double *scale, double *out);
/* Mass-resolved response matrices: the source's flavour composition (no
 * reference counterpart).  Every built-in source and every tabulated one is
 * emitted in equal thirds into the three mass states (nuSIprop.hpp:737; the
 * norm / 3.0 of the source terms).  The flux is linear in the source PER MASS
 * STATE, so the response resolved by the source's mass state j serves any
 * composition.
 *
 * The matrix.  G3[p][j][n][k][b] is the mass-basis flux of state k in bin b
 * that the cascade of point p gives when the source term of (step i, bin b,
 * state k') is
 *     delta_{k' j} * [b + i == n] * sig3[i],
 *     sig3[i] = step_c[i] * (w[i] / (1 + z[i]))  for i >= 1
 * -- tabulated_src(step_c[i], 3.0, w[i], z[i], 1.0), the same bits: the WHOLE
 * unit source goes into state j, with no third.  The solve is the existing
 * one with the source per row,
 *     v_k = (f_k + (s_k + u_k * add)) * rz_k,   s_k = (k == j) ? src : 0.0,
 * and everything after it is unchanged.  G3_fla[p][j][n][f][b] goes through
 * the finalise's |U|^2 expression.
 * Layout: [p][j][n][3][N], n_points * 3 * M * 3 * N doubles, so G3 viewed as
 * (3 n_points, M, 3, N) is a stack of ordinary response matrices, which
 * nusi_plan_response_apply and nusi_plan_response_fold accept as it stands
 * (ntab = 3 n_points).  As for G: column n = 0 is zero, and entries with
 * b >= n are +0.0, sign bit clear.
 * Sign.  The block k = j is non-negative.  For k != j an entry may be
 * NEGATIVE: M = I + offdiag has positive off-diagonals (nuSIprop.hpp:302-303,
 * without the step factor), and where a column's state k != j meets a zero
 * right-hand side -- the column's top bin of a step, b = n - i -- the 3x3 solve
 * gives -m_kj * x_j.  This is the reference's arithmetic on a source the
 * reference never had, and it is not clamped.
 *
 * nusi_plan_response_mass evolves G3 / G3_fla of n points into DEVICE arrays
 * (either may be NULL) like nusi_plan_response: the same Stage A with the same
 * deduplication; nusi_plan_tables / _warnings / _stage_ms / _kernels refer to
 * the call afterwards.  The cascade is k_cascade_mass_impulse (the impulse
 * instance with the source in one row: a workgroup per table, source state
 * and 16 source-axis bins; a FIFO of three times the plain response's per
 * table, launches of whole tables under NUSI_OPT_RESPONSE_FIFO_KB, any budget
 * the same bits); grids it does not fit and plans set to
 * NUSI_CASCADE_WAVEFRONT / REG / LDS run the scalar k_cascade_mass.
 * nusi_response_mass_shape is the call's size check as a pure function
 * (M = N + Nz - 1; *doubles, where not NULL, = n * 3 * M * 3 * N): NUSI_EPARAM
 * when n * 3 * M exceeds 2^31 - 1; the call applies it.  _host: host arrays,
 * synchronous.  nusi_response_mass: the same for an object's point.
 *
 * nusi_plan_response_compose: Qc compositions of ntab triples of rows of any
 * length X (X = M * 3 * N for G3 / G3_fla, X = M * C for a folded R3),
 *     out[t][c][x] = (kappa[t][c][0] * A[t][0][x] + kappa[t][c][1] * A[t][1][x])
 *                    + kappa[t][c][2] * A[t][2][x],
 * products and sums rounded separately, no fma.  d_A [ntab][3][X] and d_out
 * [ntab][Qc][X] are DEVICE pointers; kappa [ntab][Qc][3] is a host array,
 * copied; every entry finite and >= 0 (else NUSI_EPARAM); it need not sum to
 * 1.  With Qc = 1 the result is an ordinary stack of ntab response matrices
 * that every call taking G, G_fla or R takes unchanged.
 *   - +0.0 entries stay +0.0 (a sum of non-negative multiples of +0.0).
 *   - With some kappa_k = 0 the result may carry the negative entries above:
 *     the non-negativity that the fold's bound and the detector calls assume
 *     then holds only up to them.  With every kappa_k > 0 of ordinary size it
 *     holds (the entry's k = j partner outweighs it by ~ 1 / m_kj).
 * The call is ordered on `stream` like nusi_plan_response_apply.
 *
 * nusi_mixing: the |U_fk|^2 of an ordering, U2[3 f + k] (the matrix the
 * finalise and the couplings u_k = U2[3 flav + k] use).
 * nusi_mass_fractions: the share of a source of flavour composition phi =
 * (phi_e, phi_mu, phi_tau) emitted into mass state k,
 *     kappa_k = ((phi_e U2[0][k] + phi_mu U2[1][k]) + phi_tau U2[2][k])
 *               / ((phi_e + phi_mu) + phi_tau);
 * pure functions, no plan and no device.  NUSI_EPARAM for a negative or
 * non-finite phi, or when all phi are zero.  Equal thirds give kappa = 1/3 to
 * rounding, and composing G3 with it gives G to rounding.
 * nusi_plan_step_constants: the grid's step_c [Nz] and step_s [Nz] (either
 * may be NULL; index 0 unused), which a host evaluation of the definition
 * above needs (nusiprop_amd/response.py cascade_host). */
int nusi_mixing(int normal_ordering, double *U2 /* [9] */);
int nusi_mass_fractions(int normal_ordering, const double *phi /* [3] */, double *kappa /* [3] */);
int nusi_response_mass_shape(int N, int Nz, int n, long long *doubles /* or NULL */);
int nusi_plan_step_constants(const nusi_plan *plan, double *step_c /* [Nz] */, double *step_s /* [Nz] */);
int nusi_plan_response_mass(nusi_plan *plan, const nusi_params *pts, int n, const double *w /* [Nz] or NULL */,
                            double *d_G3, double *d_G3_fla, void *stream);
int nusi_plan_response_mass_host(nusi_plan *plan, const nusi_params *pts, int n, const double *w, double *G3,
                                 double *G3_fla);
int nusi_plan_response_compose(nusi_plan *plan, const double *d_A, int ntab, long long X,
                               const double *kappa /* [ntab][Qc][3] */, int Qc, double *d_out, void *stream);
int nusi_plan_response_compose_host(nusi_plan *plan, const double *A, int ntab, long long X, const double *kappa, int Qc,
                                    double *out);
/* The detector of a plan (no reference counterpart): folding fluxes and response matrices into expected event counts
 * per reconstructed-energy bin, on the device.
 * nusi_plan_set_detector registers D [C][3][N] and a background B [C] (NULL = 0): D[c][f][b] is the expected number
 * of events in reconstructed bin c per unit of flux_fla[f][b] as the library returns it -- the bin average dPhi/dE
 * (nuSIprop.hpp:328-336) -- so the true-energy bin width, effective area, exposure and migration are all inside D.
 * Ordering and copying are nusi_plan_set_source's: the call waits for the plan's latest call, copies synchronously
 * (the caller may free its arrays), and later calls see the new detector.  D == NULL (with any C) clears it.
 * NUSI_EPARAM for C outside 1 .. NUSI_DETECTOR_BINS_MAX or a negative or non-finite entry of D or B (everything
 * below relies on every summed term being non-negative); the calls below return NUSI_ESTATE while no detector is set.
 * A call that fails (a refused parameter, no device memory) leaves the plan with the detector it had.  The detector
 * calls of a plan may be issued on different streams: each is ordered after the plan's earlier detector calls,
 * wherever they ran.
 * nusi_plan_detector_bins: C, 0 = none.
 *
 * The fold (k_detector_fold, one batched fp64 GEMM on the matrix cores), r over the 3 N entries of a row:
 *     nusi_plan_response_fold   R[t][n][c] = sum_r G_fla[t][n][r] D[c][r]            (no background)
 *     nusi_plan_fold_flux       mu[p][c]   = sum_r flux_fla[p][r] D[c][r] + B[c]
 * d_G_fla [ntab][M][3][N] is a response matrix of nusi_plan_response (its entries of bins b >= n are +0.0 and are NOT
 * read), d_flux_fla [n][3][N] an ordinary evolve output; d_R [ntab][M][C] and d_mu [n][C] are DEVICE pointers.
 * Unlike the apply, the fold has NO defined summation order -- the matrix core owns it.  The contract is a bound:
 * every term is non-negative, and a sum of K products in any order, fused or not, carries at most K roundings per
 * term, so
 *     |computed - exact| <= gamma_K * exact,   gamma_K = K u / (1 - K u),  u = 2^-53,  K = 3 N
 * (one more rounding for the background), provided no non-zero product is subnormal; where every product is zero
 * the result is +0.0.  A table's or a row tile's result does not depend on the call's other rows.
 *
 * nusi_plan_response_events (k_detector_events): Q spectra on ntab folded matrices, in a defined order:
 *     acc = 0.0, and for n = 1 .. M-1 ascending  acc = acc + R[t][n][c] * S[q][n]
 *     mu[t][q][c] = scale[q] * acc + B[c]
 * (every product and sum rounded separately, no fma), and with data [C]
 *     nll[t][q] = sum over c ascending from 0.0 of term_c,  term_c = mu_c - data_c * log(mu_c),
 *     term_c = mu_c where data_c == 0 (the log is not evaluated)
 * -- the Poisson negative log-likelihood without its data-only constant; +inf where data_c > 0 and mu_c == 0; log is
 * the library's own (nusi_libm.hpp nm::log, the oracle's ora_log).  S [Q][M], scale [Q] (NULL = 1) and data [C] are
 * host vectors and are copied; d_mu [ntab][Q][C] and d_nll [ntab][Q] are DEVICE pointers, either may be NULL but
 * not both, and d_nll needs data.  NUSI_EPARAM for a negative or non-finite S, scale or data.  The calls are
 * ordered on `stream` (NULL = the plan's own).  The _host forms take host arrays and are synchronous. */
#define NUSI_DETECTOR_BINS_MAX 64
int nusi_plan_set_detector(nusi_plan *plan, int C, const double *D /* [C][3][N] */, const double *B /* [C] or NULL */);
int nusi_plan_detector_bins(const nusi_plan *plan);
int nusi_plan_fold_flux(nusi_plan *plan, const double *d_flux_fla /* [n][3][N] */, int n, double *d_mu /* [n][C] */,
                        void *stream);
int nusi_plan_fold_flux_host(nusi_plan *plan, const double *flux_fla, int n, double *mu);
int nusi_plan_response_fold(nusi_plan *plan, const double *d_G_fla /* [ntab][M][3][N] */, int ntab,
                            double *d_R /* [ntab][M][C] */, void *stream);
int nusi_plan_response_fold_host(nusi_plan *plan, const double *G_fla, int ntab, double *R);
int nusi_plan_response_events(nusi_plan *plan, const double *d_R, int ntab, const double *S /* [Q][M] */, int Q,
                              const double *scale /* [Q] or NULL */, const double *data /* [C] or NULL */,
                              double *d_mu /* [ntab][Q][C] or NULL */, double *d_nll /* [ntab][Q] or NULL */, void *stream);
int nusi_plan_response_events_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q, const double *scale,
                                   const double *data, double *mu, double *nll);
/* nusi_plan_response_profile (k_detector_profile): the Poisson statistic of nusi_plan_response_events PROFILED over
 * the flux normalisation -- for every table t and spectrum q the a >= 0 that minimises -ln L(a s + B | data), found
 * by Newton's iteration on the derivative g(a) = sum_c s_c - sum_c data_c s_c / (a s_c + B_c), which is increasing
 * and concave in a, from a start left of the root.  Every step is +, *, / and comparisons on IEEE doubles, each
 * rounded separately (no fma), in a defined order, so ahat, mu and status are defined to the bit:
 *   s_c      the events call's accumulator: acc = 0.0, acc = acc + R[t][n][c] * S[q][n], n = 1 .. M-1 ascending
 *   tree(x)  x over c padded to P = 2^ceil(log2 C) entries with +0.0, then the vector replaced by the sums of its
 *            adjacent pairs (0+1, 2+3, ..) until one value is left
 *   active   bin c with data_c > 0 and s_c > 0; an inactive bin adds exactly 0.0 to S2 and S3 and is never divided
 *   S1 = tree(s); if S1 == 0 or no bin is active: ahat = 0, NUSI_FIT_FLAT, no step
 *   start    a = max(0, max over active c of (data_c / S1 - B_c / s_c))
 *   step     den_c = a s_c + B_c (two roundings), u_c = s_c / den_c, r_c = data_c u_c, h_c = r_c u_c;
 *            S2 = tree(r), S3 = tree(h), g = S1 - S2;  g >= 0: stop (NUSI_FIT_BOUNDARY if a == 0);
 *            a_new = a + (S2 - S1) / S3;  a_new <= a: stop;  else a = a_new
 *   at most NUSI_FIT_ITER_MAX steps, then NUSI_FIT_NOT_CONVERGED with the last a
 *   mu[t][q][c] = ahat s_c + B_c (two roundings) and nll[t][q] the events call's statistic of that mu (+inf, and
 *   NUSI_FIT_INFINITE, where data_c > 0 = mu_c: a bin with data, no signal and no background -- it does not enter
 *   the iteration)
 *   status[t][q] = the number of steps taken (low 8 bits, NUSI_FIT_STEPS_MASK) | the flags
 * provided no non-zero product is subnormal and none overflows.  In exact arithmetic on those doubles
 * |g(ahat)| <= (2 ceil(log2 C) + 18) u (S1 + S2), u = 2^-53, wherever ahat > 0 and the iteration converged
 * (DESIGN.md sec. 4).  S [Q][M] and data [C] are host vectors and are copied (validation, copying and stream ordering
 * as for nusi_plan_response_events; there is no scale: it is what is fitted); d_ahat [ntab][Q], d_nll [ntab][Q],
 * d_mu [ntab][Q][C] (doubles) and d_status [ntab][Q] (ints) are DEVICE pointers, all but d_ahat may be NULL.
 * NUSI_ESTATE without a detector, NUSI_EPARAM for data == NULL, d_ahat == NULL or a negative or non-finite S or
 * data.  The _host form takes host arrays and is synchronous. */
#define NUSI_FIT_ITER_MAX 64
#define NUSI_FIT_STEPS_MASK 0xff
#define NUSI_FIT_FLAT 0x100
#define NUSI_FIT_BOUNDARY 0x200
#define NUSI_FIT_NOT_CONVERGED 0x400
#define NUSI_FIT_INFINITE 0x800
int nusi_plan_response_profile(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab,
                               const double *S /* [Q][M] */, int Q, const double *data /* [C] */,
                               double *d_ahat /* [ntab][Q] */, double *d_nll /* [ntab][Q] or NULL */,
                               double *d_mu /* [ntab][Q][C] or NULL */, int *d_status /* [ntab][Q] or NULL */,
                               void *stream);
int nusi_plan_response_profile_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q, const double *data,
                                    double *ahat, double *nll, double *mu, int *status);
/* Floating background templates (k_detector_fit): the statistic minimised over the signal's scale AND the
 * normalisations of K <= NUSI_FIT_TEMPLATES_MAX background templates T_j [C] >= 0 of the plan's detector, each under an
 * optional Gaussian prior (mean m_j >= 0, width sigma_j > 0; sigma_j = +inf, or prior_sigma == NULL, = none):
 *     mu_c(theta) = theta_0 s_c + sum_j theta_j T_j[c] + B_c,   theta >= 0,   j = 1 .. K
 *     f(theta)    = sum_c (mu_c - data_c log mu_c) + sum_j w_j (theta_j - m_j)^2 / 2,   w_j = 1 / (sigma_j sigma_j)
 * B stays the fixed part; the signal has no prior (w_0 = m_0 = 0 below; m_j = 0 where w_j = 0).
 * nusi_plan_set_templates copies T [K][C] and the priors (ordering and copying as nusi_plan_set_detector).  It needs
 * a detector (NUSI_ESTATE); K = 0 or T == NULL clears the templates; NUSI_EPARAM for K outside 0 ..
 * NUSI_FIT_TEMPLATES_MAX, a negative or non-finite entry of T or prior_mean, a template of zeros, sigma <= 0 or NaN.
 * Setting a detector (or clearing it) clears the templates.  nusi_plan_templates: K, 0 = none.
 *
 * nusi_plan_response_fit: theta_hat = argmin f for every table t and spectrum q, by a damped Newton iteration on the
 * bound-constrained convex problem.  Every operation is +, -, *, / or a comparison on IEEE doubles, each rounded
 * separately (no fma), in a defined order, so theta, mu and status are defined to the bit (detector.fit_host is the
 * same text in numpy); only nll passes through the log.  With X_0 = s (the profile's accumulator), X_j = T_j, n = 1 + K,
 * tree() the profile's sum over the bins, kappa = 2 (ceil(log2 C) + K) + 18 and u = 2^-53:
 *   S1_j = tree(X_j).  Component j is live when S1_j > 0 -- and, for the signal, some bin has data_c > 0 and s_c > 0;
 *            a signal that is not live keeps theta_0 = 0 (NUSI_FIT_FLAT) and the fit goes on over the templates
 *   active   bin c with data_c > 0 and (B_c > 0 or X_jc > 0 for a live j); inactive bins add exactly 0.0 to every sum
 *            below and are never divided.  dmin = min(1, the smallest active datum)
 *   start    theta_j = tree(data over the active bins) / (n_live * S1_j) for the live j, 0 for the others
 *   eval(x)  den_c = x_0 X_0c, den_c = den_c + x_j X_jc (j ascending), den_c = den_c + B_c;  bad = an active den_c is
 *            not > 0;  w_c = data_c / den_c, r_c = w_c / den_c;  S2_j = tree(X_jc w_c),
 *            H_jk = tree((X_jc r_c) X_kc) + (j == k ? w_j : 0) for j <= k,  g_j = (S1_j - S2_j) + w_j (x_j - m_j)
 *   The iteration holds theta, a direction p and a step length t.  First eval(start): bad = stop with
 *   NUSI_FIT_NOT_CONVERGED, else it is theta.  Then, with g, H and S2 of theta's eval:
 *   free     the live j with theta_j > 0 or g_j < 0
 *   stop     when every free j has |g_j| <= kappa u scale_j,  scale_j = (S1_j + S2_j) + w_j (theta_j + m_j)
 *   caps     the step before changed no theta_j, or NUSI_FIT_ITER_MAX steps are taken: NUSI_FIT_NOT_CONVERGED, stop
 *   solve    F = free.  p = -H^-1 g on F (the other j: p_j = 0) by L D L^T in ascending order:
 *            c_ij = H_ij - sum_{k<j} c_ik L_jk, L_ij = c_ij / D_j, D_i = H_ii - sum_{k<i} c_ik L_ik; y_i = -g_i -
 *            sum_{k<i} L_ik y_k; p_i = y_i / D_i - sum_{k>i} L_ki p_k (i descending; every sum subtracts k ascending).
 *            A j in F with theta_j == 0 and p_j < 0 leaves F (all such at once) and the solve is repeated.
 *            A D_i not > 0, or acc = sum_{j in F} g_j p_j (from 0.0, ascending) not < 0: NUSI_FIT_SINGULAR, stop
 *   length   ratio_j = theta_j / -p_j for the j in F with p_j < 0;  t = min(1, the ratios);  clipped = t < 1;
 *            quad = not clipped and -acc <= dmin / 16;  the candidate is x_j = theta_j + t p_j, and exactly 0 for
 *            the j whose ratio_j == t when clipped
 *   trial    eval(x);  slope = sum_j p_j g_j(x) (from 0.0, ascending).  The candidate is accepted when it is not bad
 *            and (quad or slope is not > 0): theta = x, one step counted, and on with `free`.  Otherwise t = t / 2,
 *            x_j = theta_j + t p_j and the trial is repeated; after NUSI_FIT_TRIALS_MAX halvings of one step:
 *            NUSI_FIT_NOT_CONVERGED, stop with theta
 *   mu[t][q][c] = den_c(theta_hat); nll[t][q] = the events call's statistic of that mu, then for j = 1 .. K ascending
 *   with w_j > 0: nll = nll + ((0.5 w_j) (theta_j - m_j)) (theta_j - m_j)
 *   status[t][q] = the steps taken (low 8 bits) | NUSI_FIT_FLAT | NUSI_FIT_BOUNDARY (a live signal with theta_0 == 0)
 *            | NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR | NUSI_FIT_INFINITE (data_c > 0 = mu_c, nll = +inf; such a bin
 *            is inactive) | NUSI_FIT_ZERO << j for every component j with theta_j == 0 | the halvings of all steps,
 *            saturating at NUSI_FIT_TRIALS_MASK, << NUSI_FIT_TRIALS_SHIFT
 * provided no non-zero product is subnormal and none overflows.  f / dmin is self-concordant, so the halving ends and
 * the iteration converges; where it stopped by `stop`, in exact arithmetic on those doubles
 * |g_j(theta_hat)| <= (kappa + ceil(log2 C) + 2 K + 9) u scale_j for the free j, and g_j >= -that for the others.
 * S, data and the outputs are as for nusi_plan_response_profile; d_theta [ntab][Q][1 + K] must not be NULL.
 * NUSI_ESTATE without a detector or without templates (that case is nusi_plan_response_profile). */
enum {   /* (the fit's own constants; the status word's NUSI_FIT_* macros above are shared with the profile;
            NUSI_FIT_SIGNALS_MAX: the signal components of nusi_plan_response_fit_components) */
    NUSI_FIT_TEMPLATES_MAX = 3,
    NUSI_FIT_SIGNALS_MAX = 3,
    NUSI_FIT_TRIALS_MAX = 64,
    NUSI_FIT_SINGULAR = 0x1000,
    NUSI_FIT_ZERO = 0x10000,
    NUSI_FIT_TRIALS_SHIFT = 24,
    NUSI_FIT_TRIALS_MASK = 0x7f
};
int nusi_plan_set_templates(nusi_plan *plan, int K, const double *T /* [K][C] */, const double *prior_mean /* [K] or NULL */,
                            const double *prior_sigma /* [K] or NULL */);
int nusi_plan_templates(const nusi_plan *plan);
int nusi_plan_response_fit(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab, const double *S /* [Q][M] */,
                           int Q, const double *data /* [C] */, double *d_theta /* [ntab][Q][1 + K] */,
                           double *d_nll /* [ntab][Q] or NULL */, double *d_mu /* [ntab][Q][C] or NULL */,
                           int *d_status /* [ntab][Q] or NULL */, void *stream);
int nusi_plan_response_fit_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q, const double *data,
                                double *theta, double *nll, double *mu, int *status);
/* nusi_plan_response_fit_components (k_components_fit): the fit with J = 2 .. NUSI_FIT_SIGNALS_MAX SIGNAL COMPONENTS per
 * table and spectrum, each a stack of rows of its own, floating together with the plan's K = 0 .. NUSI_FIT_TEMPLATES_MAX
 * templates, every normalisation >= 0:
 *     mu_c(theta) = sum_{j<J} theta_j s_jc + sum_{i=1..K} theta_{J+i-1} T_i[c] + B_c,   theta >= 0
 * d_R3 [ntab][J][M][C] is any stack of folded matrices, entries >= 0: the folded rows of nusi_plan_response_mass, or those
 * rows composed (nusi_plan_response_compose) onto the three pure source flavours -- then theta_j >= 0 is exactly the
 * physical flavour triangle and theta_j / sum_j theta_j the fitted composition.  It is nusi_plan_response_fit's iteration,
 * every operation and its order as defined there, with these differences and nothing else:
 *   X_j      = s_j for j < J,  s_j[c] = sum_{n=1}^{M-1} R3[t][j][n][c] S[q][n] ascending in n from 0.0 (the events call's
 *            accumulator on the rows R3[.][j]);  X_{J+i-1} = T_i for i = 1 .. K;  n = J + K.  den adds the products
 *            x_j X_jc in ascending j, then B_c
 *   live     a signal component j < J is live when S1_j > 0 and some bin has data_c > 0 and s_jc > 0; a template is live
 *            when S1_j > 0.  The start gives every live component an equal share, n_live counting both kinds
 *   priors   w_j = m_j = 0 for j < J; template i's prior is component J + i - 1's
 *   kappa    = 2 (ceil(log2 C) + J - 1 + K) + 18: den has J - 1 more products than the fit's; where it
 *            stopped by `stop`, in exact arithmetic |g_j(theta_hat)| <= (3 ceil(log2 C) + 4 (J - 1 + K) + 27) u scale_j
 *            for the free j, and g_j >= -that for the others
 *   status   the fit's word with NUSI_FIT_FLAT when NO signal component is live (the templates are fitted all the same),
 *            NUSI_FIT_BOUNDARY when some signal component is live and every signal theta_j ends at 0, and
 *            NUSI_FIT_ZERO << j for every j < J + K with theta_j == 0: bits 16 .. 21, below NUSI_FIT_TRIALS_SHIFT
 *   mu, nll  as there: mu = den(theta_hat), nll the statistic of that mu, then the penalties of the templates with
 *            w > 0, ascending
 * (detector.fit_components_host is the same text in numpy; with J = 1 and K >= 1 that host form is detector.fit_host to
 * the bit).  Two components whose rows are proportional on the bins with data, or more live components than bins with
 * data, leave the Newton system singular: NUSI_FIT_SINGULAR, as for the fit.
 * nusi_fit_components_shape is the size check the call applies (pure: no plan, no device): NUSI_EPARAM for J outside
 * 2 .. NUSI_FIT_SIGNALS_MAX (J = 1 is nusi_plan_response_fit / _profile), K outside 0 .. NUSI_FIT_TEMPLATES_MAX, C outside
 * 1 .. NUSI_DETECTOR_BINS_MAX, ntab < 1, Q outside 1 .. 2^19, or ntab Q, or the element count of any output (theta
 * [J + K] or mu [C] a record), at or beyond 2^31; *records (unless NULL) = ntab Q.
 * The call: K is nusi_plan_templates, and 0 is allowed.  S, data and the outputs are as for nusi_plan_response_fit;
 * d_theta [ntab][Q][J + K] must not be NULL.  NUSI_ESTATE without a detector; NUSI_EPARAM as the shape check says, for
 * NULL d_R3, S, data or d_theta, and for a negative or non-finite entry of data or S. */
int nusi_fit_components_shape(int C, int J, int K, int ntab, int Q, long long *records /* or NULL */);
int nusi_plan_response_fit_components(nusi_plan *plan, const double *d_R3 /* [ntab][J][M][C] */, int ntab, int J,
                                      const double *S /* [Q][M] */, int Q, const double *data /* [C] */,
                                      double *d_theta /* [ntab][Q][J + K] */, double *d_nll /* [ntab][Q] or NULL */,
                                      double *d_mu /* [ntab][Q][C] or NULL */, int *d_status /* [ntab][Q] or NULL */,
                                      void *stream);
int nusi_plan_response_fit_components_host(nusi_plan *plan, const double *R3, int ntab, int J, const double *S, int Q,
                                           const double *data, double *theta, double *nll, double *mu, int *status);
/* nusi_plan_response_fit_fixed (k_conditional_fit): the CONDITIONAL fit -- the fit above with the signal's scale HELD at
 * a given a = scale[q] >= 0 and only the K templates floating: theta_1 .. theta_K >= 0 minimising f(a, .) for every table
 * t and spectrum q.  At a = 0 it is the background-only fit; at any a it is the inner problem of the statistic
 * q(a) = 2 (min_theta f(a, theta) - min f).  It is nusi_plan_response_fit's iteration on the components j = 1 .. K alone,
 * every operation and its order as defined there, with these differences and nothing else (X_0 = s, X_j = T_j, tree(),
 * u and the priors as there):
 *   S1_j     = tree(X_j) for j = 1 .. K only; component j is live when S1_j > 0.  The signal is not a component: it is
 *            neither live nor free, has no gradient, no row of H and no direction
 *   active   bin c with data_c > 0 and (B_c > 0, or X_jc > 0 for a live j >= 1, or (a > 0 and s_c > 0)): the held signal
 *            supports a bin.  dmin as there
 *   start    theta_j = tree(data over the active bins) / (n_live * S1_j) for the live j >= 1, n_live counting them; 0 for
 *            the others
 *   eval(x)  den_c = a X_0c, den_c = den_c + x_j X_jc (j = 1 .. K ascending), den_c = den_c + B_c -- the fit's den at
 *            x_0 = a, so the conditional mu at some theta has the bits the fit's mu has at (a, theta); bad, w_c, r_c as
 *            there;  S2_j, H_jk and g_j for j, k = 1 .. K only
 *   free, stop, caps, solve, length, trial: as there over j = 1 .. K (slope and acc sum over j = 1 .. K ascending), with
 *            the same kappa = 2 (ceil(log2 C) + K) + 18: den has as many terms as the fit's, so the computed gradient
 *            carries the same roundings, and the floor sum_k H_jk theta_k <= scale_j holds for any subset of components
 *            
 *   theta[t][q][0] = a, copied; theta[t][q][j] = theta_j.  mu = den(theta_hat); nll as there (the statistic of mu, then
 *            the penalties j = 1 .. K ascending)
 *   status[t][q] = the steps taken (low 8 bits) | NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR | NUSI_FIT_INFINITE |
 *            NUSI_FIT_ZERO << j for every j >= 1 with theta_j == 0 | the halvings as there.  Component 0 never sets
 *            NUSI_FIT_ZERO (a = 0 is an input, not an outcome); NUSI_FIT_FLAT and NUSI_FIT_BOUNDARY do not apply and are
 *            never set
 * (detector.fit_fixed_host is the same text in numpy).  Where it stopped by `stop` the fit's bound on the exact
 * gradient holds for j >= 1 with the fit's constant.  scale [Q] is a host vector and is copied, like S and data; the
 * outputs are as for nusi_plan_response_fit.  NUSI_ESTATE without a detector or without templates (that case is
 * nusi_plan_response_events: nothing floats); NUSI_EPARAM as for the fit, and for scale == NULL or a scale that is
 * negative or not finite. */
int nusi_plan_response_fit_fixed(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab,
                                 const double *S /* [Q][M] */, int Q, const double *scale /* [Q] */,
                                 const double *data /* [C] */, double *d_theta /* [ntab][Q][1 + K] */,
                                 double *d_nll /* [ntab][Q] or NULL */, double *d_mu /* [ntab][Q][C] or NULL */,
                                 int *d_status /* [ntab][Q] or NULL */, void *stream);
int nusi_plan_response_fit_fixed_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q,
                                      const double *scale, const double *data, double *theta, double *nll, double *mu,
                                      int *status);
/* nusi_plan_response_limit (k_interval): profile-likelihood limits on the signal's scale.  With
 *     lambda(a) = min_theta f(a, theta) - min f      (q(a) = 2 lambda(a))
 * it returns, for every table t and spectrum q, the best fit and the roots a_lo < theta_hat_0 < a_hi of
 * lambda(a) = delta / 2 -- delta = 2.706 for a one-sided 95 % limit, 1 for a 68 % interval -- on the sides `which` asks
 * for (NUSI_LIMIT_LOWER | NUSI_LIMIT_UPPER).  lambda is convex in a (a partial minimum of a convex f), so Newton's iteration
 * in a converges monotonically from the side where lambda > delta / 2 and reaches that side in one step from the other;
 * its derivative is g_0 = S1_0 - S2_0 at the conditional optimum (the envelope theorem).  K = nusi_plan_templates(plan)
 * may be 0.  Every operation but the log is +, -, *, /, a comparison, frexp or ldexp on IEEE doubles, each rounded
 * separately, in a defined order (detector.limit_host is the same text in numpy); the log decides only through
 * lambda's last bits.  With X, tree(), u, the priors and kappa as for nusi_plan_response_fit, hd = 0.5 delta:
 *   best fit  the record of nusi_plan_response_fit (K = 0: of nusi_plan_response_profile, theta_hat = (ahat)), the same
 *            operations in the same order: theta_hat, nll_hat, status[t][q][0] and mu_hat = its mu have those calls' bits
 *   no fit   status[0] has NUSI_FIT_NOT_CONVERGED or NUSI_FIT_SINGULAR: both limits NaN, NUSI_LIMIT_NO_FIT, no step
 *   no signal  S1_0 = tree(s) == 0: a_hi = +inf (NUSI_LIMIT_UNBOUNDED), a_lo = 0 (NUSI_LIMIT_UNBOUNDED | _AT_ZERO), no step
 *   lact     bin c with data_c > 0 and mu_hat_c > 0 (a bin of NUSI_FIT_INFINITE is not: its mu is 0 at every a)
 *   step0    w_c = data_c / mu_hat_c, r_c = w_c / mu_hat_c on lact bins, 0 elsewhere; S3 = tree((s_c r_c) s_c);
 *            S3 > 0: step0 = 2^ceil(e / 2), delta / S3 = f 2^e with f in [1/2, 1) (frexp) -- the quadratic model's
 *            distance sqrt(delta / S3) rounded up to a power of two;  else step0 = hd / S1_0
 *   start    upper: a = theta_hat_0 + step0.  lower: theta_hat_0 == 0: a_lo = 0, NUSI_LIMIT_AT_ZERO, no step; else
 *            a = theta_hat_0 - step0, and 0.5 theta_hat_0 if that is not > 0.  theta = (theta_hat_1 .. theta_hat_K)
 *   zero_ok  no bin has data_c > 0, s_c > 0, B_c == 0 and no live template with T_jc > 0: such a bin's only support
 *            is the signal, lambda(0) = +inf, and the lower search never evaluates a = 0
 *   An outer step at a:
 *   inner    the iteration of nusi_plan_response_fit_fixed at the held a, every rule of its text, started from theta
 *            instead of its `start`; if that first eval is bad, from its `start` after all.  Each eval also forms
 *            S2_0 = tree(s_c w_c), the last of the round's sums.  NUSI_FIT_NOT_CONVERGED or _SINGULAR of it:
 *            NUSI_LIMIT_NOT_CONVERGED, stop.  Else theta = its result, one outer step counted, its Newton steps added
 *            to the side's inner count; S2_0 is that of the last accepted eval.  K = 0: the one eval, no step
 *   lambda   mu_c = den_c(a, theta) in the fit's order; dmu_c = mu_c - mu_hat_c; on lact bins ratio_c = mu_c /
 *            mu_hat_c, l_c = log(ratio_c) (-inf where ratio_c is not > 0), p_c = data_c l_c, term_c = dmu_c - p_c,
 *            mag_c = |dmu_c| + |p_c|; elsewhere term_c = dmu_c, mag_c = |dmu_c|;  lam = tree(term), mag = tree(mag);
 *            then for j = 1 .. K ascending with w_j > 0: d_j = theta_j - theta_hat_j, s_j = (theta_j - m_j) +
 *            (theta_hat_j - m_j), pd_j = ((0.5 w_j) d_j) s_j, lam = lam + pd_j, mag = mag + |pd_j|
 *   h = lam - hd;  eps = (kappa_lambda u) (mag + hd), kappa_lambda = 2 (ceil(log2 C) + K) + 14;  g_0 = S1_0 - S2_0
 *   at zero  (lower, a == 0)  h not > 0: a_lo = 0, NUSI_LIMIT_AT_ZERO, stop; else, unless the cap is reached, zero is
 *            done, seen = false, a = 0.5 a_prev and on with the next outer step (no Newton step from zero: lambda is
 *            log-steep there)
 *   stop     |h| <= eps, or seen and h not > 0 (the monotone phase has met the noise of h): stop, converged
 *   seen = h > 0
 *   caps     NUSI_LIMIT_ITER_MAX outer steps taken, or g_0 not > 0 (upper; not < 0, lower): NUSI_LIMIT_NOT_CONVERGED, stop
 *   step     a_new = a - h / g_0.  lower and a_new not > 0: seen = false, and a_new = 0 with a_prev = a if zero_ok and
 *            zero is not done, else a_new = 0.5 a.  a_new not < +inf: NUSI_LIMIT_NOT_CONVERGED, stop.  a_new == a: stop,
 *            converged.  Else a = a_new
 *   The side's result is the last a.  Its word status[t][q][1] (lower), [2] (upper) = the outer steps (low 8 bits,
 *   NUSI_LIMIT_STEPS_MASK) | the NUSI_LIMIT_* flags | the inner count, saturating at NUSI_LIMIT_INNER_MASK, <<
 *   NUSI_LIMIT_INNER_SHIFT.  A side not asked for: NaN and a word of 0, and its pointer may be NULL.
 * S, data and the ordering as for nusi_plan_response_fit; d_lo, d_hi, d_nll_hat [ntab][Q], d_theta_hat [ntab][Q][1 + K]
 * (doubles) and d_status [ntab][Q][3] (ints) are DEVICE pointers; any may be NULL but the result of a side asked for.
 * NUSI_ESTATE without a detector; NUSI_EPARAM as for the fit, and for a delta that is not finite or not > 0, `which`
 * outside 1 .. 3, or a NULL result of a side asked for.  The _host form takes host arrays and is synchronous. */
#define NUSI_LIMIT_LOWER 1
#define NUSI_LIMIT_UPPER 2
#define NUSI_LIMIT_ITER_MAX 64
#define NUSI_LIMIT_STEPS_MASK 0xff
#define NUSI_LIMIT_AT_ZERO 0x100
#define NUSI_LIMIT_UNBOUNDED 0x200
#define NUSI_LIMIT_NO_FIT 0x400
#define NUSI_LIMIT_NOT_CONVERGED 0x800
#define NUSI_LIMIT_INNER_SHIFT 16
#define NUSI_LIMIT_INNER_MASK 0x7fff
int nusi_plan_response_limit(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab, const double *S /* [Q][M] */,
                             int Q, const double *data /* [C] */, double delta, int which,
                             double *d_lo /* [ntab][Q] */, double *d_hi /* [ntab][Q] */,
                             double *d_theta_hat /* [ntab][Q][1 + K] or NULL */, double *d_nll_hat /* [ntab][Q] or NULL */,
                             int *d_status /* [ntab][Q][3] or NULL */, void *stream);
int nusi_plan_response_limit_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q, const double *data,
                                  double delta, int which, double *lo, double *hi, double *theta_hat, double *nll_hat,
                                  int *status);
/* nusi_plan_response_ensemble (k_ensemble_profile, k_ensemble_fit, k_ensemble_best): P data sets data[p][C] -- an
 * ensemble of pseudo-experiments -- against every table and spectrum in ONE call, and of each (p, t) only the BEST
 * spectrum's record.  The front half s[t][q][c] = sum_n R[t][n][c] S[q][n] does not depend on the data: it is computed
 * once and the P fits run on it.
 *
 * The selection rule.  For a data set p and a table t, the record of spectrum q is exactly what
 * nusi_plan_response_fit gives for (t, q) against data[p] -- theta [1 + K], status, nll -- or, on a plan without
 * templates (K = nusi_plan_templates(plan) = 0), what nusi_plan_response_profile gives: ahat (theta has width 1), status,
 * nll.  The same iteration, the same operations in the same order: the bits of those calls.  The best record is the
 * minimum under the key
 *     (isnan(nll), nll, q)   compared lexicographically, nll as numbers:
 * a NaN loses to everything, +inf included; equal nll resolve to the lowest q.  The key is a total order on the
 * spectra, so the result does not depend on how the reduction is arranged (NUSI_OPT_ENSEMBLE_QSLICES, _PSLICES:
 * the same bits for every value).  If every nll is +inf (NUSI_FIT_INFINITE) the record is that of q = 0.
 *
 * d_q[p][t] = that q, d_nll[p][t], d_theta[p][t][1 + K], d_status[p][t]: device memory; d_theta and d_status may be
 * NULL.  S [Q][M] and data [P][C] are host arrays and are copied (entries finite and >= 0); the device generates no
 * random numbers, pseudo-data are the caller's.  Asynchronous and ordered with the plan's other detector calls like
 * nusi_plan_response_fit.  NUSI_ESTATE without a detector; NUSI_EPARAM for a NULL d_R, S, data, d_q or d_nll, P outside
 * 1 .. NUSI_ENSEMBLE_DATASETS_MAX, ntab < 1, Q outside 1 .. 2^19, P ntab >= 2^31, or a negative or non-finite entry of
 * S or data; a refused call changes nothing.  _host: R and the outputs in host memory, synchronous. */
#define NUSI_ENSEMBLE_DATASETS_MAX 65536
int nusi_plan_response_ensemble(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab,
                                const double *S /* [Q][M] */, int Q, const double *data /* [P][C] */, int P,
                                int *d_q /* [P][ntab] */, double *d_nll /* [P][ntab] */,
                                double *d_theta /* [P][ntab][1 + K] or NULL */, int *d_status /* [P][ntab] or NULL */,
                                void *stream);
int nusi_plan_response_ensemble_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q,
                                     const double *data, int P, int *q, double *nll, double *theta, int *status);
/* nusi_plan_response_ensemble_limit (k_toys_limit, k_toys_band): the limits of nusi_plan_response_limit for P data sets
 * data[p][C] -- an ensemble of pseudo-experiments -- in ONE call, and of each (table, spectrum) the order statistics of
 * its P limits: the median expected limit and its bands, when the toys are background-only.  The front half
 * s[t][q][c] = sum_n R[t][n][c] S[q][n] does not depend on the data: it is computed once and the P searches run on it.
 * K = nusi_plan_templates(plan) = 0 .. 3.
 *
 * The record of (p, t, q) is exactly what nusi_plan_response_limit gives for table t and spectrum q against data[p]
 * with the same delta and `which`: lo, hi and the two side words (that call's status[t][q][1] and [2]).  The same
 * operations in the same order, the device log included: that call's bits.  It depends on no other table, spectrum or
 * data set of the call.
 *
 * The band.  Per side asked for and per (t, q): the order statistics of the P limits under the key
 *     (isnan(x), x)   ascending, x compared as a number:
 * band[t][q][k] is the value v that has at most rank[k] entries before it under the key and more than rank[k] entries
 * before or equal to it -- entry rank[k] of the sorted limits.  NaN (NUSI_LIMIT_NO_FIT) sorts after everything, +inf
 * (NUSI_LIMIT_UNBOUNDED) included.  A side's limits are never -0.0, so equal keys are equal bits and the result does
 * not depend on how the selection is arranged.  A NUSI_LIMIT_NOT_CONVERGED record enters with its last a, as a number;
 * the tally says how many there are.  rank [NR] are host ints, 0 <= rank[k] < P, duplicates allowed, NR = 0 ..
 * NUSI_BAND_RANKS_MAX; P = 1 .. NUSI_BAND_DATASETS_MAX.
 *
 * The tally.  tally[t][q][side][4] (ints; side 0 = lower, 1 = upper) counts the toys whose side word carries
 * NUSI_LIMIT_AT_ZERO, _UNBOUNDED, _NO_FIT and _NOT_CONVERGED, in that order.
 *
 * Outputs, all DEVICE pointers: d_band_lo, d_band_hi [ntab][Q][NR] (doubles), d_tally [ntab][Q][2][4] (ints), and the
 * raw records d_lo_all, d_hi_all [ntab][Q][P] (doubles) and d_words_all [ntab][Q][P][2] (ints; [..][0] the lower side's
 * word, [1] the upper's), the toy index fastest: the layout the selection reads.  Any may be NULL, except that NR > 0
 * needs the band of every side asked for.  A side not asked for: NaN bands and raw limits where a pointer is given, a
 * tally of 0 and raw words of 0.  The best fits are not returned per toy: nusi_plan_response_ensemble has them.
 *
 * Scratch and the grid.  Where a side's raw array is not given and NR > 0, its P limits per spectrum live in scratch
 * owned by the plan, at most NUSI_OPT_ENSEMBLE_LIMIT_MB (below).  The work is cut into units of one table and one
 * block of QB = 256 >> ceil(log2 C) spectra; a unit takes QB P 8 bytes of scratch per side kept there, and the call runs
 * in chunks of as many units as fit, each chunk a launch of k_toys_limit and one of k_toys_band on the call's stream.  A
 * budget below one unit is refused.  Whatever the budget, and also with the raw arrays given, a chunk holds at most
 * 2^22 spectra, so that no launch exceeds the grid a device accepts.  Inside a chunk the data sets are split into p-slices (the grid's z): automatic --
 * as many as fill the card, of at least 16 data sets each --, or NUSI_OPT_ENSEMBLE_PSLICES > 0: min(that, P); a
 * p-slice repeats the front half, writes its own section of [P] and adds its tallies (integer adds commute).
 * NUSI_OPT_ENSEMBLE_QSLICES does not apply.  Every budget and every slicing give the same bits.
 *
 * S [Q][M], data [P][C] and rank are host arrays and are copied.  Asynchronous and ordered with the plan's other
 * detector calls like nusi_plan_response_fit.  NUSI_ESTATE without a detector; NUSI_EPARAM for a NULL d_R, S or data,
 * a NULL rank with NR > 0, P, NR or a rank out of range, ntab < 1, Q outside 1 .. 2^19, a delta that is not finite or
 * not > 0, `which` outside 1 .. 3, a negative or non-finite entry of S or data, NR > 0 without the band of a side asked
 * for, NR = 0 with no tally and no raw output (nothing to do), or a budget too small for one unit; a refused call
 * changes nothing.  _host: R and the outputs in host memory, synchronous. */
#define NUSI_BAND_RANKS_MAX 16
#define NUSI_BAND_DATASETS_MAX 4096
int nusi_plan_response_ensemble_limit(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab,
                                      const double *S /* [Q][M] */, int Q, const double *data /* [P][C] */, int P,
                                      double delta, int which, const int *rank /* [NR] */, int NR,
                                      double *d_band_lo /* [ntab][Q][NR] */, double *d_band_hi /* [ntab][Q][NR] */,
                                      int *d_tally /* [ntab][Q][2][4] or NULL */, double *d_lo_all /* [ntab][Q][P] or NULL */,
                                      double *d_hi_all /* [ntab][Q][P] or NULL */,
                                      int *d_words_all /* [ntab][Q][P][2] or NULL */, void *stream);
int nusi_plan_response_ensemble_limit_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q,
                                           const double *data, int P, double delta, int which, const int *rank, int NR,
                                           double *band_lo, double *band_hi, int *tally, double *lo_all, double *hi_all,
                                           int *words_all);
/* Drawing counts (k_poisson_draw; nusi_draw.hpp, detector.draw_host): Poisson pseudo-experiments from a counter-based
 * generator on the device, every operation defined, so that a host form with the same exp and log gives the same bits.
 *
 * Random bits.  Philox4x32-10 with the multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57 and the key increments 0x9E3779B9,
 * 0xBB67AE85: ten rounds of
 *     c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)),   then k0 += 0x9E3779B9, k1 += 0xBB67AE85
 * (hi, lo: the words of the 64-bit product).  The key (k0, k1) is the call's 64-bit seed, low word first; the counter is
 * (block, p 64 + c, row, stream): p the toy, c the bin, row and stream the caller's, block = 0, 1, .. the 128-bit blocks
 * one draw consumes.  A draw's identity is global: no result depends on a chunk, a slice or the launch.  A block x gives
 * two uniforms in [0, 1):  U0 = ((x0 >> 5) 2^26 + (x1 >> 6)) 2^-53,  U1 the same from x2 and x3.
 *
 * Poisson(mu), the count k a double; every operation rounded on its own (no fma), exp and log the library's (nm::exp_i,
 * nm::log_i; the oracle's ora_exp, ora_log).
 *   mu == 0: 0, no bits are drawn.  mu negative, NaN or infinite: NaN (the calls refuse such a mu where it is an input).
 *   0 < mu < 10, inversion on U0 of block 0:
 *     p = exp(-mu); F = p; k = 0;
 *     while (!(u < F)) { k += 1; p = (p mu) / k; Fn = F + p; if ((Fn == F && k > mu) || k == 255) break; F = Fn; }
 *   mu >= 10, Hoermann's PTRS (numpy's constants): slam = sqrt(mu), loglam = log(mu), b = 0.931 + 2.53 slam,
 *     a = -0.059 + 0.02483 b, invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2).  Round r = 0, 1, ..
 *     uses block r: U = U0 - 0.5, V = U1, us = 0.5 - |U|; us == 0 rejects (k stays);
 *     k = floor(((((2 a) / us + b) U) + mu) + 0.43);  accept if us >= 0.07 && V <= vr;  reject if k < 0 || (us < 0.013
 *     && V > us);  else accept if
 *         (log(V) + log(invalpha)) - log(a / (us us) + b)  <=  (-mu + k loglam) - loggam(k + 1),    log(0) = -inf.
 *     After 64 rejected rounds the draw is max(k, 0) of the last round that formed a k (0 if none did).
 *   loggam(x) is numpy's random_loggam: 0 at x == 1 and x == 2; n = x < 7 ? (int)(7 - x) : 0, x0 = x + n,
 *     x2 = (1 / x0) (1 / x0); gl0 = a9, then for k = 8 .. 0: gl0 = gl0 x2 + a_k (two roundings), a_k = 8.333333333333333e-02,
 *     -2.777777777777778e-03, 7.936507936507937e-04, -5.952380952380952e-04, 8.417508417508418e-04, -1.917526917526918e-03,
 *     6.410256410256410e-03, -2.955065359477124e-02, 1.796443723688307e-01, -1.39243221690590e+00;
 *     gl = ((gl0 / x0 + 0.5 * 1.8378770664093453) + (x0 - 0.5) log(x0)) - x0;  then n times: x0 -= 1, gl -= log(x0).
 *
 * nusi_plan_draw_counts: d_out[row][p][c] = the draw of mu[row][c] with the identity (seed, stream, row, p, c), for
 * p < P: rows P C doubles in device memory.  mu [rows][C] is a host array and is copied (entries finite and >= 0).  The
 * plan's detector is not needed: C = 1 .. NUSI_DETECTOR_BINS_MAX is an argument.  Asynchronous on `stream` (NULL: the
 * plan's); the plan keeps mu's copy until the next draw, which waits for this one.  NUSI_EPARAM for a NULL mu or d_out,
 * rows < 1, C out of range, P outside 1 .. NUSI_DRAW_DATASETS_MAX (the counter holds p 64 + c), rows P C above
 * NUSI_DRAW_COUNTS_MAX = (2^31 - 1) 256 (one launch of 256 counts a block), or a negative or non-finite mu; a refused
 * call changes nothing.  _host: the output in host memory, synchronous. */
#define NUSI_DRAW_DATASETS_MAX 67108864
#define NUSI_DRAW_COUNTS_MAX 549755813632
int nusi_plan_draw_counts(nusi_plan *plan, const double *mu /* [rows][C] */, int rows, int C, int P,
                          unsigned long long seed, unsigned stream_id, double *d_out /* [rows][P][C] */, void *stream);
int nusi_plan_draw_counts_host(nusi_plan *plan, const double *mu, int rows, int C, int P, unsigned long long seed,
                               unsigned stream_id, double *out);
/* Drawing normals (k_normal_draw; nusi_draw.hpp draw::normal0, detector.draw_normal_host): a normal variate around
 * center >= 0 of width sigma, truncated to x >= 0, on the same Philox blocks -- the auxiliary measurements and the
 * nuisance parameters of the toys (NUSI_OPT_TOY_NUISANCE, below).  Marsaglia's polar method; every operation rounded on its
 * own (no fma), log the library's (nm::log_i; the oracle's ora_log), sqrt IEEE's.
 *   Identity.  (seed, stream, row, p, j): j = 0 .. J - 1, the component, stands in the bin's place of the counter word
 *     p 64 + j (J <= NUSI_DETECTOR_BINS_MAX = 64: the word holds j in 6 bits).  The counter's block word is 0x80000000 + r
 *     for round r = 0, 1, ..  The counts use blocks 0 .. 63 only (inversion block 0, PTRS rounds 0 .. 63), so under one
 *     seed the two families never share a block, and no count's bits depend on a normal draw.
 *   sigma == +inf (no prior): the result is center, and no bits are drawn.
 *   Round r, on the uniforms U0, U1 of block 0x80000000 + r:
 *     u = 2 U0 - 1, v = 2 U1 - 1 (both exact);  s = u u + v v (three roundings);  reject if !(s < 1) || s == 0;
 *     f = sqrt((-2 log(s)) / s) (the product exact; the quotient and the root each rounded);  z = u f;
 *     x = center + sigma z (the product, then the sum);  reject if !(x >= 0), else the draw is x.
 *   After NUSI_NORMAL_ROUNDS = 64 rejected rounds the draw is center.
 *
 * nusi_plan_draw_normals: d_out[row][p][j] = the draw around center[row][j] of width sigma[j] with the identity (seed,
 * stream_id, row, p, j), p < P: rows P J doubles in device memory.  center [rows][J] and sigma [J] are host arrays and are
 * copied; they share nusi_plan_draw_counts' staging buffer and its ordering (a draw waits for the one before).  No
 * detector is needed.  NUSI_EPARAM for a NULL center, sigma or d_out, rows < 1, J outside 1 .. NUSI_DETECTOR_BINS_MAX, P
 * outside 1 .. NUSI_DRAW_DATASETS_MAX, rows P J above NUSI_DRAW_COUNTS_MAX, a center that is negative or not finite, or a
 * sigma that is NaN or not > 0 (+inf is allowed); a refused call changes nothing.  _host: the output in host memory,
 * synchronous. */
#define NUSI_NORMAL_ROUNDS 64
int nusi_plan_draw_normals(nusi_plan *plan, const double *center /* [rows][J] */, const double *sigma /* [J] */, int rows,
                           int J, int P, unsigned long long seed, unsigned stream_id, double *d_out /* [rows][P][J] */,
                           void *stream);
int nusi_plan_draw_normals_host(nusi_plan *plan, const double *center, const double *sigma, int rows, int J, int P,
                                unsigned long long seed, unsigned stream_id, double *out);
/* The toys' treatment of constrained nuisances (NUSI_OPT_TOY_NUISANCE, a plan option; nusi_plan_response_inject,
 * nusi_plan_response_belt and their _host forms).  A prior (m_j, sigma_j) on template j stands for an auxiliary
 * measurement m_j.  Template j is CONSTRAINED where its prior has a weight w_j = 1 / sigma_j^2 > 0; sigma_j = +inf
 * otherwise.  The row of a toy's identity is the one its counts use: q in inject, q G + g in belt; the stream is t; the
 * component is the template, j = 0 .. K - 1.
 *   NUSI_TOYS_FIXED (0, the default): every toy redraws the counts and keeps the means m_j: the calls as written below.
 *   NUSI_TOYS_GLOBAL (1): the auxiliary measurements ("global observables") are redrawn per toy.  Per toy p and
 *     constrained template j, m*_j = the normal draw ("Drawing normals") around center_j of width sigma_j with the identity
 *     (seed, t, row, p, j).  The centre is the value the toys are thrown from: theta_inj[j] in inject, and in belt the
 *     observed conditional fit's theta_j(a) of the record -- d_theta_obs[t][q][1 + g][1 + j].  The counts are drawn from
 *     the unchanged mu_inj: every integer is FIXED's.  The toy's steps 2 - 4 -- the best fit, the conditional fit,
 *     lambda's penalties and the stops' magnitudes -- see the plan's priors with the mean of every constrained template
 *     replaced by m*_j: the toy's record is, bit for bit, what nusi_plan_response_fit / _fit_fixed give on a plan whose
 *     templates were set with the prior (m*, sigma) (m* >= 0 by the truncation).  belt's observed pass uses the plan's means.
 *   NUSI_TOYS_PRIOR (2; inject only): the nuisances are thrown from their priors (Cousins-Highland).  Per toy,
 *     theta*_j = the normal draw around m_j of width sigma_j with that identity for a constrained template, theta_inj[j]
 *     otherwise; the counts are drawn from a_inj s + sum_j theta*_j T_j + B in the usual order with the usual identity;
 *     the fits use the plan's means.  nusi_plan_response_belt under this value returns NUSI_EPARAM and does no device
 *     work: the profile construction has no such variant.
 * With K = 0 or no constrained template every value gives FIXED's bits (and runs FIXED's kernels).  A draw's identity is
 * global: every scratch budget, chunking and p-slicing give the same bits.  Any other value is refused.
 * nusi_plan_response_composition_belt builds the FIXED ensemble only: under GLOBAL or PRIOR with a constrained template
 * it returns NUSI_EPARAM and does no device work; without one it runs as under FIXED. */
#define NUSI_OPT_TOY_NUISANCE 17
#define NUSI_TOYS_FIXED 0
#define NUSI_TOYS_GLOBAL 1
#define NUSI_TOYS_PRIOR 2
/* nusi_plan_response_inject (k_inject, k_toys_band): the distribution of the statistic q(a) at a hypothesis, on toys drawn
 * from that hypothesis's own expectation -- critical values, toy-calibrated p-values, the coverage of a delta, discovery
 * power under an injected signal.  The toys exist only in registers: each is drawn where it is fitted.  The front half
 * s[t][q][c] = sum_n R[t][n][c] S[q][n] is computed once.  K = nusi_plan_templates(plan) = 0 .. 3.  For every table t,
 * spectrum q and toy p < P <= NUSI_BAND_DATASETS_MAX:
 *
 *   1. The datum of bin c is the draw ("Drawing counts", above) of
 *          mu_inj[c] = a_inj[q] s[t][q][c] (+ theta_inj[j] T_j[c], j ascending) + B[c]
 *      (nusi_plan_response_fit_fixed's order for mu) with the identity (seed, stream = t, row = q, p, c): the value
 *      nusi_plan_draw_counts gives at [q][p][c] for the rows mu_inj[t][.] and stream_id = t.  a_inj [Q] and theta_inj [K]
 *      are host arrays, finite and >= 0; a NULL theta_inj stands for the templates' prior means (0 without a prior).
 *   2. The best fit: nusi_plan_response_fit's record against that datum (nusi_plan_response_profile's at K = 0): its bits
 *      for theta_hat and its status word.
 *   3. The conditional fit with the signal held at a_test[q] (a NULL a_test: a_inj): nusi_plan_response_fit_fixed's, from
 *      that call's cold start, so its bits and its word.  It runs whatever the best fit did.  K = 0: the single
 *      evaluation mu = a_test s + B, word 0.
 *   4. lambda as nusi_plan_response_limit forms it at (a_test, theta) against the best fit -- per bin the ratio's term,
 *      the tree over the bins, then the penalties' differences ascending --, and
 *          stat = lambda > 0 ? 2 lambda : +0.0.
 *      mode NUSI_INJECT_TWO_SIDED: that; NUSI_INJECT_UPPER: stat = +0.0 where theta_hat_0 > a_test (the one-sided
 *      convention of an upper limit); NUSI_INJECT_DISCOVERY: stat = +0.0 where theta_hat_0 < a_test.  A best fit that is
 *      NUSI_FIT_NOT_CONVERGED or _SINGULAR: theta_hat_0 and stat are NaN; a conditional fit so flagged: stat is NaN.
 *      There is no other special case: a spectrum of zeros gets what these rules give.
 *   5. Per (t, q), on the device: d_band_theta and d_band_stat [ntab][Q][NR], the order statistics of the P values of
 *      theta_hat_0 and of stat at rank [NR] under the key (isnan(x), x) (nusi_plan_response_ensemble_limit's band; both
 *      series are non-negative doubles or NaN, never -0.0).  d_tally [ntab][Q][4] (ints) counts the toys whose best fit
 *      failed (NOT_CONVERGED or SINGULAR); whose conditional fit failed and whose best fit did not, so that the toys with
 *      a statistic are P - tally[0] - tally[1]; whose best fit has theta_hat_0 = 0 (NUSI_FIT_BOUNDARY or _FLAT); and whose
 *      best fit is NUSI_FIT_INFINITE.  d_exceed [ntab][Q] (ints) counts the toys with stat >= q_obs[t][q]; it comes with
 *      the host array q_obs [ntab][Q] and only with it; a NaN on either side never counts.  The toy p-value is
 *      exceed / (P - tally[0] - tally[1]).
 *   6. The raw records, the toy index fastest: d_theta_all, d_stat_all [ntab][Q][P] (doubles), d_words_all [ntab][Q][P][2]
 *      (ints; [0] the best fit's word, [1] the conditional fit's) and d_data_all [ntab][Q][P][C], the drawn counts.
 *
 * Every output is a DEVICE pointer and may be NULL; NR > 0 needs one band at least, and a band not given is not formed.
 * Scratch and the grid are nusi_plan_response_ensemble_limit's: units of one table and QB spectra, a series whose band
 * is asked for and whose raw array is not given kept in the plan's scratch (QB P 8 bytes a unit and series), chunks under
 * NUSI_OPT_ENSEMBLE_LIMIT_MB / _BYTES of at most 2^22 spectra, p-slices on the grid's z (NUSI_OPT_ENSEMBLE_PSLICES, or
 * automatic), the tally and exceed zeroed on the stream and added to with integer atomics.  A draw's identity is global,
 * so every budget and every slicing give the same bits.
 *
 * S, a_inj, theta_inj, a_test, rank and q_obs are host arrays and are copied.  Asynchronous and ordered with the plan's
 * other detector calls like nusi_plan_response_fit.  NUSI_ESTATE without a detector; NUSI_EPARAM for a NULL d_R, S or
 * a_inj, ntab < 1, Q outside 1 .. 2^19, P, NR or a rank out of range, a NULL rank with NR > 0, a mode outside 0 .. 2, NR >
 * 0 without a band, q_obs without d_exceed or the reverse, NR = 0 with no tally, exceed or raw output (nothing to do), a
 * negative or non-finite entry of S, a_inj, theta_inj or a_test, or a budget too small for one unit; a refused call
 * changes nothing.  _host: R and the outputs in host memory, synchronous. */
#define NUSI_INJECT_TWO_SIDED 0
#define NUSI_INJECT_UPPER 1
#define NUSI_INJECT_DISCOVERY 2
int nusi_plan_response_inject(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab, const double *S /* [Q][M] */,
                              int Q, const double *a_inj /* [Q] */, const double *theta_inj /* [K] or NULL */,
                              const double *a_test /* [Q] or NULL */, int P, unsigned long long seed, int mode,
                              const int *rank /* [NR] */, int NR, const double *q_obs /* [ntab][Q] or NULL */,
                              double *d_band_theta /* [ntab][Q][NR] */, double *d_band_stat /* [ntab][Q][NR] */,
                              int *d_tally /* [ntab][Q][4] */, int *d_exceed /* [ntab][Q] */,
                              double *d_theta_all /* [ntab][Q][P] */, double *d_stat_all /* [ntab][Q][P] */,
                              int *d_words_all /* [ntab][Q][P][2] */, double *d_data_all /* [ntab][Q][P][C] */,
                              void *stream);
int nusi_plan_response_inject_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q, const double *a_inj,
                                   const double *theta_inj, const double *a_test, int P, unsigned long long seed, int mode,
                                   const int *rank, int NR, const double *q_obs, double *band_theta, double *band_stat,
                                   int *tally, int *exceed, double *theta_all, double *stat_all, int *words_all,
                                   double *data_all);
/* nusi_plan_response_belt (k_belt, k_belt_accept): the toy-calibrated confidence interval of the signal's scale -- the
 * Feldman-Cousins interval by the profile construction -- on a grid of test scales, in one call.  What
 * nusi_plan_response_inject samples, this call inverts: per table t and spectrum q the set of grid points whose toy
 * p-value of the data exceeds alpha.  detector.belt_host / detector.belt_accept (numpy) are the same rules, and the call
 * reproduces them: the toys, theta_hat, the words' flags, the counts and the interval to the bit, q_obs and stat as
 * nusi_plan_response_inject reproduces inject_host's.  K = nusi_plan_templates(plan) = 0 .. 3.
 *
 *   The grid.  a[t][q][g] = frac[g] ref[t][q], one multiplication; frac [G] finite, >= 0 and strictly ascending, G = 1 ..
 *     NUSI_BELT_GRID_MAX; ref [ntab][Q], NULL = 1.  A ref that is NaN, infinite or negative -- what
 *     nusi_plan_response_limit returns for a failed or unbounded record -- or a product that is infinite gives
 *     NUSI_BELT_NO_GRID and is not refused: agood = ref >= 0 && a < inf, and the fits of such a point run at 0.
 *   The observed side.  d_theta_obs [ntab][Q][1 + G][1 + K] and d_words_obs [ntab][Q][1 + G]: [0] is
 *     nusi_plan_response_fit's record against data [C] (nusi_plan_response_profile's at K = 0), theta_hat and its word;
 *     NOT_CONVERGED or SINGULAR there gives NUSI_BELT_NO_FIT and no valid point.  [1 + g] is
 *     nusi_plan_response_fit_fixed's record at a from that call's cold start (K = 0: the single evaluation, word 0), theta
 *     with [0] = a; a point that is not agood has NaN and word 0 there.  A conditional fit so flagged after a good best
 *     fit gives NUSI_BELT_BAD_POINT.  d_q_obs [ntab][Q][G]: steps 2 - 4 of nusi_plan_response_inject applied to the data
 *     at a -- lambda by the ratio form, q_obs = lambda > 0 ? 2 lambda : +0.0, and +0.0 under NUSI_INJECT_UPPER where
 *     theta_hat_0 > a --, so a toy equal to the data in every bin has stat == q_obs to the bit.  A point is VALID iff it
 *     is agood and neither observed word is flagged; an invalid point has q_obs = NaN, no toys, counts of 0 and raw
 *     outputs of NaN (doubles) and 0 (ints and the counts of data_all).
 *   The toys.  Toy p < P of a valid point is the draw ("Drawing counts") of the observed conditional fit's own mu,
 *         mu_inj[c] = a s[t][q][c] (+ theta_j T_j[c], j ascending) + B[c],
 *     with the identity (seed, stream = t, row = q G + g, p, c), and gets steps 2 - 4 of nusi_plan_response_inject at
 *     a_test = a under `mode` (NUSI_INJECT_TWO_SIDED or NUSI_INJECT_UPPER).  d_theta_all, d_stat_all [ntab][Q][G][P],
 *     d_words_all [..][P][2] and d_data_all [..][P][C] are that call's raw records with g in front of p; d_tally
 *     [ntab][Q][G][4] and d_exceed [ntab][Q][G] its counts, exceed against q_obs[t][q][g] (a NaN on either side never
 *     counts), zeroed on the stream and added to with integer atomics.
 *   Acceptance.  nv = P - tally[0] - tally[1]; a point is accepted iff it is valid, nv > 0 and (double)exceed > alpha
 *     (double)nv -- one multiplication, one strict comparison; alpha in (0, 1).  d_idx [ntab][Q][2]: the first and the
 *     last accepted g; d_lo, d_hi [ntab][Q]: a there; none accepted: -1 and NaN.  d_status [ntab][Q]: NUSI_BELT_NO_GRID,
 *     _NO_FIT, _BAD_POINT (above, or a point with nv <= 0), _EMPTY (no point accepted), _LO_EDGE (idx[0] = 0), _HI_EDGE
 *     (idx[1] = G - 1), _GAPS (a point between the two is not accepted).  Nothing is interpolated.
 *
 * Every output is a DEVICE pointer and may be NULL, but not all of them.  The grid is nusi_plan_response_inject's with
 * the records in the spectra's place: units of one table and QB rows of its Q G, p-slices on the grid's z
 * (NUSI_OPT_ENSEMBLE_PSLICES, or automatic); every p-slice recomputes a record's observed side and slice 0 stores it.
 * Where the interval is asked for (d_lo, d_hi, d_idx or d_status), exceed, tally and words_obs are needed: one the caller
 * does not give lives in the plan's scratch, 4 G, 16 G and 4 (1 + G) bytes a (t, q) pair, and the call runs in chunks of
 * whole pairs under NUSI_OPT_ENSEMBLE_LIMIT_MB / _BYTES, of at most 2^22 records.  A draw's identity is global, so every
 * budget and every slicing give the same bits.
 *
 * nusi_belt_shape: the call's size limits as a pure function -- no plan, no device; the call itself applies it with the
 * detector's C.  NUSI_OK and *units (if not NULL) = ntab ceil(Q G / QB), the units of the whole call, or NUSI_EPARAM for
 * C outside 1 .. NUSI_DETECTOR_BINS_MAX, ntab < 1, Q outside 1 .. 2^19, G outside 1 .. NUSI_BELT_GRID_MAX, P outside 1 ..
 * NUSI_DRAW_DATASETS_MAX (no series is kept, so the band's 4096 does not bind; element counts are size_t) or ntab Q G >=
 * 2^31 (a record's row in an int).
 *
 * S, data, frac and ref are host arrays and are copied (they ride behind the spectra in the plan's staging block).
 * Asynchronous and ordered with the plan's other detector calls like nusi_plan_response_fit.  NUSI_ESTATE without a
 * detector; NUSI_EPARAM for nusi_belt_shape's limits, a NULL d_R, S, data or frac, a frac that is not finite, negative or
 * not strictly ascending, a mode other than the two, an alpha outside (0, 1), a negative or non-finite entry of S or
 * data, every output NULL (nothing to do), or a budget below one pair's scratch; a refused call changes nothing and does
 * no device work.  _host: R and the outputs in host memory, synchronous. */
#define NUSI_BELT_GRID_MAX 64
#define NUSI_BELT_NO_GRID 1
#define NUSI_BELT_NO_FIT 2
#define NUSI_BELT_BAD_POINT 4
#define NUSI_BELT_EMPTY 8
#define NUSI_BELT_LO_EDGE 16
#define NUSI_BELT_HI_EDGE 32
#define NUSI_BELT_GAPS 64
int nusi_belt_shape(int C, int ntab, int Q, int G, int P, long long *units);
int nusi_plan_response_belt(nusi_plan *plan, const double *d_R /* [ntab][M][C] */, int ntab, const double *S /* [Q][M] */,
                            int Q, const double *data /* [C] */, const double *frac /* [G] */, int G,
                            const double *ref /* NULL = 1, else [ntab][Q] */, int P, unsigned long long seed, int mode,
                            double alpha, double *d_lo /* [ntab][Q] */, double *d_hi /* [ntab][Q] */,
                            int *d_idx /* [ntab][Q][2] */, int *d_status /* [ntab][Q] */, int *d_exceed /* [ntab][Q][G] */,
                            int *d_tally /* [ntab][Q][G][4] */, double *d_q_obs /* [ntab][Q][G] */,
                            double *d_theta_obs /* [ntab][Q][1 + G][1 + K] */, int *d_words_obs /* [ntab][Q][1 + G] */,
                            double *d_theta_all /* [ntab][Q][G][P] */, double *d_stat_all /* [ntab][Q][G][P] */,
                            int *d_words_all /* [ntab][Q][G][P][2] */, double *d_data_all /* [ntab][Q][G][P][C] */,
                            void *stream);
int nusi_plan_response_belt_host(nusi_plan *plan, const double *R, int ntab, const double *S, int Q, const double *data,
                                 const double *frac, int G, const double *ref, int P, unsigned long long seed, int mode,
                                 double alpha, double *lo, double *hi, int *idx, int *status, int *exceed, int *tally,
                                 double *q_obs, double *theta_obs, int *words_obs, double *theta_all, double *stat_all,
                                 int *words_all, double *data_all);
/* nusi_plan_response_composition_belt (k_composition_belt, k_composition_accept): the toy-calibrated confidence region
 * of the source's flavour composition -- the Feldman-Cousins region by the profile construction -- on a grid of
 * compositions, in one call.  What nusi_plan_response_belt does for the signal's scale, this call does for the point
 * phi of the flavour triangle: per table t and spectrum q the set of grid points whose toy p-value of the data exceeds
 * alpha.  The statistic is q(phi) = 2 (min f at the held composition phi - the free minimum) of
 * nusi_plan_response_fit_components, which is chi^2 only away from the boundary theta_j >= 0 -- where most fits end --,
 * so the toys calibrate it.  detector.composition_belt_host / detector.composition_accept (numpy) are the same rules, and
 * the call reproduces them: the toys, theta, the words' flags, the counts and the mask to the bit, q_obs and stat to the
 * last bits of the log.  K = nusi_plan_templates(plan) = 0 .. 3.
 *
 *   The input.  d_R3 [ntab][3][M][C], a folded stack: nusi_plan_response_fit_components' input with J = 3 (J = 2 is not
 *     built).  phi [G][3], or [ntab][G][3] where phi_tables != 0: weights on the three rows, finite, >= 0 and not all
 *     three zero; G = 1 .. NUSI_REGION_GRID_MAX.
 *   A record (t, q, g) goes through four steps.
 *   1. The held signal: the composed row in nusi_plan_response_compose's expression, then the events call's accumulator,
 *         r[n][c] = (phi_0 R3[t][0][n][c] + phi_1 R3[t][1][n][c]) + phi_2 R3[t][2][n][c],  s_phi[c] = sum_n r[n][c] S[q][n],
 *     n ascending from 1, every product and sum rounded: bit for bit the front half that nusi_plan_response_fit /
 *     _profile compute on the composed matrix.  The three components s_j[c] are nusi_plan_response_fit_components'.
 *   2. The free fit against a data set d: nusi_plan_response_fit_components' record with J = 3 and the K templates,
 *     theta_hat [3 + K], mu_hat, word.
 *   3. The held fit at phi_g: with templates nusi_plan_response_fit's record on X = [s_phi, T_1 .. T_K]; at K = 0
 *     nusi_plan_response_profile's on s_phi.  The composition is held; its overall scale and the templates float.  theta
 *     [1 + K], mu, word.
 *   4. The statistic: lambda as nusi_plan_response_limit forms it -- per bin (mu - mu_hat) - d log(mu / mu_hat) over the
 *     bins with d > 0 and mu_hat > 0 (mu - mu_hat on the others), the tree sum, then the templates' penalty differences
 *     ascending, the held theta_j against theta_hat_{3 + j - 1} --, stat = lambda > 0 ? 2 lambda : +0.0, and NaN where
 *     either word has NUSI_FIT_NOT_CONVERGED | NUSI_FIT_SINGULAR.  There is no one-sided mode.
 *   The observed side.  Steps 2 - 4 on data [C] give d_q_obs [ntab][Q][G]; d_theta_obs [ntab][Q][1 + G][3 + K]: [0] is
 *     the free fit's theta_hat, [1 + g] the held fit's theta in slots 0 .. K with the other slots +0.0; d_words_obs
 *     [ntab][Q][1 + G] the words.  A point is VALID iff neither observed word is flagged: a flagged free fit gives
 *     NUSI_REGION_NO_FIT for the pair, a flagged held fit after a good free fit NUSI_REGION_BAD_POINT.  An invalid point
 *     has q_obs = NaN, no toys, counts of 0 and raw outputs of NaN (doubles) and 0 (ints and the counts of data_all).
 *   The toys.  Toy p < P of a valid point is the draw ("Drawing counts") of the observed held fit's own mu with the
 *     identity (seed, stream = t, row = q G + g, p, c) -- nusi_plan_response_belt's convention -- and gets steps 2 - 4 at
 *     phi_g.  d_theta_all [ntab][Q][G][P][3 + K] (the free fit's theta_hat, NaN where it failed), d_stat_all
 *     [ntab][Q][G][P], d_words_all [..][P][2] (the free fit's word, the held fit's) and d_data_all [..][P][C] are the raw
 *     records.  d_exceed [ntab][Q][G]: the toys with stat >= q_obs (a NaN on either side never counts).  d_tally
 *     [ntab][Q][G][4]: [0] the free fit failed, [1] the held fit failed and the free fit did not, [2] the free fit ends
 *     with a SIGNAL component at zero (NUSI_FIT_ZERO << j for a j < 3, NUSI_FIT_BOUNDARY or NUSI_FIT_FLAT: how far from
 *     Wilks' theorem the record is), [3] the free fit is NUSI_FIT_INFINITE.  Both are zeroed on the stream and added to
 *     with integer atomics.
 *   Acceptance.  nv = P - tally[0] - tally[1]; a point is accepted iff it is valid, nv > 0 and (double)exceed > alpha
 *     (double)nv -- one multiplication, one strict comparison; alpha in (0, 1).  d_accept [ntab][Q][G]: 0 or 1.  d_status
 *     [ntab][Q]: NUSI_REGION_NO_FIT, _BAD_POINT (above, or a valid point with nv <= 0), _EMPTY (no point accepted), _ALL
 *     (there is a valid point and every valid point is accepted: the grid does not bound the region).  d_best [ntab][Q]:
 *     the g of the smallest q_obs among the valid points, ties to the lowest g, or -1.  Nothing is interpolated.
 *
 * Every output is a DEVICE pointer and may be NULL, but not all of them; d_accept, d_status or d_best need d_exceed,
 * d_tally, d_q_obs and d_words_obs (no plan scratch, no budget chunking).  The grid is nusi_plan_response_belt's: units of
 * one table and QB rows of its Q G, cut into launches of at most 2^22 units, p-slices on the grid's z
 * (NUSI_OPT_ENSEMBLE_PSLICES, or automatic); every p-slice recomputes a record's observed side and slice 0 stores it.  A
 * draw's identity is global, so every slicing gives the same bits.  Only the FIXED toy ensemble is built: where
 * NUSI_OPT_TOY_NUISANCE is not NUSI_TOYS_FIXED and a template is constrained, the call returns NUSI_EPARAM.
 *
 * nusi_composition_belt_shape: the call's size limits as a pure function -- no plan, no device; the call itself applies
 * it with the detector's C and the plan's K.  NUSI_OK and *units (if not NULL) = ntab ceil(Q G / QB), or NUSI_EPARAM for
 * C outside 1 .. NUSI_DETECTOR_BINS_MAX, K outside 0 .. NUSI_FIT_TEMPLATES_MAX, ntab < 1, Q outside 1 .. 2^19, G outside
 * 1 .. NUSI_REGION_GRID_MAX, P outside 1 .. NUSI_DRAW_DATASETS_MAX, ntab Q G >= 2^31 (a record's row in an int), or an
 * observed-side output's element count -- ntab Q (1 + G) (3 + K), the widest -- >= 2^31, nusi_fit_components_shape's rule
 * (the raw arrays' counts are size_t).
 *
 * S, data and phi are host arrays and are copied.  Asynchronous and ordered with the plan's other detector calls like
 * nusi_plan_response_fit.  NUSI_ESTATE without a detector; NUSI_EPARAM for the shape limits, a NULL d_R3, S, data or phi,
 * a phi entry that is negative or not finite or a point with all three zero, an alpha outside (0, 1), a negative or
 * non-finite entry of S or data, every output NULL, the dependency rule above, or the toy ensemble; a refused call
 * changes nothing and does no device work.  _host: R3 and the outputs in host memory, synchronous. */
#define NUSI_REGION_GRID_MAX 1024
#define NUSI_REGION_NO_FIT 1
#define NUSI_REGION_BAD_POINT 2
#define NUSI_REGION_EMPTY 4
#define NUSI_REGION_ALL 8
int nusi_composition_belt_shape(int C, int K, int ntab, int Q, int G, int P, long long *units);
int nusi_plan_response_composition_belt(nusi_plan *plan, const double *d_R3 /* [ntab][3][M][C] */, int ntab,
                                        const double *S /* [Q][M] */, int Q, const double *data /* [C] */,
                                        const double *phi /* [G][3] or [ntab][G][3] */, int phi_tables, int G, int P,
                                        unsigned long long seed, double alpha, int *d_accept /* [ntab][Q][G] */,
                                        int *d_status /* [ntab][Q] */, int *d_best /* [ntab][Q] */,
                                        int *d_exceed /* [ntab][Q][G] */, int *d_tally /* [ntab][Q][G][4] */,
                                        double *d_q_obs /* [ntab][Q][G] */,
                                        double *d_theta_obs /* [ntab][Q][1 + G][3 + K] */,
                                        int *d_words_obs /* [ntab][Q][1 + G] */,
                                        double *d_theta_all /* [ntab][Q][G][P][3 + K] */,
                                        double *d_stat_all /* [ntab][Q][G][P] */, int *d_words_all /* [ntab][Q][G][P][2] */,
                                        double *d_data_all /* [ntab][Q][G][P][C] */, void *stream);
int nusi_plan_response_composition_belt_host(nusi_plan *plan, const double *R3, int ntab, const double *S, int Q,
                                             const double *data, const double *phi, int phi_tables, int G, int P,
                                             unsigned long long seed, double alpha, int *accept, int *status, int *best,
                                             int *exceed, int *tally, double *q_obs, double *theta_obs, int *words_obs,
                                             double *theta_all, double *stat_all, int *words_all, double *data_all);
/* Kernel times (ms) of the last nusi_plan_evolve* / nusi_plan_response*: [0] Gamma/alphaTilde
 * tables, [1] alpha table, [2] cascade.  Synchronises the plan's stream. */
int nusi_plan_stage_ms(nusi_plan *plan, float *ms3);
/* Kernel-time accounting over many calls (bench): after profile_begin, each
 * nusi_plan_evolve records HIP events around its three kernels on the launch
 * stream (up to max_calls calls); profile_end synchronises and returns the
 * summed ms per stage and the number of calls recorded. */
int nusi_plan_profile_begin(nusi_plan *plan, int max_calls);
int nusi_plan_profile_end(nusi_plan *plan, double *sum_ms3, int *ncalls);
/* Cascade kernel of the plan's later calls.  Every kind meets the same flux
 * tolerance against the reference algorithm (<= 1e-11 relative, the same
 * exact zeros); the choice is a performance / cross-check knob:
 * AUTO (default, also for the object API) = MFMA.
 * MFMA = the block-synchronous wavefront with the push on the fp64 matrix
 *   cores (k_cascade_bs: one pass up to 48 redshift steps, step passes
 *   beyond), for every source and both scattering modes; points sharing a
 *   Stage-A table share one workgroup (multi-RHS: pairs, or the gamma batch
 *   of up to 16).  Grids beyond its limits (T - 1 > 14 x 128 rows) fall back
 *   to the scalar kernel.
 * WAVEFRONT, REG, LDS = the bit-exact scalar cascade k_cascade (one
 *   wavefront per point, any N; right-looking fma()s in one fixed order).
 *   The three names are kept for the API; since round 5 they select the same
 *   kernel.
 * NUSI_EPARAM for an unknown kind. */
#define NUSI_CASCADE_AUTO 0
#define NUSI_CASCADE_WAVEFRONT 1
#define NUSI_CASCADE_REG 2
#define NUSI_CASCADE_LDS 3
#define NUSI_CASCADE_MFMA 4
int nusi_plan_set_cascade(nusi_plan *plan, int kind);
/* Explicit A/B and test options of a plan (no reference counterpart).  The
 * defaults are the production choices, and nothing in the library reads the
 * environment to select kernels.  NUSI_EPARAM for an unknown option or value.
 *   NUSI_OPT_ALPHA_BATCH   max tables per alpha batch (tables sharing m_phi,
 *                          masses and flags), 1..255; 0 = automatic
 *   NUSI_OPT_ALPHA_KERNEL  0 = k_alpha_batch (default), 1 = k_alpha_tile
 *                          batches of <= 4, 2 = one entry per work-item
 *                          (all three give the same tables bit for bit)
 *   NUSI_OPT_CASCADE_RHS   max points sharing a table per MFMA-cascade
 *                          workgroup: 0 = automatic (the gamma batch for
 *                          tables with >= 3 points, pairs for two), 1 = one
 *                          point each, 2 = pairs (k_cascade_bs_pairs),
 *                          3..16 = the gamma batch k_cascade_bs_gamma (the
 *                          points of a table, gamma on the MFMA N
 *                          dimension) of up to that many.  The MFMA sums in
 *                          blocks of four columns, so a point's fluxes depend
 *                          on its grouping to rounding (<= 1e-13), not bit for
 *                          bit; 1 makes them independent of the call's other
 *                          points
 *   NUSI_OPT_STEP_PASSES   0 = automatic (step passes beyond 48 redshift
 *                          steps), 1 = always the step-pass instance (one
 *                          point per workgroup)
 *   NUSI_OPT_SHIFT_REUSE   opt-in scan mode, K in
 *                          [0, 128]; 0 = off (default).  alpha / Gamma /
 *                          alphaTilde see the energies only through
 *                          2 m_k E / m_phi^2 (nuSIprop.hpp:1253-1256), so the
 *                          tables of m_phi' = m_phi r^(-o/2) (r = Emax[0] /
 *                          Emin[0], integer o) equal those of m_phi read o
 *                          bins higher.  Tables of one (g, masses, flags)
 *                          whose m_phi lie on that lattice within K bins of
 *                          the largest are served by ONE table set of the
 *                          largest m_phi on the axis extended by K bins.  Not
 *                          bit-exact: the bin edges round differently, and the
 *                          flux's optical depth amplifies that with the
 *                          coupling, so only tables with g <= 0.05 share
 *                          (measured <= 8.8e-10 relative there; 3e-8 at g = 1
 *                          had they shared; tests/test_shift_reuse.py); the
 *                          default path is unchanged. */
#define NUSI_OPT_ALPHA_BATCH 1
#define NUSI_OPT_ALPHA_KERNEL 2
#define NUSI_OPT_CASCADE_RHS 3
#define NUSI_OPT_STEP_PASSES 4
#define NUSI_OPT_SHIFT_REUSE 5
/*   NUSI_OPT_REFERENCE_ORDER  1 (DEFAULT, plans and objects) = build Gamma /
 *                          alphaTilde / alpha in the reference's own
 *                          arithmetic: every gsl_sf_dilog /
 *                          gsl_sf_complex_dilog_xy_e call site by GSL's own
 *                          algorithms (dilog.c restated, nusi_gsl.hpp), and
 *                          the alpha table's s-t interference member leaves
 *                          as the dilogarithm of the reference's quotient
 *                          (1+S+t)/(2 - i gr + t) and carg of its expression
 *                          (nuSIprop.hpp:1428-1467, 843-878, 1135-1192).
 *                          Fluxes <= 1e-11 of the GSL-restating oracle on
 *                          every tested config.
 *                          0 = opt-in fast mode, the shared-algorithm order
 *                          (Bernoulli series, batch-shared Taylor
 *                          coefficients; ~3x faster Stage A).  Bit-identical
 *                          to the oracle's default mode, but where the closed
 *                          forms cancel it differs from the reference's
 *                          arithmetic by up to 2.5e-6 (C2a) / 1.3e-7 (C4 at
 *                          g = 1) in a flux. */
#define NUSI_OPT_REFERENCE_ORDER 6
/*   NUSI_OPT_CASCADE_SYNC  the MFMA cascade's synchronisation: 0 = automatic
 *                          = 2 = the block-synchronous kernel k_cascade_bs
 *                          (every wave meets twice per block of four
 *                          stages).  1 (the per-stage kernels k_cascade_ws /
 *                          gb / wsp of rounds 2-3) is refused: those kernels
 *                          were removed in round 5. */
#define NUSI_OPT_CASCADE_SYNC 7
/*   NUSI_OPT_REFO_CORNER_MB  the reference-order big-batch kernel's member-
 *                          corner block (per table and pair of bin edges,
 *                          Dc = Li2(quotient) as re/im for each of the 3
 *                          mass states: 6 doubles, 3.7 MB per table at
 *                          N_E = 300): at most this many MiB, the batches run
 *                          in chunks that fit (at least one batch); 0 =
 *                          automatic (8 GiB, at most half the free memory).
 *                          Any value gives the same tables bit for bit. */
#define NUSI_OPT_REFO_CORNER_MB 8
/*   NUSI_OPT_GA_BATCH      the reference order's Gamma / alphaTilde path:
 *                          0 = automatic (the batch path for calls of more
 *                          than 16 tables), 1 = the per-table kernel,
 *                          2 = the batch path whenever alpha batches exist
 *                          (NUSI_OPT_ALPHA_KERNEL 0), also for calls of few
 *                          tables.  The batch path evaluates the
 *                          dilogarithms that do not read the coupling once
 *                          per batch and the others with a batch's tables on
 *                          neighbouring lanes (k_ga_dilogs_batch).  Any value
 *                          gives the same tables bit for bit.
 *   NUSI_OPT_GA_PRE_MB     the batch path's block of dilogarithm values: at
 *                          most this many MiB, the batches run in chunks
 *                          that fit (at least one batch); 0 = 512.  Any
 *                          value gives the same tables bit for bit.
 *   NUSI_OPT_GA_PRE_KB     the same budget in KiB (> 0: it holds instead of
 *                          NUSI_OPT_GA_PRE_MB): a small grid's batch takes
 *                          far less than a MiB (21 KB per table at N_E = 45),
 *                          and the tests cut such a call into chunks. */
#define NUSI_OPT_GA_BATCH 9
#define NUSI_OPT_GA_PRE_MB 10
#define NUSI_OPT_GA_PRE_KB 11
/*   NUSI_OPT_RESPONSE_FIFO_KB  nusi_plan_response's impulse cascade hands its
 *                          step passes on through a FIFO of 3 N 16 doubles
 *                          per workgroup (2.5 MB per table at N_E = 300): at
 *                          most this many KiB, the tables run in chunks that
 *                          fit (at least one table); 0 = 1 GiB.  Any value
 *                          gives the same bits. */
#define NUSI_OPT_RESPONSE_FIFO_KB 12
/*   NUSI_OPT_ENSEMBLE_QSLICES, NUSI_OPT_ENSEMBLE_PSLICES  the grid of
 *                          nusi_plan_response_ensemble is (tables, q-slices,
 *                          p-slices): a block takes the spectrum blocks of its
 *                          q-slice and the data sets of its p-slice.  0 =
 *                          automatic (the grid fills the card, the q-slices'
 *                          records stay within 256 MiB of scratch); n >= 1 =
 *                          exactly min(n, what there is to split) (tests: every
 *                          path at small shapes).  Any value gives the same
 *                          bits. */
#define NUSI_OPT_ENSEMBLE_QSLICES 13
#define NUSI_OPT_ENSEMBLE_PSLICES 14
/*   NUSI_OPT_ENSEMBLE_LIMIT_MB  the scratch of nusi_plan_response_ensemble_limit
 *                          (a spectrum's P limits per side whose raw array
 *                          the caller does not give): at most this many MiB,
 *                          the call runs in chunks of (table, spectrum block)
 *                          units that fit; 0 = 256.  A budget below one unit
 *                          (QB P 8 bytes per such side) makes the call fail
 *                          with NUSI_EPARAM.  Any value gives the same bits.
 *   NUSI_OPT_ENSEMBLE_LIMIT_BYTES  the same budget in bytes, up to 2^30 (> 0:
 *                          it holds instead of NUSI_OPT_ENSEMBLE_LIMIT_MB):
 *                          for calls whose units are far smaller than a MiB
 *                          (a unit at C = 64 and P = 16 is 512 bytes a side),
 *                          where a budget in MiB cannot bound the scratch any
 *                          closer than to the whole call. */
#define NUSI_OPT_ENSEMBLE_LIMIT_MB 15
#define NUSI_OPT_ENSEMBLE_LIMIT_BYTES 16
/*   NUSI_OPT_TOY_NUISANCE  (17, defined with the calls it governs, above: "The toys' treatment of constrained
 *                          nuisances") NUSI_TOYS_FIXED = 0 (default), NUSI_TOYS_GLOBAL = 1, NUSI_TOYS_PRIOR = 2. */
int nusi_plan_set_option(nusi_plan *plan, int option, int value);
/* per-point NUSI_WARN_* bits of the last call */
int nusi_plan_warnings(nusi_plan *plan, int *out, int n);
/* Names of the main alpha-table and cascade kernels the last call launched (static strings, e.g.
 * "k_alpha_batch", "k_cascade_bs"); for reports -- bench.py's roofline lines.  No reference
 * counterpart. */
int nusi_plan_kernels(const nusi_plan *plan, const char **alpha, const char **cascade);
/* The Gamma / alphaTilde path of the last call (a static string): "k_gamma_alphat" (the per-table kernel),
 * "k_ga_dilogs + k_gamma_alphat[pre]" (calls of few tables) or "k_ga_dilogs_batch + k_gamma_alphat[pre]" (the batch
 * path, NUSI_OPT_GA_BATCH). */
int nusi_plan_ga_kernel(const nusi_plan *plan, const char **ga);
/* Copy point `i`'s Stage-A tables of the last call to the host (parity
 * tests): Gamma[T], alphaTilde[T], alpha packed transposed [T(T-1)/2] with
 * alpha(n,m), n<m, at m(m-1)/2+n.  Any pointer may be NULL. */
int nusi_plan_tables(nusi_plan *plan, int i, double *Gamma, double *alphaTilde, double *alpha_packed);

/* Convenience: evolve n points on `device` with host buffers (creates a
 * transient plan; points must share the grid). */
int nusi_evolve_batch(int device, const nusi_params *pts, int n, double *flux, double *flux_fla);

#ifdef __cplusplus
}
#endif
#endif /* NUSI_H */
