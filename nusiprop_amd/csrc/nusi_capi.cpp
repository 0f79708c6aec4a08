// nuSIprop MI355X -- C ABI (include/nusi.h): host set-up, plans, object API.
//
// Host work here is the reference's per-object scalar set-up only (grid,
// mixing matrix, masses, normalisation; nuSIprop.hpp:102-171, 184-205) and
// the energy-conservation diagnostic; the table build and the cascade run
// on the GPU (nusi_kernels.hip).  There is no CPU fallback.
#include <climits>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <tuple>
#include <array>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <string>
#include <utility>
#include <vector>

#include "nusi.h"
#include "nusi_internal.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg)
{
    g_err = msg;
    return code;
}

#define HIPCHECK(x)                                                                              \
    do {                                                                                         \
        hipError_t e_ = (x);                                                                     \
        if (e_ != hipSuccess) return fail(NUSI_EHIP, std::string("HIP error: ") + hipGetErrorString(e_) + " (" #x ")"); \
    } while (0)

inline double sq(double a) { return a * a; }
inline double cu(double a) { return a * a * a; }

// ---------------------------------------------------------------------------
// grid: constructor nuSIprop.hpp:113-128, table axis :224-233, per-step
// scalars of the cascade :256-259, 268-269, 283
// ---------------------------------------------------------------------------
struct HostGrid {
    int N = 0, Nz = 0, T = 0;
    double lEmin = 0, lEmax = 0, zmax_in = 0, zmax_eff = 0;
    std::vector<double> Emin, Emax, Enu, z, lo, hi, step_c, step_s, sfr;
};

double hubble_h(double z) { return 1.5e-33 * pow(0.692 + 0.308 * cu(1 + z), 0.5); }
double n_nu_h(double z) { return 4.3528e-13 * cu(1 + z); }
double sfr_h(double z)
{
    return pow(pow(1 + z, -3.4 * 10) + pow((1 + z) / 5161, 0.3 * 10) + pow((1 + z) / 9.06, 3.5 * 10), -1. / 10.);
}

HostGrid make_grid(int N, double lEmin, double lEmax, double zmax)
{
    HostGrid G;
    G.N = N;
    G.lEmin = lEmin;
    G.lEmax = lEmax;
    G.zmax_in = zmax;
    G.Emin.resize(N);
    G.Emax.resize(N);
    G.Enu.resize(N);
    for (int i = 0; i < N; ++i) {
        G.Emin[i] = pow(10, lEmin + (lEmax - lEmin) * (i * 1.0) / N);
        G.Enu[i] = pow(10, lEmin + (lEmax - lEmin) * (i + 0.5) / N);
        G.Emax[i] = pow(10, lEmin + (lEmax - lEmin) * (i + 1.0) / N);
    }
    G.Nz = (int)(log((1 + zmax) / (1 + 0)) / log(G.Emax[0] / G.Emin[0]) + 2);
    G.z.resize(G.Nz);
    for (int i = 0; i < G.Nz; ++i) G.z[i] = (1 + 0) * pow(G.Emax[0] / G.Emin[0], i) - 1;
    G.zmax_eff = G.z[G.Nz - 1];
    G.T = N + G.Nz - 2;
    G.lo.resize(G.T);
    G.hi.resize(G.T);
    for (int n = 0; n < G.T; ++n) {
        if (n < N) {
            G.lo[n] = G.Emin[n];
            G.hi[n] = G.Emax[n];
        } else {
            G.lo[n] = G.Emin[N - 1] * (1 + G.z[n - N + 1]);
            G.hi[n] = G.Emax[N - 1] * (1 + G.z[n - N + 1]);
        }
    }
    G.step_c.assign(G.Nz, 0.0);
    G.step_s.assign(G.Nz, 0.0);
    const double dlogz = log(1 + G.z[1]) - log(1 + G.z[0]);
    for (int i = 1; i < G.Nz; ++i) {
        const double zz = G.z[i - 1];
        G.step_c[i] = (1 + zz) * dlogz / hubble_h(zz);
        G.step_s[i] = n_nu_h(zz) / sq(1 + zz);
    }
    G.sfr.resize(G.Nz);
    for (int i = 0; i < G.Nz; ++i) G.sfr[i] = sfr_h(G.z[i]);
    return G;
}

// |U_fk|^2 from NuFIT 5.0 angles, nuSIprop.hpp:130-163.  Only std::norm(U)
// is used by the reference; the complex entries are formed with explicit real
// operations (real*complex component-wise, s13/del by Smith's division, the
// algorithm of libgcc's __divdc3 for finite operands) so that the result does
// not depend on the host compiler's complex runtime.
void pmns_sq(bool normal, double U2[9])
{
    double t12, t13, t23, dcp;
    if (normal) {
        t12 = 33.44 * (M_PI / 180);
        t13 = 8.57 * (M_PI / 180);
        t23 = 49.0 * (M_PI / 180);
        dcp = 195.0 * (M_PI / 180);
    } else {
        t12 = 33.45 * (M_PI / 180);
        t13 = 8.61 * (M_PI / 180);
        t23 = 49.3 * (M_PI / 180);
        dcp = 286.0 * (M_PI / 180);
    }
    const double c12 = cos(t12), c13 = cos(t13), c23 = cos(t23);
    const double s12 = sin(t12), s13 = sin(t13), s23 = sin(t23);
    const nusi::cd del = nusi::C(cos(dcp), sin(dcp));
    nusi::cd U[3][3];
    U[0][0] = nusi::C(c12 * c13);
    U[0][1] = nusi::C(s12 * c13);
    U[0][2] = (s13 * 1.0) / del;
    U[1][0] = -s12 * c23 - (c12 * s23 * s13) * del;
    U[1][1] = c12 * c23 - (s12 * s23 * s13) * del;
    U[1][2] = nusi::C(s23 * c13);
    U[2][0] = s12 * s23 - (c12 * c23 * s13) * del;
    U[2][1] = -c12 * s23 - (s12 * c23 * s13) * del;
    U[2][2] = nusi::C(c23 * c13);
    for (int f = 0; f < 3; ++f)
        for (int k = 0; k < 3; ++k) U2[3 * f + k] = U[f][k].r * U[f][k].r + U[f][k].i * U[f][k].i;
}

// Lightest mass, aux.hpp:12-50.  The reference's quartic + constraint filter
// selects the unique root of the un-squared mass-sum equation, found here by
// bisection to full precision; at the minimal mass sum (root 0, where GSL
// returns rounding noise and m = 0 would make the tables NaN) the lightest
// mass is set to kMlFloor.
constexpr double kMlFloor = 1e-12;
double mass_sum(double m, double dmqSL, double dmqAT)
{
    if (dmqAT > 0) return m + sqrt(sq(m) + dmqSL) + sqrt(sq(m) + dmqAT);
    const double m2 = sqrt(sq(m) - dmqAT);
    return m + m2 + sqrt(sq(m2) - dmqSL);
}
bool lightest_mass(double mSum, double dmqSL, double dmqAT, double* mL)
{
    const double f0 = mass_sum(0.0, dmqSL, dmqAT) - mSum;
    double ml;
    if (f0 >= 0) {
        if (f0 > 64 * 2.220446049250313e-16 * mSum) return false;
        ml = kMlFloor;
    } else {
        double lo = 0.0, hi = mSum;
        for (int it = 0; it < 2000; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (mid <= lo || mid >= hi) break;
            if (mass_sum(mid, dmqSL, dmqAT) - mSum > 0) hi = mid;
            else lo = mid;
        }
        ml = (fabs(mass_sum(hi, dmqSL, dmqAT) - mSum) < fabs(mass_sum(lo, dmqSL, dmqAT) - mSum)) ? hi : lo;
        if (ml <= 0) ml = kMlFloor;
    }
    const bool ok1 = (mSum - ml > 1.0e-7);
    const bool ok2 = (dmqAT > 0) ? (sq(mSum) - dmqAT - dmqSL - sq(ml) - 2 * ml * mSum > 1.0e-7)
                                 : (sq(mSum) + 2 * dmqAT + dmqSL - sq(ml) - 2 * ml * mSum > 1.0e-7);
    if (!(ok1 && ok2)) return false;
    *mL = ml;
    return true;
}

const double kGLw[3] = {5. / 9., 8. / 9., 5. / 9.};
const double kGLx[3] = {-0.7745966692414834, 0.0, 0.7745966692414834};

// flux_FS_E0, nuSIprop.hpp:666-692
double flux_fs_e0(double si, double zmax_eff)
{
    double res = 0;
    const double z_min = 0, z_max = zmax_eff;
    const int NI = 100;
    for (int f = 0; f < NI; f++) {
        const double a = z_min + f * (z_max - z_min) / NI;
        const double b = z_min + (f + 1.0) * (z_max - z_min) / NI;
        double zz[3];
        for (int q = 0; q < 3; ++q) zz[q] = (b - a) / 2. * kGLx[q] + (b + a) / 2.;
        res += (b - a) / 2. * (kGLw[0] * pow(1 + zz[0], -si) * sfr_h(zz[0]) / hubble_h(zz[0])
                               + kGLw[1] * pow(1 + zz[1], -si) * sfr_h(zz[1]) / hubble_h(zz[1])
                               + kGLw[2] * pow(1 + zz[2], -si) * sfr_h(zz[2]) / hubble_h(zz[2]));
    }
    return res;
}

// energy_FS / Lum_times_E, nuSIprop.hpp:694-744 (power law; stale norm_total)
double energy_fs(double si, double norm_total, double zmax_eff, double lEmin, double lEmax)
{
    const double E0 = 1e14;
    auto lte = [&](double z, double Em, double Ep) {
        if (fabs(si - 2) < 1e-5)
            return norm_total * sfr_h(z) * pow(E0 / (1 + z), si) * (log(Ep / Em) + (2 - si) / 2.0 * (sq(log(Ep)) - sq(log(Em))));
        return norm_total * sfr_h(z) * pow(E0 / (1 + z), si) * (pow(Ep, 2 - si) - pow(Em, 2 - si)) / (2 - si);
    };
    double res = 0;
    const double z_min = 0, z_max = zmax_eff, lo = pow(10, lEmin), hi = pow(10, lEmax);
    for (int f = 0; f < 100; f++) {
        const double a = z_min + f * (z_max - z_min) / 100;
        const double b = z_min + (f + 1.0) * (z_max - z_min) / 100;
        double zz[3];
        for (int q = 0; q < 3; ++q) zz[q] = (b - a) / 2. * kGLx[q] + (b + a) / 2.;
        res += (b - a) / 2. * (kGLw[0] * lte(zz[0], lo, hi) / hubble_h(zz[0]) + kGLw[1] * lte(zz[1], lo, hi) / hubble_h(zz[1])
                               + kGLw[2] * lte(zz[2], lo, hi) / hubble_h(zz[2]));
    }
    return res;
}

// ---------------------------------------------------------------------------
// phi-phi tables (interp.hpp:173-320, binary branch) -> device SplineDev
// ---------------------------------------------------------------------------
struct SplineStore {
    int device = 0;
    std::vector<void*> bufs;
    nusi::SplineSet set;
    nusi::SplineSet* d_set = nullptr;   // `set` in device memory: the kernels take it by pointer (a by-value
                                        // kernel argument whose address reaches a call is copied to scratch
                                        // by every work-item, 320 B each)
    ~SplineStore()
    {
        if (bufs.empty()) return;
        int prev = 0;
        hipGetDevice(&prev);
        hipSetDevice(device);
        for (void* b : bufs) hipFree(b);
        hipSetDevice(prev);
    }
};

// weights of interp.hpp:576-636 (the last node's weights are never read), node-major: the 16 weights
// of node j at w[16 j + 4 a + b]
void spline_weights(const std::vector<double>& x, std::vector<double>& w)
{
    const int n = (int)x.size();
    w.assign((size_t)16 * n, 0.0);
    auto W = [&](int a, int b, int j) -> double& { return w[(size_t)16 * j + 4 * a + b]; };
    for (int j = 0; j + 1 < n; ++j) {
        const double xm = (j > 0) ? x[j - 1] : 0.0, x0 = x[j], x1 = x[j + 1], x2 = (j + 2 < n) ? x[j + 2] : 0.0;
        if (j == 0) {
            W(0, 1, j) = (x0 - x1) / (x0 - x2);
            W(0, 2, j) = (-1 + (x1 - x0) / (x0 - x2));
            W(0, 3, j) = 1;
            W(1, 1, j) = (x1 - x0) / (x1 - x2);
            W(1, 2, j) = (x0 - x2) / (x1 - x2);
            W(2, 1, j) = sq(x1 - x0) / ((x2 - x1) * (x2 - x0));
            W(2, 2, j) = sq(x1 - x0) / ((x2 - x1) * (x0 - x2));
        } else if (j == n - 2) {
            W(0, 1, j) = sq(x1 - x0) / ((xm - x0) * (xm - x1));
            W(0, 2, j) = sq(x1 - x0) / ((x0 - xm) * (xm - x1));
            W(1, 1, j) = (x1 - x0) / (xm - x0);
            W(1, 2, j) = (2 * x0 - x1 - xm) / (xm - x0);
            W(1, 3, j) = 1;
            W(2, 1, j) = (x0 - x1) / (xm - x1);
            W(2, 2, j) = (xm - x0) / (xm - x1);
        } else {
            W(0, 0, j) = sq(x1 - x0) / ((x0 - xm) * (xm - x1));
            W(0, 1, j) = 2 * sq(x1 - x0) / ((xm - x0) * (xm - x1));
            W(0, 2, j) = sq(x1 - x0) / ((x0 - xm) * (xm - x1));
            W(1, 0, j) = (x0 - x1) * (1 / (xm - x0) + 1 / (x0 - x2));
            W(1, 1, j) = (x0 - x1) * (2 / (x0 - xm) + 1 / (x2 - x0));
            W(1, 2, j) = (2 * x0 - x1 - xm) / (xm - x0);
            W(1, 3, j) = 1;
            W(2, 0, j) = (x1 - x0) * (1 / (xm - x1) + 1 / (x1 - x2));
            W(2, 1, j) = (x1 - x0) * (2 / (x1 - xm) + 1 / (x2 - x1));
            W(2, 2, j) = (xm - x0) / (xm - x1);
            W(3, 0, j) = sq(x1 - x0) / ((-x1 + x2) * (-x0 + x2));
            W(3, 1, j) = sq(x1 - x0) / ((x1 - x2) * (-x0 + x2));
        }
    }
}

// file identity for the table-set cache of nusi_plan_load_phiphi: path, device and inode, size and the
// modification time to the nanosecond (a file rewritten in place gets a new mtime)
std::string file_stamp(const char* path)
{
    struct stat sb;
    if (stat(path, &sb) != 0) return std::string(path) + "|?";
    return std::string(path) + "|" + std::to_string((unsigned long long)sb.st_dev) + ":" +
           std::to_string((unsigned long long)sb.st_ino) + "|" + std::to_string((long long)sb.st_size) + "|" +
           std::to_string((long long)sb.st_mtim.tv_sec) + "." + std::to_string((long long)sb.st_mtim.tv_nsec);
}
// the cache: one entry per key; its mutex is held while that key loads (1.6 GB read + upload + windows), so
// loads of other keys (e.g. the same files on another device) run concurrently
struct SplineSlot {
    std::mutex mu;
    std::weak_ptr<SplineStore> set;
};
std::mutex g_spl_mu;   // guards the map only
std::map<std::string, std::shared_ptr<SplineSlot>> g_spl_cache;

int load_spline(const char* path, int ndim, const int* dims, SplineStore& st, nusi::SplineDev& out)
{
    FILE* fp = fopen(path, "rb");
    if (!fp)
        return fail(NUSI_ETABLE, std::string("Error at interp: the input file ") + path + " does not exist");
    std::vector<std::vector<double>> x(ndim);
    size_t nf = 1;
    for (int i = 0; i < ndim; ++i) {
        x[i].assign(dims[i], 0.0);
        nf *= (size_t)dims[i];
    }
    std::vector<float> f(nf);
    std::vector<float> chunk((size_t)(ndim + 1) * 65536);
    size_t r = 0;
    while (r < nf) {
        const size_t want = std::min<size_t>(65536, nf - r);
        if (fread(chunk.data(), sizeof(float) * (ndim + 1), want, fp) != want) {
            fclose(fp);
            return fail(NUSI_ETABLE, std::string("Error at interp: the input file ") + path + " is truncated");
        }
        for (size_t q = 0; q < want; ++q, ++r) {
            size_t rem = r;
            int idx[nusi::kSplMaxDim];
            for (int i = ndim - 1; i >= 0; --i) {
                idx[i] = (int)(rem % (size_t)dims[i]);
                rem /= (size_t)dims[i];
            }
            const float* rec = &chunk[q * (ndim + 1)];
            for (int i = 0; i < ndim; ++i) x[i][idx[i]] = (double)rec[i];
            f[r] = rec[ndim];
        }
    }
    fclose(fp);
    nusi::SplineDev sd;
    sd.ndim = ndim;
    sd.islog[0] = 1;  // both reference tables interpolate in log(x0) (nuSIprop.hpp:168-169)
    for (int i = 0; i < ndim; ++i) {
        sd.n[i] = dims[i];
        if (sd.islog[i])
            for (double& v : x[i]) v = log(v);
        std::vector<double> w;
        spline_weights(x[i], w);
        double *dx = nullptr, *dw = nullptr;
        HIPCHECK(hipMalloc(&dx, sizeof(double) * x[i].size()));
        st.bufs.push_back(dx);
        HIPCHECK(hipMalloc(&dw, sizeof(double) * w.size()));
        st.bufs.push_back(dw);
        HIPCHECK(hipMemcpy(dx, x[i].data(), sizeof(double) * x[i].size(), hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(dw, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
        sd.x[i] = dx;
        sd.w[i] = dw;
        // guide table of the node search (nusi_spline.hpp): gd[u] = the last node <= the lower end of
        // bucket u, 4 (n-1) buckets over [x[0], x[n-1]]
        const std::vector<double>& xi = x[i];
        const int n = dims[i], G = 4 * (n - 1);
        const double h = (xi[n - 1] - xi[0]) / G;
        if (n >= 2 && h > 0 && std::is_sorted(xi.begin(), xi.end())) {
            std::vector<int> gd(G);
            for (int u = 0; u < G; ++u) {
                const double lo = xi[0] + u * h;
                const int k = (int)(std::upper_bound(xi.begin(), xi.end(), lo) - xi.begin()) - 1;
                gd[u] = std::max(0, std::min(n - 2, k));
            }
            int* dg = nullptr;
            HIPCHECK(hipMalloc(&dg, sizeof(int) * G));
            st.bufs.push_back(dg);
            HIPCHECK(hipMemcpy(dg, gd.data(), sizeof(int) * G, hipMemcpyHostToDevice));
            sd.gd[i] = dg;
            sd.ng[i] = G;
            sd.ginv[i] = 1.0 / h;
        }
    }
    float* df = nullptr;
    HIPCHECK(hipMalloc(&df, sizeof(float) * nf));
    st.bufs.push_back(df);
    HIPCHECK(hipMemcpy(df, f.data(), sizeof(float) * nf, hipMemcpyHostToDevice));
    sd.f = df;
    if (ndim == 3) {
        float* dw = nullptr;   // 16 x the table: the 4 x 4 windows of nusi_spline.hpp
        HIPCHECK(hipMalloc(&dw, sizeof(float) * 16 * nf));
        st.bufs.push_back(dw);
        HIPCHECK(nusi::spline_windows_build(df, dims[0], dims[1], dims[2], dw));
        sd.fw = dw;
    }
    out = sd;
    return NUSI_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------
// the alpha-table batches of one call (nusi::launch_alpha): count, how many lack the phi-phi channel, the cap
struct AlphaBatches {
    int nbatch = 0, nb_plain = 0, cap = 1;
};

struct nusi_plan {
    int device = 0;
    hipStream_t stream = nullptr;
    HostGrid grid;
    int max_points = 0;
    nusi::GridDev gd{};
    double* d_grid = nullptr;
    nusi::Point* d_pts = nullptr;
    nusi::Point* h_pts = nullptr;  // pinned
    nusi::Point* d_tpts = nullptr;  // one representative per distinct table (table kernels)
    nusi::Point* h_tpts = nullptr;  // pinned
    int* d_batches = nullptr;       // alpha-table batches (nusi::launch_alpha): first table | count << 24
    int* h_batches = nullptr;       // pinned
    int alpha_batch = 0;            // NUSI_OPT_ALPHA_BATCH: max tables per batch; 0 = auto
    int alpha_kind = 0;             // NUSI_OPT_ALPHA_KERNEL: 0 k_alpha_batch, 1 k_alpha_tile<G> (<= 4), 2 per entry
    int cascade_rhs = 0;            // NUSI_OPT_CASCADE_RHS: 0 = auto, 1 = one point per MFMA-cascade workgroup,
                                    // 2 = pairs, 3..16 = gamma batches of up to that many (k_cascade_bs_gamma)
    int* d_gidx = nullptr;          // gamma batches: the points of each batch, batch after batch
    int* h_gidx = nullptr;          // pinned
    int2* d_gbgrp = nullptr;        // ... per batch: first index into gidx, count
    int2* h_gbgrp = nullptr;        // pinned
    double* d_fh = nullptr;         // k_cascade_bs's F FIFO between step passes, cascade_bs_scratch_doubles per workgroup
    int step_passes = 0;            // NUSI_OPT_STEP_PASSES: 1 = the step-pass instance of k_cascade_bs also where one pass fits
    int shift_max = 0;              // NUSI_OPT_SHIFT_REUSE: K, the largest bin offset served by a base table set
    int ref_order = 1;              // NUSI_OPT_REFERENCE_ORDER: 1 (default) = the tables in the reference's own arithmetic,
                                    // 0 = the shared-algorithm order (opt-in fast mode)
    int cascade_sync = 0;           // NUSI_OPT_CASCADE_SYNC: 0 = auto, 2 = block-synchronous (the same kernel; 1 is refused)
    int corner_mb = 0;              // NUSI_OPT_REFO_CORNER_MB: the member-corner block's budget (0 = automatic)
    int ga_batch = 0;               // NUSI_OPT_GA_BATCH: 0 = auto, 1 = the per-table Gamma / alphaTilde kernel, 2 = the
                                    // batch path (k_ga_dilogs_batch) whenever batches exist
    int ga_pre_mb = 0;              // NUSI_OPT_GA_PRE_MB: the batch path's block budget (0 = kGaPreBudget)
    int ga_pre_kb = 0;              // NUSI_OPT_GA_PRE_KB: the same in KiB (> 0: it holds instead)
    size_t fh_doubles = 0;          // capacity of d_fh in doubles (the block-synchronous kernels' FIFOs)
    nusi_plan* shift = nullptr;     // ... its plan: the same grid with K more redshift steps (axis T + K)
    int2* d_smap = nullptr;         // per shifted table: base index in `shift`, bin offset
    int2* h_smap = nullptr;         // pinned
    AlphaBatches shift_batches;     // the base plan's alpha batches of the last call
    double* d_src = nullptr;        // source terms of the MFMA cascade's points that are not the power law
                                    // [src_cap][cascade_src_doubles] (k_source_dsnb, k_source_tab)
    int src_cap = 0;
    double* d_slots = nullptr;      // tabulated sources (nusi_plan_set_source): [slot_cap][cascade_slot_doubles], S then w
    int slot_cap = 0;
    std::vector<unsigned char> slot_set;   // [slot_cap]: the slot holds a source
    // nusi_plan_response (the impulse cascade) and nusi_plan_response_apply
    int response_fifo_kb = 0;       // NUSI_OPT_RESPONSE_FIFO_KB: the impulse cascade's FIFO budget (0 = kResponseFifoBytes)
    double* d_rw = nullptr;         // the call's redshift weights [Nz]
    std::vector<double> h_rw;
    double* d_rslots = nullptr;     // the scalar fallback's unit-vector slots [T + 1][cascade_slot_doubles] ...
    std::vector<double> h_rslots;
    nusi::Point* d_rpts = nullptr;  // ... its temporary point records of one chunk [kResponseChunk] ...
    double* d_rscr = nullptr;       // ... and a chunk's output where the caller passed NULL [kResponseChunk][3 N]
    double* d_app = nullptr;        // apply: the spectra S [Q][T + 1], then scale [Q]
    size_t app_doubles = 0;
    std::vector<double> h_app;
    hipEvent_t ev_app = nullptr;    // end of the latest apply (the next one reuses d_app / h_app)
    bool app_ran = false;
    double* d_kap = nullptr;        // compose: the mass fractions kappa [ntab][Qc][3]
    size_t kap_doubles = 0;
    std::vector<double> h_kap;
    hipEvent_t ev_cmp = nullptr;    // end of the latest compose (the next one reuses d_kap / h_kap)
    bool cmp_ran = false;
    // the detector (nusi_plan_set_detector) and its calls (fold, events)
    int det_C = 0;                  // reconstructed bins; 0 = no detector
    double* d_det = nullptr;        // Dt [3 N][detector_ld(C)] (K-major, zero-padded columns), then the background [C]
    int fit_K = 0;                  // background templates of the fit (nusi_plan_set_templates); 0 = none
    double* d_tpl = nullptr;        // T [K][C]
    double fit_m[NUSI_FIT_TEMPLATES_MAX] = {}, fit_w[NUSI_FIT_TEMPLATES_MAX] = {};   // the priors: means, 1 / sigma^2 (0 = none)
    double* d_evt = nullptr;        // events: the spectra S [Q][T + 1], then scale [Q], then data [C] (the ensemble: [P][C])
    size_t evt_doubles = 0;
    int ens_qslices = 0;            // NUSI_OPT_ENSEMBLE_QSLICES, NUSI_OPT_ENSEMBLE_PSLICES: 0 = automatic
    int ens_pslices = 0;
    void* d_ens = nullptr;          // the ensemble's q-slice records [qslices][P][ntab] (at most kEnsScratchBytes when
    size_t ens_bytes = 0;           // the slices are automatic)
    int toy_nuis = NUSI_TOYS_FIXED;   // NUSI_OPT_TOY_NUISANCE: the ensemble of inject's and belt's toys
    double fit_s[NUSI_FIT_TEMPLATES_MAX] = {};   // the priors' widths sigma where fit_w > 0, +inf elsewhere (the toys' normals)
    int toys_mb = 0, toys_b = 0;   // NUSI_OPT_ENSEMBLE_LIMIT_MB, _BYTES: the ensemble limit's scratch budget (0 = kToysScratchBytes)
    double* d_toys = nullptr;       // a chunk's limits per side kept here [units QB][P] (grown on demand)
    size_t toys_bytes = 0;
    int* d_rank = nullptr;          // the band's ranks [NUSI_BAND_RANKS_MAX], staged from h_rank
    int h_rank[NUSI_BAND_RANKS_MAX] = {};
    std::vector<double> h_evt;
    double* d_draw = nullptr;       // nusi_plan_draw_counts: the expectations mu [rows][C], staged from h_draw
    size_t draw_doubles = 0;
    std::vector<double> h_draw;
    hipEvent_t ev_draw = nullptr;   // end of the latest draw (the next one reuses d_draw / h_draw)
    bool draw_ran = false;
    hipEvent_t ev_det = nullptr;    // end of the latest fold / events call (set_detector and the next events wait for it)
    bool det_ran = false;
    std::vector<int> slot_of;       // table slot of each point of the last call
    int last_ntab = 0;
    int* d_warn = nullptr;
    // The per-call inputs in ONE device block and its pinned mirror, uploaded by ONE copy per call (a single
    // propagation paid a DMA blit of ~4 us per array, five of them, plus a fill for the warnings): sections
    // [warn | batches | gbgrp | gidx | pts | tpts], each sized for max_points (in_sections); the warnings are zeroed
    // on the host side of the copy
    char* d_in = nullptr;
    char* h_in = nullptr;      // pinned
    int* h_warn0 = nullptr;    // pinned: the warn section of h_in (zeros)
    size_t in_tpts = 0;        // byte offset of the tpts section (the copy runs up to its ntab-th Point)
    // evolve_host's output staging (pinned; the warnings, then flux / flux_fla; only for calls of at most
    // kStageBytes) and the warnings it fetched, for nusi_plan_warnings without a second round trip
    char* h_out = nullptr;
    size_t h_out_bytes = 0;
    std::vector<int> warn_host;
    bool warn_host_valid = false;
    nusi::TablesDev tabs{};
    nusi::AlphaTilesDev atiles{};
    nusi::MCornerDev mc{};         // NUSI_OPT_REFERENCE_ORDER: member corners of the big-batch kernel (mcorner_ensure)
    double* d_scratch = nullptr;   // flux outputs when the caller passes NULL
    double* d_kt = nullptr;        // the k-split alpha path's term buffer (TablesDev::Kt), kt_doubles doubles
    size_t kt_doubles = 0;
    double* d_gpre = nullptr;      // the reference order's Gamma / alphaTilde dilogarithms (TablesDev::Gpre)
    nusi::GaBatchDev gab{};        // ... per alpha batch, of scans (ga_batch_ensure, launch_gamma_alphat)
    const char* ga_kernel = "";    // the Gamma / alphaTilde path of the latest call (nusi_plan_ga_kernel)
    size_t gpre_doubles = 0;
    std::shared_ptr<SplineStore> spl;
    nusi::SplineSet* d_nospl = nullptr;   // an empty spline set in device memory (no phi-phi tables loaded)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_copy = nullptr;
    hipEvent_t ev_done = nullptr;      // end of the latest call's kernels (the next call waits for it)
    hipStream_t side = nullptr;        // Gamma / alphaTilde beside alpha in calls of few tables (kOverlapTables)
    hipEvent_t ev_fork = nullptr;
    bool ran = false;
    int last_n = 0;
    std::vector<hipEvent_t> prof_ev;   // 4 per recorded call
    hipEvent_t last_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // the latest call's stage events (handles)
    const char* alpha_kernel = "";     // main kernels of the latest call (nusi_plan_kernels)
    std::string alpha_label;           // ... storage of a composed alpha label (shift reuse)
    const char* cascade_kernel = "";
    int prof_max = 0, prof_n = 0;
    int cascade_kind = NUSI_CASCADE_AUTO;
    double U2[2][9];
    std::map<double, double> fs_cache;                      // si -> flux_FS_E0
    std::map<std::pair<double, int>, std::vector<double>> mass_cache;
};

namespace {

// the Point fields the Stage-A kernels read (nusi_physics.hpp gamma/alphat/alpha_entry)
using TableKey = std::array<double, 12>;
TableKey table_key(const nusi::Point& P)
{
    return TableKey{P.mphi, P.g, P.Ga, P.mn[0], P.mn[1], P.mn[2], P.u[0], P.u[1], P.u[2],
                    (double)P.majorana, (double)P.non_resonant, (double)P.phiphi};
}

int build_point(nusi_plan* pl, const nusi_params& p, nusi::Point& P)
{
    const HostGrid& G = pl->grid;
    if (p.N_bins_E != G.N || p.lEmin != G.lEmin || p.lEmax != G.lEmax || p.zmax != G.zmax_in)
        return fail(NUSI_EPARAM, "point grid (N_bins_E, lEmin, lEmax, zmax) differs from the plan's");
    if (p.flav < 0 || p.flav > 2) return fail(NUSI_EPARAM, "flav must be 0, 1 or 2");
    if (p.source_model < 0) return fail(NUSI_EPARAM, "unknown source_model");
    const bool tab = p.source_model >= NUSI_SOURCE_TABULATED;
    if (tab) {
        const long long slot = (long long)p.source_model - NUSI_SOURCE_TABULATED;
        if (slot >= (long long)pl->slot_set.size() || !pl->slot_set[(size_t)slot])
            return fail(NUSI_EPARAM, "source_model names a tabulated source slot that is empty (nusi_plan_set_source)");
    }
    const int no = p.normal_ordering ? 1 : 0;
    // masses, nuSIprop.hpp:184-203
    const double dmq21 = 7.42e-5;
    const double dmqAT = no ? 2.514e-3 : -2.497e-3;
    auto key = std::make_pair(p.mntot, no);
    auto it = pl->mass_cache.find(key);
    if (it == pl->mass_cache.end()) {
        double mL;
        if (!lightest_mass(p.mntot, dmq21, dmqAT, &mL)) {
            char buf[256];
            snprintf(buf, sizeof buf,
                     "No neutrino mass spectrum was found corresponding to \\sum m = %g, dmqAT = %g, dmqSL = %g. Exiting...",
                     p.mntot, dmqAT, dmq21);
            return fail(NUSI_ENOSPECTRUM, buf);
        }
        std::vector<double> mn(3);
        if (no) {
            mn[0] = mL;
            mn[1] = sqrt(dmq21 + sq(mL));
            mn[2] = sqrt(dmqAT + sq(mL));
        } else {
            mn[2] = mL;
            mn[1] = sqrt(sq(mL) - dmqAT);
            mn[0] = sqrt(sq(mn[1]) - dmq21);
        }
        it = pl->mass_cache.emplace(key, mn).first;
    }
    // a tabulated source's norm is absolute and its si unused: no free-streaming normalisation
    auto fit = pl->fs_cache.end();
    if (!tab) {
        fit = pl->fs_cache.find(p.si);
        if (fit == pl->fs_cache.end()) fit = pl->fs_cache.emplace(p.si, flux_fs_e0(p.si, G.zmax_eff)).first;
    }
    memset(&P, 0, sizeof(P));
    P.mphi = p.mphi;
    P.g = p.g;
    P.mntot = p.mntot;
    P.si = tab ? 0.0 : p.si;   // (only the power-law source reads it)
    P.norm = p.norm;
    P.norm_total = tab ? p.norm : p.norm / fit->second;
    P.Ga = p.majorana ? sq(p.g) * p.mphi / (16.0 * M_PI) : sq(p.g) * p.mphi / (8.0 * M_PI);
    for (int k = 0; k < 3; ++k) P.mn[k] = it->second[k];
    for (int k = 0; k < 9; ++k) P.U2[k] = pl->U2[no][k];
    for (int k = 0; k < 3; ++k) P.u[k] = pl->U2[no][3 * p.flav + k];
    P.majorana = p.majorana ? 1 : 0;
    P.non_resonant = p.non_resonant ? 1 : 0;
    P.phiphi = p.phiphi ? 1 : 0;
    P.source = p.source_model;
    nusi::point_derive(P);
    if (P.non_resonant && P.phiphi && !pl->spl)
        return fail(NUSI_ETABLE, "phiphi requested but the phi-phi tables are not loaded (nusi_plan_load_phiphi)");
    return NUSI_OK;
}


// Order the tables h_tpts[0, ntab) so that those sharing m_phi, the masses and the flags -- whose alpha tables
// share every leaf of (S', t) alone -- are neighbours (slots renumbered; perm[old] = new), and cut them into the
// batches h_batches.
AlphaBatches alpha_batches(nusi_plan* pl, int ntab, std::vector<int>& perm)
{
    AlphaBatches ab;
    std::vector<int> order(ntab);
    perm.assign(ntab, 0);
    for (int j = 0; j < ntab; ++j) order[j] = j;
    auto bkey = [&](int j) {
        const nusi::Point& P = pl->h_tpts[j];
        // phi-phi first: the tables with the channel come last (their batches run on their own launch)
        return std::make_tuple(P.phiphi && P.non_resonant, P.mphi, P.mn[0], P.mn[1], P.mn[2], P.majorana, P.non_resonant,
                               P.phiphi);
    };
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bkey(a) < bkey(b); });
    {
        std::vector<nusi::Point> tmp(pl->h_tpts, pl->h_tpts + ntab);
        for (int j = 0; j < ntab; ++j) {
            pl->h_tpts[j] = tmp[order[j]];
            perm[order[j]] = j;
        }
    }
    for (int j = 0; j < ntab; ++j) pl->h_tpts[j].tslot = j;
    // batch cap: the tile kernel's LDS holds <= 4 (3 measured best); the big-batch kernel shares the leaves of
    // any number, but one workgroup runs a batch's points one after the other, so the cap keeps ~2 rounds of
    // workgroups per CU slot (256 CUs x 3) in the grid: ntab x class-0 tiles / cap >= 1536
    int cap = pl->alpha_kind == 1 ? std::min(pl->alpha_batch, 4) : pl->alpha_batch;
    if (cap <= 0) {
        if (pl->alpha_kind == 1) cap = 3;
        else {
            const long long work = (long long)ntab * std::max(1, pl->atiles.ncls[0]);
            cap = (int)std::max(1LL, std::min(64LL, (work + 1535) / 1536));
        }
    }
    ab.cap = cap;
    for (int j = 0; j < ntab;) {
        int run = 1;   // the group of tables sharing bkey, split into near-equal batches of <= cap
        while (j + run < ntab && bkey(j + run) == bkey(j)) ++run;
        const int nb = (run + cap - 1) / cap;
        for (int b = 0; b < nb; ++b) {
            const int lo = j + (int)((long long)run * b / nb), hi = j + (int)((long long)run * (b + 1) / nb);
            pl->h_batches[ab.nbatch++] = lo | ((hi - lo) << 24);
        }
        j += run;
    }
    while (ab.nb_plain < ab.nbatch) {   // batches without the phi-phi channel (sorted first by bkey)
        const nusi::Point& F = pl->h_tpts[pl->h_batches[ab.nb_plain] & 0xffffff];
        if (F.phiphi && F.non_resonant) break;
        ++ab.nb_plain;
    }
    return ab;
}

// NUSI_OPT_REFERENCE_ORDER on the big-batch kernel: the member-corner block of plan p (MCornerDev) for the batches of
// this call -- 6 NC doubles per table (C4's N_E = 300 axis: NC = 77 421, 3.7 MB), allocated for at most
// NUSI_OPT_REFO_CORNER_MB (automatic: kMCornerBudget bytes and half the free memory) of tables, at least the largest
// batch; launch_alpha runs the batches in chunks that fit
constexpr size_t kMCornerBudget = size_t(8) << 30;
constexpr int kOverlapTables = 16;   // calls of at most this many tables overlap Gamma / alphaTilde with alpha
constexpr size_t kStageBytes = size_t(4) << 20;   // nusi_plan_evolve_host's pinned output staging, at most
constexpr int kSplitTables = 2;   // calls of at most this many tables (no phi-phi) run the k-split alpha path
// the plan's distinct bin edges in device memory (MCornerDev::eu, ue, ub), uploaded once by whoever needs them first:
// the member-corner block or the Gamma / alphaTilde batch path
int edges_ensure(nusi_plan* p)
{
    nusi::MCornerDev& mc = p->mc;
    if (mc.eu) return NUSI_OK;
    std::vector<int> eu, ub;
    std::vector<double> ue;
    nusi::mcorner_edges(p->grid.T, p->grid.lo.data(), p->grid.hi.data(), eu, ue);
    nusi::ga_batch_edge_bins(p->grid.T, eu, (int)ue.size(), ub);
    HIPCHECK(hipMalloc(&mc.ue, sizeof(double) * ue.size()));
    HIPCHECK(hipMemcpy(mc.ue, ue.data(), sizeof(double) * ue.size(), hipMemcpyHostToDevice));
    HIPCHECK(hipMalloc(&mc.ub, sizeof(int) * ub.size()));
    HIPCHECK(hipMemcpy(mc.ub, ub.data(), sizeof(int) * ub.size(), hipMemcpyHostToDevice));
    mc.U = (int)ue.size();
    mc.NC = (long long)mc.U * (mc.U + 1) / 2;
    HIPCHECK(hipMalloc(&mc.eu, sizeof(int) * eu.size()));   // (last: mc.eu marks the set complete)
    HIPCHECK(hipMemcpy(mc.eu, eu.data(), sizeof(int) * eu.size(), hipMemcpyHostToDevice));
    return NUSI_OK;
}

// The Gamma / alphaTilde batch path's block (GaBatchDev) for a call of ntab tables in nbatch batches: the whole call
// where that fits the budget (NUSI_OPT_GA_PRE_MB, or NUSI_OPT_GA_PRE_KB in KiB; default kGaPreBudget, C4 72 + 4 MB),
// else the budget and at least the largest batch -- launch_gamma_alphat then runs chunks of whole batches.  Grown
// on demand; an explicit budget also shrinks it, so that a test can hold it to a size.
constexpr size_t kGaPreBudget = size_t(512) << 20;
int ga_batch_ensure(nusi_plan* p, int ntab, int nbatch, int budget_mb, int budget_kb)
{
    if (int r = edges_ensure(p)) return r;
    nusi::GaBatchDev& gb = p->gab;
    const int T = p->grid.T, U = p->mc.U;
    int nbmax = 1;
    for (int b = 0; b < nbatch; ++b) nbmax = std::max(nbmax, (int)((unsigned)p->h_batches[b] >> 24));
    const bool set = budget_mb > 0 || budget_kb > 0;
    const size_t budget = budget_kb > 0 ? ((size_t)budget_kb << 10) : budget_mb > 0 ? ((size_t)budget_mb << 20) : kGaPreBudget;
    const size_t want = std::max(std::min(nusi::ga_batch_bytes(T, U, ntab, nbatch), budget), nusi::ga_batch_bytes(T, U, nbmax, 1));
    if (gb.bytes < want || (set && gb.bytes != want)) {
        hipFree(gb.buf);
        gb.buf = nullptr;
        gb.bytes = 0;
        HIPCHECK(hipMalloc(&gb.buf, want));
        gb.bytes = want;
    }
    gb.eu = p->mc.eu;
    gb.ue = p->mc.ue;
    gb.ub = p->mc.ub;
    gb.U = U;
    return NUSI_OK;
}

int mcorner_ensure(nusi_plan* p, int ntab, const AlphaBatches& ab, int budget_mb)
{
    nusi::MCornerDev& mc = p->mc;
    if (int r = edges_ensure(p)) return r;
    const size_t per = sizeof(double) * 6 * (size_t)mc.NC;
    if (mc.buf && budget_mb == 0 && mc.cap_tables >= ntab && per * mc.cap_tables <= kMCornerBudget)
        return NUSI_OK;   // every table of the call fits the block already (no hipMemGetInfo per call)
    int nbmax = 1;
    for (int b = 0; b < ab.nbatch; ++b) nbmax = std::max(nbmax, (int)((unsigned)p->h_batches[b] >> 24));
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = kMCornerBudget;
    const size_t budget = budget_mb > 0 ? ((size_t)budget_mb << 20)
                                        : std::min(kMCornerBudget, (fr + (mc.buf ? per * mc.cap_tables : 0)) / 2);
    const int want = std::max(nbmax, (int)std::min<size_t>((size_t)ntab, budget / per));
    if (mc.buf && mc.cap_tables >= want && (budget_mb == 0 || mc.cap_tables == want)) return NUSI_OK;
    hipFree(mc.buf);
    mc.buf = nullptr;
    mc.cap_tables = 0;
    HIPCHECK(hipMalloc(&mc.buf, per * want));
    mc.cap_tables = want;
    return NUSI_OK;
}

// NUSI_OPT_SHIFT_REUSE.  alpha / Gamma / alphaTilde see the energies only through
// 2 m_k E / m_phi^2 (nuSIprop.hpp:1253-1256) and g through g^4 and Gamma_phi / m_phi = g^2 / 16 pi, so the tables of
// m_phi' = m_phi r^(-o/2) (r = Emax[0] / Emin[0] = the table axis' bin ratio) are those of m_phi read o bins higher.
// Only tables with g <= kShiftReuseGMax = 0.05 take part (the optical depth amplifies the shifted tables' rounding
// with g); the others are built directly.  Tables of one (g, masses, |U|^2, flags) are taken in
// decreasing m_phi: each group starts at its largest m_phi (the base) and takes the following ones whose offset
// o = 2 ln(m_base / m_phi) / ln r is within |o - round(o)| ln(r) / 2 < 1e-13 of an integer (m_phi reproduced to
// ~1e-13 relative) in [1, K].  Groups of two or more go to slots [nd, ntab) in group order (remap[old slot] = new slot; smap[slot - nd]
// = (base index, o); bases[] = the base Points); the rest stay in [0, nd).  Returns nd.
int shift_groups(nusi_plan* pl, int ntab, std::vector<int>& remap, std::vector<int2>& smap, std::vector<nusi::Point>& bases)
{
    const double lr = log(pl->grid.Emax[0] / pl->grid.Emin[0]);
    const int K = pl->shift_max;
    const nusi::Point* tp = pl->h_tpts;
    auto gkey = [&](int j) {
        const nusi::Point& P = tp[j];
        return std::make_tuple(P.g, P.mn[0], P.mn[1], P.mn[2], P.u[0], P.u[1], P.u[2], P.majorana, P.non_resonant,
                               P.phiphi);
    };
    // only couplings up to kShiftReuseGMax share: the shifted tables differ from a point's own by rounding, and the
    // flux's optical depth amplifies that with the coupling (scripts/dev_shift_reuse_errors.py on the GPU, vs each
    // point's own evolution: c4s lattice <= 1.7e-11 for g <= 0.044, 6.4e-10 at 0.135, 3e-8 at g = 1; N_E = 850,
    // m_phi = 3e7: 8.8e-10 at g = 0.05, 1.4e-8 at 0.1; the north star bounds fluxes at 1e-9)
    constexpr double kShiftReuseGMax = 0.05;
    std::vector<int> idx;
    for (int j = 0; j < ntab; ++j)
        if (tp[j].g <= kShiftReuseGMax) idx.push_back(j);
    const int nsh = (int)idx.size();
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
        const auto ka = gkey(a), kb = gkey(b);
        return ka != kb ? ka < kb : tp[a].mphi > tp[b].mphi;
    });
    std::vector<int> grp(ntab, -1), off(ntab, 0);
    std::vector<std::vector<int>> members;
    for (int a = 0; a < nsh;) {
        int b = a + 1;
        while (b < nsh && gkey(idx[b]) == gkey(idx[a])) ++b;
        std::vector<int> cur{idx[a]};
        int last = 0;
        for (int c = a + 1; c <= b; ++c) {
            bool join = false;
            int o = 0;
            if (c < b) {
                const double kf = 2.0 * log(tp[cur[0]].mphi / tp[idx[c]].mphi) / lr;
                o = (int)lround(kf);
                // the lattice m_phi must reproduce the point's own to a few ulp: m_base r^(-o/2) differs from it by
                // |kf - o| ln(r) / 2 relative, and the cascade sees only the tables (1e-6 in o let a
                // point 2e-8 off the lattice take the tables of a slightly different m_phi)
                join = o > last && o <= K && fabs(kf - o) * lr * 0.5 < 1e-13;
            }
            if (join) {
                cur.push_back(idx[c]);
                off[idx[c]] = last = o;
                continue;
            }
            if (cur.size() >= 2) {
                for (int m : cur) grp[m] = (int)members.size();
                members.push_back(cur);
            }
            if (c < b) {
                cur.assign(1, idx[c]);
                off[idx[c]] = last = 0;
            }
        }
        a = b;
    }
    remap.assign(ntab, 0);
    int nd = 0;
    for (int j = 0; j < ntab; ++j)
        if (grp[j] < 0) remap[j] = nd++;
    int s = nd;
    smap.clear();
    bases.clear();
    for (size_t g = 0; g < members.size(); ++g) {
        bases.push_back(tp[members[g][0]]);
        for (int m : members[g]) {
            remap[m] = s++;
            smap.push_back(make_int2((int)g, off[m]));
        }
    }
    return nd;
}

// the base plan of NUSI_OPT_SHIFT_REUSE: the plan's grid with K more redshift steps, so that its table axis is
// the plan's, bit for bit, extended by K bins on top (nuSIprop.hpp:224-233: bins >= N are Emin/Emax[N-1] (1 + z));
// sized for the call's nbase base tables (grown on demand, at most max_points / 2: a base serves >= 2 tables), with
// the per-row warning records (TablesDev::Wmin) that k_table_shift reads
int ensure_shift_plan(nusi_plan* pl, int nbase)
{
    const int K = pl->shift_max;
    if (pl->shift && pl->shift->grid.T == pl->grid.T + K && pl->shift->max_points >= nbase) return NUSI_OK;
    int cap = nbase;
    if (pl->shift) {
        cap = std::max(nbase, std::min(2 * pl->shift->max_points, std::max(1, pl->max_points / 2)));
        if (pl->ran) {   // the previous call's kernels read the old base tables
            HIPCHECK(hipSetDevice(pl->device));
            HIPCHECK(hipEventSynchronize(pl->ev_done));
        }
        nusi_plan_destroy(pl->shift);
        pl->shift = nullptr;
    }
    const HostGrid& G = pl->grid;
    const double r = G.Emax[0] / G.Emin[0];
    const double zb = pow(r, G.Nz + K - 1.5) - 1;   // N_steps_z = (int)(ln(1 + zb) / ln r + 2) = Nz + K
    nusi_plan* sp = nullptr;
    int rc = nusi_plan_create(pl->device, G.N, G.lEmin, G.lEmax, zb, std::max(1, cap), &sp);
    if (rc) return rc;
    const HostGrid& B = sp->grid;
    bool same = B.T == G.T + K;
    for (int n = 0; same && n < G.T; ++n) same = B.lo[n] == G.lo[n] && B.hi[n] == G.hi[n];
    if (!same) {
        nusi_plan_destroy(sp);
        return fail(NUSI_EPARAM, "shift reuse: the extended axis does not match the plan's below T");
    }
    sp->alpha_batch = pl->alpha_batch;
    sp->alpha_kind = pl->alpha_kind;
    sp->spl = pl->spl;
    HIPCHECK(hipSetDevice(pl->device));
    if (hipMalloc(&sp->tabs.Wmin, sizeof(int) * 4 * (size_t)B.T * sp->max_points) != hipSuccess) {
        nusi_plan_destroy(sp);
        return fail(NUSI_EHIP, "shift reuse: no device memory for the base plan's warning records");
    }
    if (!pl->d_smap) {
        HIPCHECK(hipMalloc(&pl->d_smap, sizeof(int2) * pl->max_points));
        HIPCHECK(hipHostMalloc((void**)&pl->h_smap, sizeof(int2) * pl->max_points, hipHostMallocDefault));
    }
    pl->shift = sp;
    return NUSI_OK;
}
}  // namespace

extern "C" {

const char* nusi_last_error(void) { return g_err.c_str(); }

int nusi_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void nusi_params_default(nusi_params* p, double mphi, double g, double mntot, double si)
{
    p->mphi = mphi;
    p->g = g;
    p->mntot = mntot;
    p->si = si;
    p->norm = 1;
    p->majorana = 1;
    p->non_resonant = 1;
    p->normal_ordering = 1;
    p->N_bins_E = 300;
    p->lEmin = 12.0;
    p->lEmax = 17.0;
    p->zmax = 5.0;
    p->flav = 2;
    p->phiphi = 0;
    p->source_model = NUSI_SOURCE_DSNB;
}

void nusi_plan_destroy(nusi_plan* pl)
{
    if (!pl) return;
    int prev = 0;
    hipGetDevice(&prev);
    hipSetDevice(pl->device);
    if (pl->stream) hipStreamSynchronize(pl->stream);
    for (auto& e : pl->ev)
        if (e) hipEventDestroy(e);
    if (pl->ev_copy) hipEventDestroy(pl->ev_copy);
    if (pl->ev_done) hipEventDestroy(pl->ev_done);
    if (pl->ev_fork) hipEventDestroy(pl->ev_fork);
    if (pl->side) hipStreamDestroy(pl->side);
    for (auto& e : pl->prof_ev) hipEventDestroy(e);
    hipFree(pl->d_grid);
    hipFree(pl->d_in);   // (d_pts, d_tpts, d_batches, d_warn, d_gidx, d_gbgrp and their pinned mirrors live in it)
    if (pl->h_in) hipHostFree(pl->h_in);
    if (pl->h_out) hipHostFree(pl->h_out);
    hipFree(pl->tabs.G);
    hipFree(pl->tabs.At);
    hipFree(pl->tabs.A);
    hipFree(pl->tabs.Med);
    hipFree(pl->tabs.Wmin);
    hipFree(pl->d_nospl);
    hipFree(pl->d_src);
    hipFree(pl->d_slots);
    hipFree(pl->d_smap);
    if (pl->h_smap) hipHostFree(pl->h_smap);
    hipFree(pl->d_fh);
    if (pl->ev_app) hipEventDestroy(pl->ev_app);
    if (pl->ev_cmp) hipEventDestroy(pl->ev_cmp);
    hipFree(pl->d_kap);
    hipFree(pl->d_rw);
    hipFree(pl->d_rslots);
    hipFree(pl->d_rpts);
    hipFree(pl->d_rscr);
    hipFree(pl->d_app);
    if (pl->ev_det) hipEventDestroy(pl->ev_det);
    hipFree(pl->d_det);
    hipFree(pl->d_tpl);
    hipFree(pl->d_evt);
    hipFree(pl->d_ens);
    hipFree(pl->d_toys);
    hipFree(pl->d_rank);
    if (pl->ev_draw) hipEventDestroy(pl->ev_draw);
    hipFree(pl->d_draw);
    nusi::alpha_tiles_destroy(&pl->atiles);
    hipFree(pl->mc.buf);
    hipFree(pl->mc.eu);
    hipFree(pl->mc.ue);
    hipFree(pl->mc.ub);
    hipFree(pl->gab.buf);
    hipFree(pl->d_scratch);
    hipFree(pl->d_kt);
    hipFree(pl->d_gpre);
    if (pl->stream) hipStreamDestroy(pl->stream);
    pl->spl.reset();
    nusi_plan* sh = pl->shift;
    hipSetDevice(prev);
    delete pl;
    nusi_plan_destroy(sh);
}

int nusi_plan_create(int device, int N_bins_E, double lEmin, double lEmax, double zmax, int max_points, nusi_plan** out)
{
    *out = nullptr;
    if (N_bins_E < 2 || !(lEmax > lEmin) || !(zmax > 0) || max_points < 1)
        return fail(NUSI_EPARAM, "bad grid: need N_bins_E >= 2, lEmax > lEmin, zmax > 0, max_points >= 1");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(NUSI_EHIP, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(NUSI_EPARAM, "device index out of range");
    HIPCHECK(hipSetDevice(device));
    std::unique_ptr<nusi_plan, void (*)(nusi_plan*)> pl(new nusi_plan, nusi_plan_destroy);
    pl->device = device;
    pl->grid = make_grid(N_bins_E, lEmin, lEmax, zmax);
    pl->max_points = max_points;
    pmns_sq(true, pl->U2[1]);
    pmns_sq(false, pl->U2[0]);
    const HostGrid& G = pl->grid;
    if (G.Nz < 2) return fail(NUSI_EPARAM, "redshift grid has fewer than two steps");
    HIPCHECK(hipStreamCreateWithFlags(&pl->stream, hipStreamNonBlocking));
    for (auto& e : pl->ev) HIPCHECK(hipEventCreate(&e));
    HIPCHECK(hipEventCreateWithFlags(&pl->ev_copy, hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&pl->ev_done, hipEventDisableTiming));
    HIPCHECK(hipStreamCreateWithFlags(&pl->side, hipStreamNonBlocking));
    HIPCHECK(hipEventCreateWithFlags(&pl->ev_fork, hipEventDisableTiming));
    // grid arrays in one allocation
    const size_t ng = 2 * (size_t)G.N + 2 * (size_t)G.T + 4 * (size_t)G.Nz;
    HIPCHECK(hipMalloc(&pl->d_grid, sizeof(double) * ng));
    std::vector<double> hg;
    hg.reserve(ng);
    hg.insert(hg.end(), G.Emin.begin(), G.Emin.end());
    hg.insert(hg.end(), G.Emax.begin(), G.Emax.end());
    hg.insert(hg.end(), G.lo.begin(), G.lo.end());
    hg.insert(hg.end(), G.hi.begin(), G.hi.end());
    hg.insert(hg.end(), G.z.begin(), G.z.end());
    hg.insert(hg.end(), G.step_c.begin(), G.step_c.end());
    hg.insert(hg.end(), G.step_s.begin(), G.step_s.end());
    hg.insert(hg.end(), G.sfr.begin(), G.sfr.end());
    HIPCHECK(hipMemcpy(pl->d_grid, hg.data(), sizeof(double) * ng, hipMemcpyHostToDevice));
    nusi::GridDev& gd = pl->gd;
    gd.N = G.N;
    gd.Nz = G.Nz;
    gd.T = G.T;
    gd.PT = (long long)G.T * (G.T - 1) / 2;
    double* q = pl->d_grid;
    gd.Emin = q;
    q += G.N;
    gd.Emax = q;
    q += G.N;
    gd.lo = q;
    q += G.T;
    gd.hi = q;
    q += G.T;
    gd.z = q;
    q += G.Nz;
    gd.step_c = q;
    q += G.Nz;
    gd.step_s = q;
    q += G.Nz;
    gd.sfr = q;
    {   // the per-call input block (nusi_plan::d_in)
        const size_t mp = (size_t)max_points;
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t o_warn = 0, o_bat = al(o_warn + sizeof(int) * mp), o_grp = al(o_bat + sizeof(int) * mp);
        const size_t o_gidx = al(o_grp + sizeof(int2) * mp), o_pts = al(o_gidx + sizeof(int) * mp);
        const size_t o_tpts = al(o_pts + sizeof(nusi::Point) * mp), tot = o_tpts + sizeof(nusi::Point) * mp;
        HIPCHECK(hipMalloc(&pl->d_in, tot));
        HIPCHECK(hipHostMalloc((void**)&pl->h_in, tot, hipHostMallocDefault));
        memset(pl->h_in, 0, tot);
        pl->d_warn = (int*)(pl->d_in + o_warn);
        pl->h_warn0 = (int*)(pl->h_in + o_warn);
        pl->d_batches = (int*)(pl->d_in + o_bat);
        pl->h_batches = (int*)(pl->h_in + o_bat);
        pl->d_gbgrp = (int2*)(pl->d_in + o_grp);
        pl->h_gbgrp = (int2*)(pl->h_in + o_grp);
        pl->d_gidx = (int*)(pl->d_in + o_gidx);
        pl->h_gidx = (int*)(pl->h_in + o_gidx);
        pl->d_pts = (nusi::Point*)(pl->d_in + o_pts);
        pl->h_pts = (nusi::Point*)(pl->h_in + o_pts);
        pl->d_tpts = (nusi::Point*)(pl->d_in + o_tpts);
        pl->h_tpts = (nusi::Point*)(pl->h_in + o_tpts);
        pl->in_tpts = o_tpts;
    }
    HIPCHECK(hipMalloc(&pl->tabs.G, sizeof(double) * (size_t)G.T * max_points));
    HIPCHECK(hipMalloc(&pl->tabs.At, sizeof(double) * (size_t)G.T * max_points));
    HIPCHECK(hipMalloc(&pl->tabs.A, sizeof(double) * (size_t)gd.PT * max_points));
    HIPCHECK(hipMalloc(&pl->tabs.Med, sizeof(double) * 3 * nusi::kMedFields * (size_t)G.T * max_points));
    {   // the empty spline set of plans without phi-phi tables (device memory, like SplineStore::d_set)
        const nusi::SplineSet none{};
        HIPCHECK(hipMalloc(&pl->d_nospl, sizeof(nusi::SplineSet)));
        HIPCHECK(hipMemcpy(pl->d_nospl, &none, sizeof(nusi::SplineSet), hipMemcpyHostToDevice));
    }
    std::vector<unsigned char> shared(G.T, 0);   // bin edges shared bitwise with the next bin
    for (int n = 0; n + 1 < G.T; ++n) shared[n] = (G.hi[n] == G.lo[n + 1]);
    HIPCHECK(nusi::alpha_tiles_create(G.T, shared.data(), &pl->atiles));
    *out = pl.release();
    return NUSI_OK;
}

// Loaded table sets are shared by every plan / object on the same device that loads the same files
// (path, dims, size and mtime): the reference reads the tables in every constructor
// (nuSIprop.hpp:166-170); here a set costs 400 MB + its 6.4 GB of windows in HBM, so a second
// calculate_flux object reuses the first one's while it is alive.
int nusi_plan_load_phiphi(nusi_plan* pl, const char* at_path, const int* at_dims, const char* a_path, const int* a_dims)
{
    static const int def2[2] = {5000, 100}, def3[3] = {1000, 1000, 100};
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    if (!at_path || !a_path) return fail(NUSI_EPARAM, "phi-phi table path is NULL");
    HIPCHECK(hipSetDevice(pl->device));
    const int* d2 = at_dims ? at_dims : def2;
    const int* d3 = a_dims ? a_dims : def3;
    const std::string key = std::to_string(pl->device) + "|" + file_stamp(at_path) + "|" + std::to_string(d2[0]) + "x" +
                            std::to_string(d2[1]) + "|" + file_stamp(a_path) + "|" + std::to_string(d3[0]) + "x" +
                            std::to_string(d3[1]) + "x" + std::to_string(d3[2]);
    std::shared_ptr<SplineSlot> slot;
    {
        std::lock_guard<std::mutex> lock(g_spl_mu);
        auto& e = g_spl_cache[key];
        if (!e) e = std::make_shared<SplineSlot>();
        slot = e;
    }
    std::lock_guard<std::mutex> lock(slot->mu);
    if (auto hit = slot->set.lock()) {
        pl->spl = hit;
        return NUSI_OK;
    }
    auto st = std::make_shared<SplineStore>();
    st->device = pl->device;
    int r = load_spline(at_path, 2, d2, *st, st->set.at);
    if (r) return r;
    r = load_spline(a_path, 3, d3, *st, st->set.a);
    if (r) return r;
    HIPCHECK(hipMalloc(&st->d_set, sizeof(nusi::SplineSet)));
    st->bufs.push_back(st->d_set);
    HIPCHECK(hipMemcpy(st->d_set, &st->set, sizeof(nusi::SplineSet), hipMemcpyHostToDevice));
    slot->set = st;
    pl->spl = st;
    return NUSI_OK;
}

int nusi_plan_grid(const nusi_plan* pl, int* N, int* Nz, double* Enu)
{
    if (N) *N = pl->grid.N;
    if (Nz) *Nz = pl->grid.Nz;
    if (Enu) memcpy(Enu, pl->grid.Enu.data(), sizeof(double) * pl->grid.N);
    return NUSI_OK;
}

// The source axis: the table axis of make_grid continued by one bin (a bin b <= N - 1 at step i <= Nz - 1 reads
// source-axis bin b + i <= T).
int nusi_plan_source_axis(const nusi_plan* pl, int* M, double* lo, double* hi, double* z)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    const HostGrid& G = pl->grid;
    if (M) *M = G.T + 1;
    if (lo) {
        memcpy(lo, G.lo.data(), sizeof(double) * G.T);
        lo[G.T] = G.Emin[G.N - 1] * (1 + G.z[G.Nz - 1]);
    }
    if (hi) {
        memcpy(hi, G.hi.data(), sizeof(double) * G.T);
        hi[G.T] = G.Emax[G.N - 1] * (1 + G.z[G.Nz - 1]);
    }
    if (z) memcpy(z, G.z.data(), sizeof(double) * G.Nz);
    return NUSI_OK;
}

int nusi_plan_set_source(nusi_plan* pl, int slot, const double* S, const double* w)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    if (slot < 0 || slot >= NUSI_SOURCE_SLOTS_MAX) return fail(NUSI_EPARAM, "source slot outside [0, NUSI_SOURCE_SLOTS_MAX)");
    if (!S) {   // clear (the storage stays; build_point refuses the slot)
        if ((size_t)slot < pl->slot_set.size()) pl->slot_set[(size_t)slot] = 0;
        return NUSI_OK;
    }
    const HostGrid& G = pl->grid;
    const int M = G.T + 1;
    for (int n = 0; n < M; ++n)
        if (!(S[n] >= 0.0) || !std::isfinite(S[n])) return fail(NUSI_EPARAM, "source spectrum: a bin integral is negative or not finite");
    if (w)
        for (int i = 0; i < G.Nz; ++i)
            if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(NUSI_EPARAM, "source redshift weight: an entry is negative or not finite");
    HIPCHECK(hipSetDevice(pl->device));
    // ordered with the plan's calls: the earlier ones (on whatever stream they ran) finish with the old contents,
    // and the copies below are complete when this returns
    if (pl->ran) HIPCHECK(hipEventSynchronize(pl->ev_done));
    const size_t per = nusi::cascade_slot_doubles(pl->gd);
    if (slot >= pl->slot_cap) {   // grow: doubled, at least 16 and the slot asked for
        const int cap = std::min(NUSI_SOURCE_SLOTS_MAX, std::max({16, 2 * pl->slot_cap, slot + 1}));
        double* d = nullptr;
        HIPCHECK(hipMalloc(&d, sizeof(double) * per * cap));
        if (pl->slot_cap) {
            const hipError_t e = hipMemcpy(d, pl->d_slots, sizeof(double) * per * pl->slot_cap, hipMemcpyDeviceToDevice);
            if (e != hipSuccess) {
                hipFree(d);
                HIPCHECK(e);
            }
        }
        hipFree(pl->d_slots);
        pl->d_slots = d;
        pl->slot_cap = cap;
        pl->slot_set.resize((size_t)cap, 0);
    }
    pl->slot_set[(size_t)slot] = 0;   // (empty if a copy fails half way)
    std::vector<double> v(per);
    memcpy(v.data(), S, sizeof(double) * M);
    memcpy(v.data() + M, w ? w : G.sfr.data(), sizeof(double) * G.Nz);
    HIPCHECK(hipMemcpy(pl->d_slots + per * (size_t)slot, v.data(), sizeof(double) * per, hipMemcpyHostToDevice));
    pl->slot_set[(size_t)slot] = 1;
    return NUSI_OK;
}

// nusi_plan_response's part of a call (plan_run): the redshift weights (validated; NULL = get_SFR)
struct ResponseCall {
    const double* w;
    bool mass;   // nusi_plan_response_mass: the response resolved by the source's mass state, G3[p][j][n][3][N]
};
static int response_prepare(nusi_plan* pl, const ResponseCall& rc, int n, hipStream_t s);
static int response_cascade(nusi_plan* pl, int n, bool all_nr, bool mass, double* d_G, double* d_G_fla, hipStream_t s);

// One call of a plan: Stage A for the points' distinct tables (deduplication, batches, every NUSI_OPT_*), then the
// cascade -- the points' own sources into d_flux / d_fla (nusi_plan_evolve; rc == nullptr), or the impulse cascade
// of every point's response matrix (nusi_plan_response; d_flux / d_fla are then G / G_fla and may stay NULL).
static int plan_run(nusi_plan* pl, const nusi_params* pts, int n, double* d_flux, double* d_fla, void* stream,
                    const ResponseCall* rc)
{
    if (n < 1 || n > pl->max_points) return fail(NUSI_EPARAM, "number of points outside [1, max_points]");
    HIPCHECK(hipSetDevice(pl->device));
    pl->warn_host_valid = false;
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    if (pl->ran) {
        HIPCHECK(hipEventSynchronize(pl->ev_copy));          // the pinned h_pts / h_tpts / h_batches are reused
        HIPCHECK(hipStreamWaitEvent(s, pl->ev_done, 0));     // so are d_pts, the tables and the warnings: one plan
    }                                                        // serialises its calls, whatever streams they use
    for (int i = 0; i < n; ++i) {
        nusi_params q = pts[i];
        if (rc) {   // a response ignores the point's source: si, norm and source_model (the table key reads none)
            q.source_model = NUSI_SOURCE_POWER_LAW;
            q.si = 2.0;
            q.norm = 1.0;
        }
        const int r = build_point(pl, q, pl->h_pts[i]);
        if (r) return r;
    }
    // one Stage-A table per distinct (mphi, g, Gamma_phi, masses, |U|^2, flags): the tables do not
    // depend on si, norm or the source (nuSIprop.hpp:217-253), so e.g. a gamma scan shares them
    std::map<TableKey, int> slots;
    pl->slot_of.resize(n);
    int ntab = 0;
    for (int i = 0; i < n; ++i) {
        nusi::Point& P = pl->h_pts[i];
        const TableKey key = table_key(P);
        auto it = slots.find(key);
        if (it == slots.end()) {
            it = slots.emplace(key, ntab).first;
            pl->h_tpts[ntab++] = P;
        }
        P.tslot = it->second;
        pl->slot_of[i] = it->second;
    }
    // NUSI_OPT_SHIFT_REUSE (opt-in): the tables a shifted base set serves go to the slots
    // [nd, ntab) (filled by k_table_shift), the others are built directly in [0, nd)
    int nd = ntab, nbase = 0;
    if (pl->shift_max > 0) {
        std::vector<int> remap;
        std::vector<nusi::Point> bases;
        std::vector<int2> smap;
        nd = shift_groups(pl, ntab, remap, smap, bases);
        nbase = (int)bases.size();
        if (nbase) {
            const int r = ensure_shift_plan(pl, nbase);
            if (r) return r;
            if (nbase > pl->shift->max_points) return fail(NUSI_EPARAM, "shift reuse: more base tables than the base plan holds");
            std::vector<nusi::Point> tmp(pl->h_tpts, pl->h_tpts + ntab);
            for (int j = 0; j < ntab; ++j) pl->h_tpts[remap[j]] = tmp[j];
            for (int j = 0; j < ntab; ++j) pl->h_tpts[j].tslot = j;
            for (int i = 0; i < n; ++i) pl->h_pts[i].tslot = pl->slot_of[i] = remap[pl->slot_of[i]];
            // the base plan's tables, ordered and batched like any others (their slots move: remap the map)
            nusi_plan* sp = pl->shift;
            sp->spl = pl->spl;   // (the phi-phi set may have been loaded after the base plan was made)
            sp->alpha_batch = pl->alpha_batch;   // (and the alpha options may have changed since)
            sp->alpha_kind = pl->alpha_kind;
            if (sp->ran) HIPCHECK(hipEventSynchronize(sp->ev_copy));
            for (int b = 0; b < nbase; ++b) {
                sp->h_tpts[b] = bases[b];
                sp->h_tpts[b].tslot = b;
            }
            std::vector<int> bperm;
            const AlphaBatches bb = alpha_batches(sp, nbase, bperm);
            for (int q = 0; q < ntab - nd; ++q) pl->h_smap[q] = make_int2(bperm[smap[q].x], smap[q].y);
            pl->shift_batches = bb;
        }
        if (!nbase) nd = ntab;
    }
    // the directly built tables, ordered so that those sharing m_phi, the masses and the flags -- whose alpha
    // tables share every leaf of (S', t) alone -- are neighbours, and cut into batches
    std::vector<int> perm;
    const AlphaBatches ab = alpha_batches(pl, nd, perm);
    for (int i = 0; i < n; ++i)
        if (pl->slot_of[i] < nd) pl->h_pts[i].tslot = pl->slot_of[i] = perm[pl->slot_of[i]];
    const int cap = ab.cap, nbatch = ab.nbatch, nb_plain = ab.nb_plain;
    const size_t N3 = (size_t)3 * pl->grid.N;
    if (!rc && (!d_flux || !d_fla)) {
        if (!pl->d_scratch) HIPCHECK(hipMalloc(&pl->d_scratch, sizeof(double) * 2 * N3 * pl->max_points));
        if (!d_flux) d_flux = pl->d_scratch;
        if (!d_fla) d_fla = pl->d_scratch + N3 * pl->max_points;
    }
    // the cascade.  AUTO / MFMA: the block-synchronous MFMA cascade k_cascade_bs for every point kind -- the points of
    // a table slot in workgroups of up to 16 (>= 3 points: the gamma batch), pairs, or one per workgroup
    // (NUSI_OPT_CASCADE_RHS caps the group size; NUSI_OPT_STEP_PASSES = 1: one point per workgroup on the
    // step-pass instance), any source and scattering mode, step passes on long grids.  WAVEFRONT / REG / LDS, and a
    // grid k_cascade_bs does not fit: the bit-exact scalar cascade k_cascade.
    const int kind = pl->cascade_kind == NUSI_CASCADE_AUTO ? NUSI_CASCADE_MFMA : pl->cascade_kind;
    // (every point that is not the power law reads its source from tabs.Src: the DSNB's from k_source_dsnb, the
    // tabulated ones' from k_source_tab)
    bool any_dsnb = false, any_tab = false, all_nr = true;
    for (int i = 0; i < n; ++i) {
        any_dsnb = any_dsnb || pl->h_pts[i].source == NUSI_SOURCE_DSNB;
        any_tab = any_tab || pl->h_pts[i].source >= NUSI_SOURCE_TABULATED;
        all_nr = all_nr && pl->h_pts[i].non_resonant;
    }
    const bool force_passes = pl->step_passes == 1;
    const bool bs = kind == NUSI_CASCADE_MFMA && nusi::cascade_bs_config(pl->gd, 1, force_passes) != 0;
    int ngb = 0, ngidx = 0;
    int bs_nwg[3] = {0, 0, 0};   // workgroups of P = 16, 2, 1 (their groups in h_gbgrp in that order)
    if (rc) {   // (the impulse cascade's own buffers; it groups source-axis bins, not points)
        if (int r = response_prepare(pl, *rc, n, s)) return r;
    } else if (bs) {
        const int rmax = force_passes ? 1 : pl->cascade_rhs == 0 ? 16 : pl->cascade_rhs;
        const bool g16 = rmax >= 3 && nusi::cascade_bs_config(pl->gd, 16, false) != 0;
        const bool g2 = rmax >= 2 && nusi::cascade_bs_config(pl->gd, 2, false) != 0;
        std::vector<std::vector<int>> by(ntab);
        for (int i = 0; i < n; ++i) by[pl->h_pts[i].tslot].push_back(i);
        std::vector<std::vector<int>> grs[3];   // groups for P = 16, 2, 1
        for (int j = 0; j < ntab; ++j) {
            const int c = (int)by[j].size();
            const int cap = (g16 && c >= 3) ? std::min(rmax, 16) : (g2 && c >= 2) ? 2 : 1;
            const int nb = (c + cap - 1) / cap;   // near-equal groups
            for (int k = 0; k < nb; ++k) {
                const int lo = (int)((long long)c * k / nb), hi = (int)((long long)c * (k + 1) / nb);
                const int sz = hi - lo, w = sz >= 3 ? 0 : sz == 2 ? 1 : 2;
                grs[w].emplace_back(by[j].begin() + lo, by[j].begin() + hi);
            }
        }
        size_t fhd = 0;
        const int Pk[3] = {16, 2, 1};
        for (int w = 0; w < 3; ++w) {
            for (const auto& gp : grs[w]) {
                pl->h_gbgrp[ngb++] = make_int2(ngidx, (int)gp.size());
                for (int i : gp) pl->h_gidx[ngidx++] = i;
            }
            bs_nwg[w] = (int)grs[w].size();
            fhd += nusi::cascade_bs_scratch_doubles(pl->gd, Pk[w]) * grs[w].size();
        }
        if (fhd > pl->fh_doubles) {
            hipFree(pl->d_fh);
            pl->d_fh = nullptr;
            pl->fh_doubles = 0;
            HIPCHECK(hipMalloc(&pl->d_fh, sizeof(double) * fhd));
            pl->fh_doubles = fhd;
        }
    }
    if (bs && (any_dsnb || any_tab) && pl->src_cap < pl->max_points) {
        hipFree(pl->d_src);
        pl->d_src = nullptr;
        pl->src_cap = 0;
        HIPCHECK(hipMalloc(&pl->d_src, sizeof(double) * nusi::cascade_src_doubles(pl->gd) * pl->max_points));
        pl->src_cap = pl->max_points;
        pl->tabs.Src = pl->d_src;
    }
    // NUSI_OPT_REFERENCE_ORDER on the big-batch kernel: the member-corner blocks sized (allocations, the edge maps'
    // synchronous upload) before the first event of the call and before any fork to the side stream
    const bool refo = pl->ref_order != 0;
    const bool mcorn = refo && pl->alpha_kind == 0;
    if (mcorn && nd && nbatch) {
        AlphaBatches ab;
        ab.nbatch = nbatch;
        if (int r = mcorner_ensure(pl, nd, ab, pl->corner_mb)) return r;
    }
    if (mcorn && nbase && pl->shift_batches.nbatch)
        if (int r = mcorner_ensure(pl->shift, nbase, pl->shift_batches, pl->corner_mb)) return r;
    // a call of few tables without the phi-phi channel: the k-split alpha path (TablesDev::Kt, 8 doubles per entry,
    // mass state and table; 11.5 MB per table at N_E = 300); scans keep the k loop inside the workgroup
    pl->tabs.Kt = nullptr;
    if (nbase == 0 && nd > 0 && nd <= kSplitTables && nb_plain == nbatch && pl->alpha_kind == 0) {
        const size_t need = (size_t)8 * 3 * (size_t)pl->gd.PT * nd;
        if (pl->kt_doubles < need) {
            hipFree(pl->d_kt);
            pl->d_kt = nullptr;
            pl->kt_doubles = 0;
            HIPCHECK(hipMalloc(&pl->d_kt, sizeof(double) * need));
            pl->kt_doubles = need;
        }
        pl->tabs.Kt = pl->d_kt;
    }
    // a call of few tables in the reference order: Gamma / alphaTilde's GSL dilogarithms one per work-item first
    // (k_ga_dilogs; 2.2 MB per table at N_E = 300).  The one place "few" is decided: launch_gamma_alphat follows Gpre
    // Scans in the reference order with batches formed: the dilogarithms per alpha batch instead (k_ga_dilogs_batch;
    // NUSI_OPT_GA_BATCH).  Automatic: every call of more than kOverlapTables tables, whatever its batches' sizes -- 32
    // m_phi x {1, 2, 3, 4, 8, 32} couplings at N_E = 300 all measured faster than the per-table kernel, batches of
    // one table included (0.31 -> 0.17 ms).  The shift-reuse base plan keeps the per-table kernel.
    const bool ga_batch = refo && pl->alpha_kind == 0 && nd > 0 && nbatch > 0 && pl->ga_batch != 1 &&
                          (pl->ga_batch == 2 || nd > kOverlapTables);
    if (ga_batch)
        if (int r = ga_batch_ensure(pl, nd, nbatch, pl->ga_pre_mb, pl->ga_pre_kb)) return r;
    pl->tabs.Gpre = nullptr;
    if (refo && !ga_batch && nbase == 0 && nd > 0 && nd <= kOverlapTables) {
        const size_t need = nusi::gamma_alphat_pre_doubles(pl->gd.T, nd);
        if (pl->gpre_doubles < need) {
            hipFree(pl->d_gpre);
            pl->d_gpre = nullptr;
            pl->gpre_doubles = 0;
            HIPCHECK(hipMalloc(&pl->d_gpre, sizeof(double) * need));
            pl->gpre_doubles = need;
        }
        pl->tabs.Gpre = pl->d_gpre;
    }
    // one upload: the zeroed warnings, batches, gamma groups, points and tables (nusi_plan::d_in)
    HIPCHECK(hipMemcpyAsync(pl->d_in, pl->h_in, pl->in_tpts + sizeof(nusi::Point) * ntab, hipMemcpyHostToDevice, s));
    nusi_plan* sp = nbase ? pl->shift : nullptr;
    if (sp) {
        HIPCHECK(hipMemcpyAsync(pl->d_smap, pl->h_smap, sizeof(int2) * (ntab - nd), hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(sp->d_tpts, sp->h_tpts, sizeof(nusi::Point) * nbase, hipMemcpyHostToDevice, s));
        HIPCHECK(hipMemcpyAsync(sp->d_batches, sp->h_batches, sizeof(int) * pl->shift_batches.nbatch,
                                hipMemcpyHostToDevice, s));
        HIPCHECK(hipEventRecord(sp->ev_copy, s));
        HIPCHECK(hipMemsetAsync(sp->d_warn, 0, sizeof(int) * nbase, s));
        HIPCHECK(hipMemsetAsync(sp->tabs.Wmin, 0x7f, sizeof(int) * 4 * (size_t)sp->grid.T * nbase, s));   // no row warned
        sp->ran = true;
    }
    HIPCHECK(hipEventRecord(pl->ev_copy, s));
    const nusi::SplineSet* spl = pl->spl ? pl->spl->d_set : pl->d_nospl;
    hipEvent_t* ev = pl->ev;
    if (pl->prof_n < pl->prof_max) ev = &pl->prof_ev[4 * (size_t)pl->prof_n++];
    HIPCHECK(hipEventRecord(ev[0], s));
    // A call of few tables leaves most of the GPU idle in each Stage-A kernel: Gamma / alphaTilde (independent of
    // alpha) run on the side stream beside the alpha kernels, and the cascade waits for both.  (Stage times: ev[1]
    // is then Gamma / alphaTilde's end on the side stream, and the alpha stage counts from there.)  Scans keep the
    // stages in order: beside a full alpha launch the overlap measured no gain (C4 155.0 -> 155.4 k, round 4).
    const bool ovl = !sp && nd > 0 && nd <= kOverlapTables;
    // after a fork, any early error return still joins the side stream into s (the next call's memsets and table
    // writes on s must not race a still-running Gamma / alphaTilde kernel)
    struct SideJoin {
        hipStream_t s = nullptr, side = nullptr;
        hipEvent_t done = nullptr;
        bool armed = false;
        ~SideJoin()
        {
            if (!armed) return;
            if (hipEventRecord(done, side) != hipSuccess) (void)hipStreamSynchronize(side);
            else (void)hipStreamWaitEvent(s, done, 0);
        }
    } join{s, pl->side, pl->ev_fork, false};
    if (ovl) {
        HIPCHECK(hipEventRecord(pl->ev_fork, s));
        HIPCHECK(hipStreamWaitEvent(pl->side, pl->ev_fork, 0));
        join.armed = true;
        HIPCHECK(nusi::launch_gamma_alphat(pl->gd, pl->d_tpts, nd, spl, pl->tabs, pl->d_warn, pl->side, refo,
                                           ga_batch ? &pl->gab : nullptr, pl->d_batches, pl->h_batches, nbatch));
        pl->ga_kernel = nusi::last_ga_kernel();
        HIPCHECK(hipEventRecord(ev[1], pl->side));
    } else {
        if (nd) {
            HIPCHECK(nusi::launch_gamma_alphat(pl->gd, pl->d_tpts, nd, spl, pl->tabs, pl->d_warn, s, refo,
                                               ga_batch ? &pl->gab : nullptr, pl->d_batches, pl->h_batches, nbatch));
            pl->ga_kernel = nusi::last_ga_kernel();
        }
        if (sp) HIPCHECK(nusi::launch_gamma_alphat(sp->gd, sp->d_tpts, nbase, spl, sp->tabs, sp->d_warn, s, refo));
        if (sp && !nd) pl->ga_kernel = nusi::last_ga_kernel();
        HIPCHECK(hipEventRecord(ev[1], s));
    }
    if (nd) {
        HIPCHECK(nusi::launch_alpha(pl->gd, pl->d_tpts, nd, spl, pl->atiles, pl->tabs, pl->d_warn, s, pl->d_batches,
                                    nbatch, cap, pl->alpha_kind, nb_plain, refo, pl->h_batches, &pl->mc));
    }
    if (sp) {
        const AlphaBatches& bb = pl->shift_batches;
        HIPCHECK(nusi::launch_alpha(sp->gd, sp->d_tpts, nbase, spl, sp->atiles, sp->tabs, sp->d_warn, s, sp->d_batches,
                                    bb.nbatch, bb.cap, pl->alpha_kind, bb.nb_plain, refo, sp->h_batches, &sp->mc));
        HIPCHECK(nusi::launch_table_shift(pl->gd, sp->gd, pl->d_smap, nd, ntab - nd, sp->tabs, pl->tabs, pl->d_warn, s));
    }
    if (ovl) {
        join.armed = false;
        HIPCHECK(hipStreamWaitEvent(s, ev[1], 0));
    }
    HIPCHECK(hipEventRecord(ev[2], s));
    if (bs && any_dsnb) HIPCHECK(nusi::launch_source_dsnb(pl->gd, pl->d_pts, n, pl->d_src, s));
    if (bs && any_tab) HIPCHECK(nusi::launch_source_tab(pl->gd, pl->d_pts, n, pl->d_slots, pl->d_src, s));
    const char* gb_name = nullptr;
    if (rc) {
        if (int r = response_cascade(pl, n, all_nr, rc->mass, d_flux, d_fla, s)) return r;
    } else if (bs) {
        const int Pk[3] = {16, 2, 1};
        static const char* const names[8] = {"", "k_cascade_bs_gamma", "k_cascade_bs_pairs", "k_cascade_bs_gamma + pairs",
                                             "k_cascade_bs", "k_cascade_bs_gamma + k_cascade_bs",
                                             "k_cascade_bs_pairs + k_cascade_bs", "k_cascade_bs_gamma + pairs + k_cascade_bs"};
        int off = 0, mask = 0;
        double* fh = pl->d_fh;
        for (int w = 0; w < 3; ++w) {
            if (bs_nwg[w]) {
                HIPCHECK(nusi::launch_cascade_bs(pl->gd, pl->d_pts, Pk[w], pl->d_gidx, pl->d_gbgrp + off, bs_nwg[w], pl->tabs,
                                                 fh, d_flux, d_fla, s, all_nr, force_passes));
                mask |= 1 << w;
            }
            fh += nusi::cascade_bs_scratch_doubles(pl->gd, Pk[w]) * bs_nwg[w];
            off += bs_nwg[w];
        }
        gb_name = names[mask];
    } else {
        HIPCHECK(nusi::launch_cascade_exact(pl->gd, pl->d_pts, n, pl->tabs, pl->d_slots, d_flux, d_fla, s));
    }
    HIPCHECK(hipEventRecord(ev[3], s));
    HIPCHECK(hipEventRecord(pl->ev_done, s));
    pl->alpha_kernel = nusi::last_alpha_kernel();
    if (sp) {   // the label of the kernel that built the base tables (the base launch runs last)
        pl->alpha_label = std::string(nusi::last_alpha_kernel()) + (nd ? " + k_table_shift" : " (shift base) + k_table_shift");
        pl->alpha_kernel = pl->alpha_label.c_str();
    }
    pl->cascade_kernel = gb_name ? gb_name : nusi::last_cascade_kernel();
    for (int k = 0; k < 4; ++k) pl->last_ev[k] = ev[k];   // stage_ms / warnings / tables refer to the latest call
    pl->ran = true;
    pl->last_n = n;
    pl->last_ntab = ntab;
    return NUSI_OK;
}

int nusi_plan_evolve(nusi_plan* pl, const nusi_params* pts, int n, double* d_flux, double* d_fla, void* stream)
{
    return plan_run(pl, pts, n, d_flux, d_fla, stream, nullptr);
}

// ---------------------------------------------------------------------------
// Response matrices (nusi_plan_response, nusi_plan_response_apply)
// ---------------------------------------------------------------------------
constexpr size_t kResponseFifoBytes = size_t(1) << 30;   // the impulse cascade's FIFO, at most (NUSI_OPT_RESPONSE_FIFO_KB = 0)
constexpr int kResponseChunk = 4096;                     // columns per launch of the scalar fallback

static bool response_impulse(const nusi_plan* pl)
{
    const int kind = pl->cascade_kind == NUSI_CASCADE_AUTO ? NUSI_CASCADE_MFMA : pl->cascade_kind;
    return kind == NUSI_CASCADE_MFMA && nusi::cascade_impulse_fits(pl->gd);
}
// tables per launch of the impulse cascade: whole tables whose FIFOs fit the budget (at least one); the mass-resolved
// cascade's table has three times the workgroups, hence three times the FIFO
static int response_chunk(const nusi_plan* pl, int n, bool mass)
{
    const size_t per = sizeof(double) * nusi::cascade_impulse_scratch_doubles(pl->gd) * (mass ? 3 : 1);
    const size_t budget = pl->response_fifo_kb > 0 ? (size_t)pl->response_fifo_kb << 10 : kResponseFifoBytes;
    return (int)std::min<size_t>((size_t)n, std::max<size_t>(1, budget / per));
}

// Before the call's upload: the buffers of the response's cascade (allocations may synchronise) and its weights.
static int response_prepare(nusi_plan* pl, const ResponseCall& rc, int n, hipStream_t s)
{
    const HostGrid& G = pl->grid;
    const nusi::GridDev& g = pl->gd;
    if (rc.mass) {
        if (int r = nusi_response_mass_shape(G.N, G.Nz, n, nullptr)) return r;
    } else if ((long long)n * (G.T + 1) > (long long)INT_MAX)
        return fail(NUSI_EPARAM, "response: points x source-axis bins exceed 2^31 - 1");
    pl->h_rw.assign(rc.w ? rc.w : G.sfr.data(), (rc.w ? rc.w : G.sfr.data()) + G.Nz);
    if (response_impulse(pl)) {
        if (!pl->d_rw) HIPCHECK(hipMalloc(&pl->d_rw, sizeof(double) * G.Nz));
        if (g.Nz - 1 > 6) {   // (one pass of 6 steps hands nothing on)
            const size_t fhd = nusi::cascade_impulse_scratch_doubles(g) * (rc.mass ? 3 : 1) * (size_t)response_chunk(pl, n, rc.mass);
            if (fhd > pl->fh_doubles) {
                hipFree(pl->d_fh);
                pl->d_fh = nullptr;
                pl->fh_doubles = 0;
                HIPCHECK(hipMalloc(&pl->d_fh, sizeof(double) * fhd));
                pl->fh_doubles = fhd;
            }
        }
        HIPCHECK(hipMemcpyAsync(pl->d_rw, pl->h_rw.data(), sizeof(double) * G.Nz, hipMemcpyHostToDevice, s));
        return NUSI_OK;
    }
    // the scalar fallback: slot n of a private slot array holds S = e_n and the weights
    const size_t per = nusi::cascade_slot_doubles(g), M = (size_t)G.T + 1;
    if (!pl->d_rslots) HIPCHECK(hipMalloc(&pl->d_rslots, sizeof(double) * per * M));
    if (!pl->d_rpts) HIPCHECK(hipMalloc(&pl->d_rpts, sizeof(nusi::Point) * kResponseChunk));
    if (!pl->d_rscr) HIPCHECK(hipMalloc(&pl->d_rscr, sizeof(double) * 3 * G.N * kResponseChunk));
    pl->h_rslots.assign(per * M, 0.0);
    for (size_t m = 0; m < M; ++m) {
        pl->h_rslots[per * m + m] = 1.0;
        memcpy(&pl->h_rslots[per * m + M], pl->h_rw.data(), sizeof(double) * G.Nz);
    }
    HIPCHECK(hipMemcpyAsync(pl->d_rslots, pl->h_rslots.data(), sizeof(double) * per * M, hipMemcpyHostToDevice, s));
    return NUSI_OK;
}

// The cascade of a response call: G[p][n][3][N] / G_fla (either may be NULL) of the call's n points; mass:
// G3[p][j][n][3][N] / G3_fla, a matrix per source mass state j.
static int response_cascade(nusi_plan* pl, int n, bool all_nr, bool mass, double* d_G, double* d_Gf, hipStream_t s)
{
    const nusi::GridDev& g = pl->gd;
    const size_t N3 = (size_t)3 * g.N, M = (size_t)g.T + 1;
    if (response_impulse(pl)) {
        // column 0 (bin 0 is never read): zeros; the kernel writes the columns 1 .. T
        for (double* out : {d_G, d_Gf})
            if (out) HIPCHECK(hipMemset2DAsync(out, sizeof(double) * M * N3, 0, sizeof(double) * N3, (size_t)n * (mass ? 3 : 1), s));
        const int chunk = response_chunk(pl, n, mass);
        for (int p0 = 0; p0 < n; p0 += chunk) {   // whole tables under the FIFO budget, one after the other on s
            if (mass)
                HIPCHECK(nusi::launch_cascade_mass_impulse(g, pl->d_pts, p0, std::min(chunk, n - p0), pl->d_rw, pl->tabs,
                                                           pl->d_fh, d_G, d_Gf, s, all_nr));
            else
            HIPCHECK(nusi::launch_cascade_impulse(g, pl->d_pts, p0, std::min(chunk, n - p0), pl->d_rw, pl->tabs, pl->d_fh,
                                                  d_G, d_Gf, s, all_nr));
        }
        return NUSI_OK;
    }
    if (mass) {
        // k_cascade_mass on temporary points: column c = (p 3 + j) M + n is point p on the private slot n with the
        // whole unit source (norm = 3: no third) in row j, which the kernel takes from the column's index
        std::vector<nusi::Point> tmp;
        const size_t ncol = (size_t)n * 3 * M;
        for (size_t c0 = 0; c0 < ncol; c0 += kResponseChunk) {
            const size_t cnt = std::min<size_t>(kResponseChunk, ncol - c0);
            tmp.resize(cnt);
            for (size_t c = 0; c < cnt; ++c) {
                const size_t p = (c0 + c) / (3 * M), m = (c0 + c) % M;
                tmp[c] = pl->h_pts[p];
                tmp[c].source = NUSI_SOURCE_TABULATED + (int)m;
                tmp[c].norm = tmp[c].norm_total = 3.0;
            }
            HIPCHECK(hipMemcpyAsync(pl->d_rpts, tmp.data(), sizeof(nusi::Point) * cnt, hipMemcpyHostToDevice, s));
            HIPCHECK(hipStreamSynchronize(s));   // (tmp is reused; the slow path)
            HIPCHECK(nusi::launch_cascade_mass_exact(g, pl->d_rpts, (int)cnt, pl->tabs, pl->d_rslots,
                                                     d_G ? d_G + c0 * N3 : pl->d_rscr, d_Gf ? d_Gf + c0 * N3 : pl->d_rscr,
                                                     (long long)c0, s));
        }
        return NUSI_OK;
    }
    // the unchanged scalar k_cascade on temporary points: column c = p M + n is point p on the private slot n
    // (norm = 1), a chunk of columns per launch; its outputs are contiguous in the n-major layout
    std::vector<nusi::Point> tmp;
    const size_t ncol = (size_t)n * M;
    for (size_t c0 = 0; c0 < ncol; c0 += kResponseChunk) {
        const size_t cnt = std::min<size_t>(kResponseChunk, ncol - c0);
        tmp.resize(cnt);
        for (size_t c = 0; c < cnt; ++c) {
            const size_t p = (c0 + c) / M, m = (c0 + c) - p * M;
            tmp[c] = pl->h_pts[p];
            tmp[c].source = NUSI_SOURCE_TABULATED + (int)m;
            tmp[c].norm = tmp[c].norm_total = 1.0;
        }
        HIPCHECK(hipMemcpyAsync(pl->d_rpts, tmp.data(), sizeof(nusi::Point) * cnt, hipMemcpyHostToDevice, s));
        HIPCHECK(hipStreamSynchronize(s));   // (tmp is reused; the slow path)
        HIPCHECK(nusi::launch_cascade_exact(g, pl->d_rpts, (int)cnt, pl->tabs, pl->d_rslots, d_G ? d_G + c0 * N3 : pl->d_rscr,
                                            d_Gf ? d_Gf + c0 * N3 : pl->d_rscr, s));
    }
    return NUSI_OK;
}

static int no_plan();
static int check_weights(const nusi_plan* pl, const double* w)
{
    if (w)
        for (int i = 0; i < pl->grid.Nz; ++i)
            if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(NUSI_EPARAM, "source redshift weight: an entry is negative or not finite");
    return NUSI_OK;
}

int nusi_plan_response(nusi_plan* pl, const nusi_params* pts, int n, const double* w, double* d_G, double* d_G_fla,
                       void* stream)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    if (int r = check_weights(pl, w)) return r;
    const ResponseCall rc{w, false};
    return plan_run(pl, pts, n, d_G, d_G_fla, stream, &rc);
}

// ---------------------------------------------------------------------------
// The mass-resolved response and the source's flavour composition (include/nusi.h)
// ---------------------------------------------------------------------------
int nusi_mixing(int normal_ordering, double* U2)
{
    if (!U2) return fail(NUSI_EPARAM, "mixing: U2 must not be NULL");
    pmns_sq(normal_ordering != 0, U2);
    return NUSI_OK;
}

int nusi_mass_fractions(int normal_ordering, const double* phi, double* kappa)
{
    if (!phi || !kappa) return fail(NUSI_EPARAM, "mass fractions: phi and kappa must not be NULL");
    for (int f = 0; f < 3; ++f)
        if (!(phi[f] >= 0.0) || !std::isfinite(phi[f])) return fail(NUSI_EPARAM, "mass fractions: a flavour share is negative or not finite");
    const double tot = (phi[0] + phi[1]) + phi[2];
    if (!(tot > 0.0) || !std::isfinite(tot)) return fail(NUSI_EPARAM, "mass fractions: the flavour shares are all zero (or their sum overflows)");
    double U2[9];
    pmns_sq(normal_ordering != 0, U2);
    for (int k = 0; k < 3; ++k) kappa[k] = ((phi[0] * U2[k] + phi[1] * U2[3 + k]) + phi[2] * U2[6 + k]) / tot;
    return NUSI_OK;
}

int nusi_response_mass_shape(int N, int Nz, int n, long long* doubles)
{
    if (N < 1 || Nz < 2 || n < 1) return fail(NUSI_EPARAM, "response mass: need N >= 1, Nz >= 2 and n >= 1");
    const long long M = (long long)N + Nz - 1;
    if ((long long)n * 3 * M > (long long)INT_MAX)
        return fail(NUSI_EPARAM, "response mass: points x 3 x source-axis bins exceed 2^31 - 1");
    if (doubles) *doubles = (long long)n * 3 * M * 3 * N;
    return NUSI_OK;
}

int nusi_plan_step_constants(const nusi_plan* pl, double* step_c, double* step_s)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    const HostGrid& G = pl->grid;
    if (step_c) memcpy(step_c, G.step_c.data(), sizeof(double) * G.Nz);
    if (step_s) memcpy(step_s, G.step_s.data(), sizeof(double) * G.Nz);
    return NUSI_OK;
}

int nusi_plan_response_mass(nusi_plan* pl, const nusi_params* pts, int n, const double* w, double* d_G3, double* d_G3_fla,
                            void* stream)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    if (int r = check_weights(pl, w)) return r;
    const ResponseCall rc{w, true};
    return plan_run(pl, pts, n, d_G3, d_G3_fla, stream, &rc);
}

int nusi_plan_response_mass_host(nusi_plan* pl, const nusi_params* pts, int n, const double* w, double* G3, double* G3_fla)
{
    if (!pl) return no_plan();
    if (n < 1 || n > pl->max_points) return fail(NUSI_EPARAM, "number of points outside [1, max_points]");
    if (int r = nusi_response_mass_shape(pl->grid.N, pl->grid.Nz, n, nullptr)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    const size_t nb = sizeof(double) * (size_t)n * 3 * (pl->grid.T + 1) * 3 * pl->grid.N;
    double* d[2] = {nullptr, nullptr};
    double* h[2] = {G3, G3_fla};
    int r = NUSI_OK;
    for (int k = 0; k < 2 && !r; ++k)
        if (h[k] && hipMalloc(&d[k], nb) != hipSuccess) r = fail(NUSI_EHIP, "response mass: no device memory for the result");
    if (!r) r = nusi_plan_response_mass(pl, pts, n, w, d[0], d[1], nullptr);
    if (!r && hipStreamSynchronize(pl->stream) != hipSuccess) r = fail(NUSI_EHIP, "response mass: the stream failed");
    for (int k = 0; k < 2 && !r; ++k)
        if (h[k] && hipMemcpy(h[k], d[k], nb, hipMemcpyDeviceToHost) != hipSuccess) r = fail(NUSI_EHIP, "response mass: copy to the host failed");
    hipFree(d[0]);
    hipFree(d[1]);
    if (r) return r;
    std::vector<int> wn(n);
    r = nusi_plan_warnings(pl, wn.data(), n);
    if (r) return r;
    for (int v : wn)
        if (v & nusi::kWarnSplineOOB) return fail(NUSI_EINTERP, "Error at interp: a phi-phi table lookup fell outside the node range");
    return NUSI_OK;
}

// out[t][c][x] = (kappa[t][c][0] A[t][0][x] + kappa[t][c][1] A[t][1][x]) + kappa[t][c][2] A[t][2][x] (k_response_compose)
static int compose_check(const nusi_plan* pl, const void* A, const void* out, int ntab, long long X, const double* kappa, int Qc)
{
    if (!pl) return no_plan();
    if (!A || !out || !kappa) return fail(NUSI_EPARAM, "response compose: A, kappa and out must not be NULL");
    if (ntab < 1 || Qc < 1 || X < 1) return fail(NUSI_EPARAM, "response compose: need ntab >= 1, Qc >= 1 and X >= 1");
    if ((long long)ntab * ((X + 255) / 256) > (long long)INT_MAX) return fail(NUSI_EPARAM, "response compose: too many elements (ntab X / 256 >= 2^31)");
    if ((long long)ntab * Qc > (long long)INT_MAX / 3) return fail(NUSI_EPARAM, "response compose: too many compositions (3 ntab Qc >= 2^31)");
    for (size_t e = 0; e < (size_t)ntab * Qc * 3; ++e)
        if (!(kappa[e] >= 0.0) || !std::isfinite(kappa[e])) return fail(NUSI_EPARAM, "response compose: a mass fraction is negative or not finite");
    return NUSI_OK;
}

int nusi_plan_response_compose(nusi_plan* pl, const double* d_A, int ntab, long long X, const double* kappa, int Qc,
                               double* d_out, void* stream)
{
    if (int r = compose_check(pl, d_A, d_out, ntab, X, kappa, Qc)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    if (!pl->ev_cmp) HIPCHECK(hipEventCreateWithFlags(&pl->ev_cmp, hipEventDisableTiming));
    if (pl->cmp_ran) HIPCHECK(hipEventSynchronize(pl->ev_cmp));   // d_kap / h_kap are reused
    const size_t need = (size_t)ntab * Qc * 3;
    if (pl->kap_doubles < need) {
        hipFree(pl->d_kap);
        pl->d_kap = nullptr;
        pl->kap_doubles = 0;
        HIPCHECK(hipMalloc(&pl->d_kap, sizeof(double) * need));
        pl->kap_doubles = need;
    }
    pl->h_kap.assign(kappa, kappa + need);
    HIPCHECK(hipMemcpyAsync(pl->d_kap, pl->h_kap.data(), sizeof(double) * need, hipMemcpyHostToDevice, s));
    HIPCHECK(nusi::launch_response_compose(d_A, ntab, (size_t)X, pl->d_kap, Qc, d_out, s));
    HIPCHECK(hipEventRecord(pl->ev_cmp, s));
    pl->cmp_ran = true;
    return NUSI_OK;
}

int nusi_plan_response_compose_host(nusi_plan* pl, const double* A, int ntab, long long X, const double* kappa, int Qc,
                                    double* out)
{
    if (int r = compose_check(pl, A, out, ntab, X, kappa, Qc)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    const size_t ab = sizeof(double) * (size_t)ntab * 3 * (size_t)X, ob = sizeof(double) * (size_t)ntab * Qc * (size_t)X;
    double *dA = nullptr, *dO = nullptr;
    int r = NUSI_OK;
    if (hipMalloc(&dA, ab) != hipSuccess || hipMalloc(&dO, ob) != hipSuccess) r = fail(NUSI_EHIP, "response compose: no device memory");
    if (!r && hipMemcpy(dA, A, ab, hipMemcpyHostToDevice) != hipSuccess) r = fail(NUSI_EHIP, "response compose: copy to the device failed");
    if (!r) r = nusi_plan_response_compose(pl, dA, ntab, X, kappa, Qc, dO, nullptr);
    if (!r && hipStreamSynchronize(pl->stream) != hipSuccess) r = fail(NUSI_EHIP, "response compose: the stream failed");
    if (!r && hipMemcpy(out, dO, ob, hipMemcpyDeviceToHost) != hipSuccess) r = fail(NUSI_EHIP, "response compose: copy to the host failed");
    hipFree(dA);
    hipFree(dO);
    return r;
}

int nusi_plan_response_host(nusi_plan* pl, const nusi_params* pts, int n, const double* w, double* G, double* G_fla)
{
    if (!pl) {   // (no plan exists without a GPU: say so, as nusi_plan_create does)
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(NUSI_EHIP, "no HIP device available");
        return fail(NUSI_EPARAM, "plan is NULL");
    }
    if (n < 1 || n > pl->max_points) return fail(NUSI_EPARAM, "number of points outside [1, max_points]");
    HIPCHECK(hipSetDevice(pl->device));
    const size_t nb = sizeof(double) * (size_t)n * (pl->grid.T + 1) * 3 * pl->grid.N;
    double* d[2] = {nullptr, nullptr};
    double* h[2] = {G, G_fla};
    int r = NUSI_OK;
    for (int k = 0; k < 2 && !r; ++k)
        if (h[k] && hipMalloc(&d[k], nb) != hipSuccess) r = fail(NUSI_EHIP, "response: no device memory for the result");
    if (!r) r = nusi_plan_response(pl, pts, n, w, d[0], d[1], nullptr);
    if (!r && hipStreamSynchronize(pl->stream) != hipSuccess) r = fail(NUSI_EHIP, "response: the stream failed");
    for (int k = 0; k < 2 && !r; ++k)
        if (h[k] && hipMemcpy(h[k], d[k], nb, hipMemcpyDeviceToHost) != hipSuccess) r = fail(NUSI_EHIP, "response: copy to the host failed");
    hipFree(d[0]);
    hipFree(d[1]);
    if (r) return r;
    std::vector<int> wn(n);
    r = nusi_plan_warnings(pl, wn.data(), n);
    if (r) return r;
    for (int v : wn)
        if (v & nusi::kWarnSplineOOB) return fail(NUSI_EINTERP, "Error at interp: a phi-phi table lookup fell outside the node range");
    return NUSI_OK;
}

int nusi_plan_response_apply(nusi_plan* pl, const double* d_G, int ntab, const double* S, int Q, const double* scale,
                             double* d_out, void* stream)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    if (!d_G || !d_out || !S) return fail(NUSI_EPARAM, "response apply: G, S and out must not be NULL");
    if (ntab < 1 || Q < 1 || Q > (1 << 19)) return fail(NUSI_EPARAM, "response apply: need ntab >= 1 and 1 <= Q <= 2^19");
    const size_t M = (size_t)pl->grid.T + 1;
    if ((long long)ntab * ((3 * pl->grid.N + 255) / 256) > (long long)INT_MAX) return fail(NUSI_EPARAM, "response apply: too many tables");
    for (size_t e = 0; e < (size_t)Q * M; ++e)
        if (!(S[e] >= 0.0) || !std::isfinite(S[e])) return fail(NUSI_EPARAM, "source spectrum: a bin integral is negative or not finite");
    if (scale)
        for (int q = 0; q < Q; ++q)
            if (!std::isfinite(scale[q])) return fail(NUSI_EPARAM, "response apply: a scale is not finite");
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    if (!pl->ev_app) HIPCHECK(hipEventCreateWithFlags(&pl->ev_app, hipEventDisableTiming));
    if (pl->app_ran) HIPCHECK(hipEventSynchronize(pl->ev_app));   // d_app / h_app are reused
    const size_t need = (size_t)Q * M + (size_t)Q;
    if (pl->app_doubles < need) {
        hipFree(pl->d_app);
        pl->d_app = nullptr;
        pl->app_doubles = 0;
        HIPCHECK(hipMalloc(&pl->d_app, sizeof(double) * need));
        pl->app_doubles = need;
    }
    pl->h_app.assign(S, S + (size_t)Q * M);
    if (scale) pl->h_app.insert(pl->h_app.end(), scale, scale + Q);
    HIPCHECK(hipMemcpyAsync(pl->d_app, pl->h_app.data(), sizeof(double) * pl->h_app.size(), hipMemcpyHostToDevice, s));
    HIPCHECK(nusi::launch_response_apply(pl->gd, d_G, ntab, pl->d_app, Q, scale ? pl->d_app + (size_t)Q * M : nullptr, d_out, s));
    HIPCHECK(hipEventRecord(pl->ev_app, s));
    pl->app_ran = true;
    return NUSI_OK;
}

int nusi_plan_response_apply_host(nusi_plan* pl, const double* G, int ntab, const double* S, int Q, const double* scale,
                                  double* out)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    if (!G || !out || ntab < 1 || Q < 1) return fail(NUSI_EPARAM, "response apply: G and out must not be NULL, ntab and Q >= 1");
    HIPCHECK(hipSetDevice(pl->device));
    const size_t N3 = (size_t)3 * pl->grid.N, gb = sizeof(double) * (size_t)ntab * (pl->grid.T + 1) * N3;
    const size_t ob = sizeof(double) * (size_t)ntab * Q * N3;
    double *dG = nullptr, *dO = nullptr;
    int r = NUSI_OK;
    if (hipMalloc(&dG, gb) != hipSuccess || hipMalloc(&dO, ob) != hipSuccess) r = fail(NUSI_EHIP, "response apply: no device memory");
    if (!r && hipMemcpy(dG, G, gb, hipMemcpyHostToDevice) != hipSuccess) r = fail(NUSI_EHIP, "response apply: copy to the device failed");
    if (!r) r = nusi_plan_response_apply(pl, dG, ntab, S, Q, scale, dO, nullptr);
    if (!r && hipStreamSynchronize(pl->stream) != hipSuccess) r = fail(NUSI_EHIP, "response apply: the stream failed");
    if (!r && hipMemcpy(out, dO, ob, hipMemcpyDeviceToHost) != hipSuccess) r = fail(NUSI_EHIP, "response apply: copy to the host failed");
    hipFree(dG);
    hipFree(dO);
    return r;
}

// ---------------------------------------------------------------------------
// The detector of a plan: nusi_plan_set_detector, the folds and the expected counts (nusi_detector.hip)
static int no_plan()   // (no plan exists without a GPU: say so, as nusi_plan_create does)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(NUSI_EHIP, "no HIP device available");
    return fail(NUSI_EPARAM, "plan is NULL");
}
// The detector calls of a plan may run on different streams, and ONE event, ev_det, stands for the end of all of them:
// each call first makes its stream wait for the event as it stands (the earlier calls, wherever they ran) and records
// it anew after its kernel, so whoever waits for ev_det -- set_detector before it frees d_det, the next events call
// before it overwrites d_evt -- waits for every earlier detector call.
static int detector_chain(nusi_plan* pl, hipStream_t s)
{
    if (pl->det_ran) HIPCHECK(hipStreamWaitEvent(s, pl->ev_det, 0));
    return NUSI_OK;
}
static int detector_mark(nusi_plan* pl, hipStream_t s)   // the end of a call that read the detector
{
    if (!pl->ev_det) HIPCHECK(hipEventCreateWithFlags(&pl->ev_det, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(pl->ev_det, s));
    pl->det_ran = true;
    return NUSI_OK;
}
static int detector_plan(const nusi_plan* pl, const char* what)   // a plan, and one with a detector
{
    if (!pl) return no_plan();
    if (!pl->det_C) return fail(NUSI_ESTATE, std::string(what) + ": the plan has no detector (nusi_plan_set_detector)");
    return NUSI_OK;
}
// the background of the plan's detector: d_det is Dt [3 N][ld], then bg [C]
static const double* detector_bg(const nusi_plan* pl) { return pl->d_det + (size_t)3 * pl->grid.N * nusi::detector_ld(pl->det_C); }
static int detector_fold(nusi_plan* pl, const double* d_X, int ntab, int rows, bool tri, double* d_out, void* stream, const char* what)
{
    if (int r = detector_plan(pl, what)) return r;
    if (!d_X || !d_out) return fail(NUSI_EPARAM, std::string(what) + ": the input and the output must not be NULL");
    if (ntab < 1 || rows < 1) return fail(NUSI_EPARAM, std::string(what) + ": need at least one row");
    if ((long long)ntab * ((rows + 15) / 16) > (long long)INT_MAX) return fail(NUSI_EPARAM, std::string(what) + ": too many rows");
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    if (int r = detector_chain(pl, s)) return r;
    HIPCHECK(nusi::launch_detector_fold(pl->gd, d_X, ntab, rows, tri, pl->d_det, pl->det_C, tri ? nullptr : detector_bg(pl), d_out, s));
    return detector_mark(pl, s);
}
// host arrays through a device call: in [nin] -> out [nout] doubles
static int detector_host(nusi_plan* pl, const double* in, size_t nin, double* out, size_t nout, const char* what,
                  const std::function<int(const double*, double*)>& call)
{
    HIPCHECK(hipSetDevice(pl->device));
    double *dI = nullptr, *dO = nullptr;
    int r = NUSI_OK;
    if (hipMalloc(&dI, sizeof(double) * nin) != hipSuccess || hipMalloc(&dO, sizeof(double) * nout) != hipSuccess)
        r = fail(NUSI_EHIP, std::string(what) + ": no device memory");
    if (!r && hipMemcpy(dI, in, sizeof(double) * nin, hipMemcpyHostToDevice) != hipSuccess)
        r = fail(NUSI_EHIP, std::string(what) + ": copy to the device failed");
    if (!r) r = call(dI, dO);
    if (!r && hipStreamSynchronize(pl->stream) != hipSuccess) r = fail(NUSI_EHIP, std::string(what) + ": the stream failed");
    if (!r && hipMemcpy(out, dO, sizeof(double) * nout, hipMemcpyDeviceToHost) != hipSuccess)
        r = fail(NUSI_EHIP, std::string(what) + ": copy to the host failed");
    hipFree(dI);
    hipFree(dO);
    return r;
}
// The events, the profile and the fit call on host arrays: R [ntab][M][C] through detector_host into one block of the
// output segments in their order, each on a multiple of 8 bytes; the call gets their device addresses (NULL where the
// host pointer is NULL) and the segments asked for are copied back.
struct HostSeg {
    void* host;
    size_t count, size;   // elements, bytes per element
};
static int events_host(nusi_plan* pl, const double* R, int ntab, const std::vector<HostSeg>& segs, const char* what,
                       const std::function<int(const double*, void* const*)>& call)
{
    std::vector<size_t> off(1, 0);
    for (const HostSeg& g : segs) off.push_back(off.back() + (g.count * g.size + 7) / 8);
    std::vector<double> o(off.back());
    const int r = detector_host(pl, R, (size_t)ntab * (pl->grid.T + 1) * pl->det_C, o.data(), o.size(), what,
                                [&](const double* dI, double* dO) {
                                    std::vector<void*> d;
                                    for (const HostSeg& g : segs) d.push_back(g.host ? dO + off[d.size()] : nullptr);
                                    return call(dI, d.data());
                                });
    for (size_t k = 0; k < segs.size() && !r; ++k)
        if (segs[k].host) memcpy(segs[k].host, o.data() + off[k], segs[k].count * segs[k].size);
    return r;
}

int nusi_plan_set_detector(nusi_plan* pl, int C, const double* D, const double* B)
{
    if (!pl) return no_plan();
    const bool clear = !D;   // (C = 0 comes with D = NULL; a D with C = 0 is refused below)
    if (D) {
        if (C < 1 || C > NUSI_DETECTOR_BINS_MAX) return fail(NUSI_EPARAM, "detector: C outside 1 .. NUSI_DETECTOR_BINS_MAX");
        const size_t R3 = (size_t)3 * pl->grid.N;
        for (size_t e = 0; e < (size_t)C * R3; ++e)
            if (!(D[e] >= 0.0) || !std::isfinite(D[e])) return fail(NUSI_EPARAM, "detector: an entry of D is negative or not finite");
        if (B)
            for (int c = 0; c < C; ++c)
                if (!(B[c] >= 0.0) || !std::isfinite(B[c])) return fail(NUSI_EPARAM, "detector: a background is negative or not finite");
    }
    HIPCHECK(hipSetDevice(pl->device));
    // the new detector first, in a block of its own: a failure below leaves the plan with the detector it had
    double* d_new = nullptr;
    if (!clear) {
        const size_t R3 = (size_t)3 * pl->grid.N;
        const int ld = nusi::detector_ld(C);
        std::vector<double> v(R3 * ld + (size_t)C, 0.0);
        for (int c = 0; c < C; ++c)
            for (size_t r = 0; r < R3; ++r) v[r * ld + c] = D[(size_t)c * R3 + r];
        if (B) memcpy(v.data() + R3 * ld, B, sizeof(double) * C);
        HIPCHECK(hipMalloc(&d_new, sizeof(double) * v.size()));
        const hipError_t e = hipMemcpy(d_new, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(d_new);
            HIPCHECK(e);
        }
    }
    // ordered with the plan's calls (nusi_plan_set_source's rule): the earlier ones, on whatever stream they ran,
    // finish with the old detector (ev_det covers every detector call: detector_chain) before it is freed
    hipError_t e = pl->ran ? hipEventSynchronize(pl->ev_done) : hipSuccess;
    if (e == hipSuccess && pl->det_ran) e = hipEventSynchronize(pl->ev_det);
    if (e != hipSuccess) {
        hipFree(d_new);
        HIPCHECK(e);
    }
    hipFree(pl->d_det);
    pl->d_det = d_new;
    pl->det_C = clear ? 0 : C;
    hipFree(pl->d_tpl);   // the templates belong to the detector they were set for
    pl->d_tpl = nullptr;
    pl->fit_K = 0;
    return NUSI_OK;
}

int nusi_plan_detector_bins(const nusi_plan* pl) { return pl ? pl->det_C : 0; }

int nusi_plan_fold_flux(nusi_plan* pl, const double* d_flux_fla, int n, double* d_mu, void* stream)
{
    if (!pl) return no_plan();
    return detector_fold(pl, d_flux_fla, 1, n, false, d_mu, stream, "fold flux");
}

int nusi_plan_response_fold(nusi_plan* pl, const double* d_G_fla, int ntab, double* d_R, void* stream)
{
    if (!pl) return no_plan();
    return detector_fold(pl, d_G_fla, ntab, pl->grid.T + 1, true, d_R, stream, "response fold");
}

int nusi_plan_fold_flux_host(nusi_plan* pl, const double* flux_fla, int n, double* mu)
{
    if (int r = detector_plan(pl, "fold flux")) return r;
    if (!flux_fla || !mu || n < 1) return fail(NUSI_EPARAM, "fold flux: the input and the output must not be NULL, n >= 1");
    return detector_host(pl, flux_fla, (size_t)n * 3 * pl->grid.N, mu, (size_t)n * pl->det_C, "fold flux",
                         [&](const double* dI, double* dO) { return nusi_plan_fold_flux(pl, dI, n, dO, nullptr); });
}

int nusi_plan_response_fold_host(nusi_plan* pl, const double* G_fla, int ntab, double* R)
{
    if (int r = detector_plan(pl, "response fold")) return r;
    if (!G_fla || !R || ntab < 1) return fail(NUSI_EPARAM, "response fold: the input and the output must not be NULL, ntab >= 1");
    const size_t M = (size_t)pl->grid.T + 1;
    return detector_host(pl, G_fla, (size_t)ntab * M * 3 * pl->grid.N, R, (size_t)ntab * M * pl->det_C, "response fold",
                         [&](const double* dI, double* dO) { return nusi_plan_response_fold(pl, dI, ntab, dO, nullptr); });
}

// The argument checks of the events and the profile call (what: the call's name in the messages), and the staging of
// their host vectors: S [Q][M], scale [Q] (or zeros) and data [P][C] (or zeros; P = 1 for every call but the ensemble)
// into the plan's d_evt, in that order, on s.
static int events_check(const nusi_plan* pl, const char* what, const double* d_R, int ntab, const double* S, int Q,
                        const double* scale, const double* data, int P)
{
    if (!d_R || !S) return fail(NUSI_EPARAM, std::string(what) + ": R and S must not be NULL");
    if (ntab < 1 || Q < 1 || Q > (1 << 19)) return fail(NUSI_EPARAM, std::string(what) + ": need ntab >= 1 and 1 <= Q <= 2^19");
    const size_t M = (size_t)pl->grid.T + 1;
    for (size_t e = 0; e < (size_t)Q * M; ++e)
        if (!(S[e] >= 0.0) || !std::isfinite(S[e])) return fail(NUSI_EPARAM, "source spectrum: a bin integral is negative or not finite");
    if (scale)
        for (int q = 0; q < Q; ++q)
            if (!(scale[q] >= 0.0) || !std::isfinite(scale[q])) return fail(NUSI_EPARAM, std::string(what) + ": a scale is negative or not finite");
    if (data)
        for (size_t c = 0; c < (size_t)P * pl->det_C; ++c)
            if (!(data[c] >= 0.0) || !std::isfinite(data[c])) return fail(NUSI_EPARAM, std::string(what) + ": a datum is negative or not finite");
    return NUSI_OK;
}
// d_evt's layout, written down here and nowhere else: S [Q][M], scale [Q], data [P][C], then a call's further host
// vectors, extra [nextra] (the calibration call's a_test and q_obs); offsets in doubles
struct EvtLayout {
    size_t scale, data, extra, total;
};
static EvtLayout evt_layout(const nusi_plan* pl, int Q, int P, size_t nextra)
{
    EvtLayout l;
    l.scale = (size_t)Q * ((size_t)pl->grid.T + 1);
    l.data = l.scale + (size_t)Q;
    l.extra = l.data + (size_t)P * pl->det_C;
    l.total = l.extra + nextra;
    return l;
}
static int events_stage(nusi_plan* pl, const double* S, int Q, const double* scale, const double* data, int P, hipStream_t s,
                        const double* extra = nullptr, size_t nextra = 0)
{
    const size_t M = (size_t)pl->grid.T + 1;
    const int C = pl->det_C;
    if (pl->det_ran) HIPCHECK(hipEventSynchronize(pl->ev_det));   // d_evt / h_evt are reused (every earlier detector
                                                                  // call has finished: detector_chain)
    const EvtLayout l = evt_layout(pl, Q, P, nextra);
    const size_t need = l.total;
    if (pl->evt_doubles < need) {
        hipFree(pl->d_evt);
        pl->d_evt = nullptr;
        pl->evt_doubles = 0;
        HIPCHECK(hipMalloc(&pl->d_evt, sizeof(double) * need));
        pl->evt_doubles = need;
    }
    pl->h_evt.assign(S, S + (size_t)Q * M);
    pl->h_evt.resize(need, 0.0);
    if (scale) memcpy(pl->h_evt.data() + l.scale, scale, sizeof(double) * Q);
    if (data) memcpy(pl->h_evt.data() + l.data, data, sizeof(double) * P * C);
    if (extra) memcpy(pl->h_evt.data() + l.extra, extra, sizeof(double) * nextra);
    HIPCHECK(hipMemcpyAsync(pl->d_evt, pl->h_evt.data(), sizeof(double) * need, hipMemcpyHostToDevice, s));
    return NUSI_OK;
}
// What the events, the profile and the fit call share after their own checks: events_check, the device and the stream,
// events_stage; gives the stream and the staged vectors (scale: NULL without one) with the detector's background.
// The call launches on a.s and ends with detector_mark.
struct EventsArgs {
    hipStream_t s;
    const double *S, *scale, *data, *bg;
};
static int events_begin(nusi_plan* pl, const char* what, const double* d_R, int ntab, const double* S, int Q,
                        const double* scale, const double* data, int P, void* stream, EventsArgs& a)
{
    if (int r = events_check(pl, what, d_R, ntab, S, Q, scale, data, P)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    a.s = stream ? (hipStream_t)stream : pl->stream;
    if (int r = events_stage(pl, S, Q, scale, data, P, a.s)) return r;
    const EvtLayout l = evt_layout(pl, Q, P, 0);
    a.S = pl->d_evt;
    a.scale = scale ? pl->d_evt + l.scale : nullptr;
    a.data = pl->d_evt + l.data;
    a.bg = detector_bg(pl);
    return NUSI_OK;
}

int nusi_plan_response_events(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* scale,
                              const double* data, double* d_mu, double* d_nll, void* stream)
{
    if (int r = detector_plan(pl, "response events")) return r;
    if (!d_mu && !d_nll) return fail(NUSI_EPARAM, "response events: mu and nll are both NULL");
    if (d_nll && !data) return fail(NUSI_EPARAM, "response events: nll needs data");
    EventsArgs a;
    if (int r = events_begin(pl, "response events", d_R, ntab, S, Q, scale, data, 1, stream, a)) return r;
    HIPCHECK(nusi::launch_detector_events(pl->gd, d_R, ntab, a.S, Q, a.scale, a.data, a.bg, pl->det_C, d_mu, d_nll, a.s));
    return detector_mark(pl, a.s);
}

int nusi_plan_response_events_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* scale,
                                   const double* data, double* mu, double* nll)
{
    if (int r = detector_plan(pl, "response events")) return r;
    if (!R || ntab < 1 || Q < 1) return fail(NUSI_EPARAM, "response events: R must not be NULL, ntab and Q >= 1");
    if (!mu && !nll) return fail(NUSI_EPARAM, "response events: mu and nll are both NULL");
    const size_t nn = (size_t)ntab * Q, nmu = nn * pl->det_C;
    return events_host(pl, R, ntab, {{mu, nmu, sizeof(double)}, {nll, nn, sizeof(double)}}, "response events",
                       [&](const double* dI, void* const* d) {
                           return nusi_plan_response_events(pl, dI, ntab, S, Q, scale, data, (double*)d[0], (double*)d[1], nullptr);
                       });
}

int nusi_plan_response_profile(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* data,
                               double* d_ahat, double* d_nll, double* d_mu, int* d_status, void* stream)
{
    if (int r = detector_plan(pl, "response profile")) return r;
    if (!data || !d_ahat) return fail(NUSI_EPARAM, "response profile: data and ahat must not be NULL");
    EventsArgs a;
    if (int r = events_begin(pl, "response profile", d_R, ntab, S, Q, nullptr, data, 1, stream, a)) return r;
    HIPCHECK(nusi::launch_detector_profile(pl->gd, d_R, ntab, a.S, Q, a.data, a.bg, pl->det_C, d_ahat, d_nll, d_mu, d_status, a.s));
    return detector_mark(pl, a.s);
}

int nusi_plan_response_profile_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* data,
                                    double* ahat, double* nll, double* mu, int* status)
{
    if (int r = detector_plan(pl, "response profile")) return r;
    if (!R || ntab < 1 || Q < 1) return fail(NUSI_EPARAM, "response profile: R must not be NULL, ntab and Q >= 1");
    if (!data || !ahat) return fail(NUSI_EPARAM, "response profile: data and ahat must not be NULL");
    const size_t nn = (size_t)ntab * Q, nmu = nn * pl->det_C;
    return events_host(pl, R, ntab,
                       {{ahat, nn, sizeof(double)}, {nll, nn, sizeof(double)}, {mu, nmu, sizeof(double)}, {status, nn, sizeof(int)}},
                       "response profile", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_profile(pl, dI, ntab, S, Q, data, (double*)d[0], (double*)d[1], (double*)d[2],
                                                             (int*)d[3], nullptr);
                       });
}

// The fit's background templates (nusi_plan_set_templates) and the fit (nusi_detector.hip k_detector_fit)
int nusi_plan_set_templates(nusi_plan* pl, int K, const double* T, const double* prior_mean, const double* prior_sigma)
{
    if (int r = detector_plan(pl, "templates")) return r;
    const bool clear = !T || K == 0;
    const int C = pl->det_C;
    double m[NUSI_FIT_TEMPLATES_MAX] = {}, w[NUSI_FIT_TEMPLATES_MAX] = {}, sw[NUSI_FIT_TEMPLATES_MAX];
    for (double& x : sw) x = HUGE_VAL;
    if (!clear) {
        if (K < 0 || K > NUSI_FIT_TEMPLATES_MAX) return fail(NUSI_EPARAM, "templates: K outside 0 .. NUSI_FIT_TEMPLATES_MAX");
        for (int j = 0; j < K; ++j) {
            bool some = false;
            for (int c = 0; c < C; ++c) {
                const double x = T[(size_t)j * C + c];
                if (!(x >= 0.0) || !std::isfinite(x)) return fail(NUSI_EPARAM, "templates: an entry is negative or not finite");
                some = some || x > 0.0;
            }
            if (!some) return fail(NUSI_EPARAM, "templates: a template of zeros");
            if (prior_mean && (!(prior_mean[j] >= 0.0) || !std::isfinite(prior_mean[j])))
                return fail(NUSI_EPARAM, "templates: a prior mean is negative or not finite");
            if (prior_sigma) {
                const double sg = prior_sigma[j];
                if (!(sg > 0.0)) return fail(NUSI_EPARAM, "templates: a prior width is not > 0");
                w[j] = 1.0 / (sg * sg);
                m[j] = (w[j] > 0.0 && prior_mean) ? prior_mean[j] : 0.0;
                if (w[j] > 0.0) sw[j] = sg;
            }
        }
    } else if (K < 0 || K > NUSI_FIT_TEMPLATES_MAX) {
        return fail(NUSI_EPARAM, "templates: K outside 0 .. NUSI_FIT_TEMPLATES_MAX");
    }
    HIPCHECK(hipSetDevice(pl->device));
    double* d_new = nullptr;
    if (!clear) {
        HIPCHECK(hipMalloc(&d_new, sizeof(double) * (size_t)K * C));
        const hipError_t e = hipMemcpy(d_new, T, sizeof(double) * (size_t)K * C, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            hipFree(d_new);
            HIPCHECK(e);
        }
    }
    // (ev_det covers every earlier detector call, the fits among them: nusi_plan_set_detector's rule)
    const hipError_t e = pl->det_ran ? hipEventSynchronize(pl->ev_det) : hipSuccess;
    if (e != hipSuccess) {
        hipFree(d_new);
        HIPCHECK(e);
    }
    hipFree(pl->d_tpl);
    pl->d_tpl = d_new;
    pl->fit_K = clear ? 0 : K;
    memcpy(pl->fit_m, m, sizeof(m));
    memcpy(pl->fit_w, w, sizeof(w));
    memcpy(pl->fit_s, sw, sizeof(sw));
    return NUSI_OK;
}

int nusi_plan_templates(const nusi_plan* pl) { return pl ? pl->fit_K : 0; }

int nusi_plan_response_fit(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* data,
                           double* d_theta, double* d_nll, double* d_mu, int* d_status, void* stream)
{
    if (int r = detector_plan(pl, "response fit")) return r;
    if (!pl->fit_K) return fail(NUSI_ESTATE, "response fit: the plan has no templates (nusi_plan_set_templates; without them: nusi_plan_response_profile)");
    if (!data || !d_theta) return fail(NUSI_EPARAM, "response fit: data and theta must not be NULL");
    EventsArgs a;
    if (int r = events_begin(pl, "response fit", d_R, ntab, S, Q, nullptr, data, 1, stream, a)) return r;
    HIPCHECK(nusi::launch_detector_fit(pl->gd, d_R, ntab, a.S, Q, a.data, a.bg, pl->det_C, pl->fit_K, pl->d_tpl, pl->fit_m,
                                       pl->fit_w, d_theta, d_nll, d_mu, d_status, a.s));
    return detector_mark(pl, a.s);
}

int nusi_plan_response_fit_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* data,
                                double* theta, double* nll, double* mu, int* status)
{
    if (int r = detector_plan(pl, "response fit")) return r;
    if (!pl->fit_K) return fail(NUSI_ESTATE, "response fit: the plan has no templates (nusi_plan_set_templates; without them: nusi_plan_response_profile)");
    if (!R || ntab < 1 || Q < 1) return fail(NUSI_EPARAM, "response fit: R must not be NULL, ntab and Q >= 1");
    if (!data || !theta) return fail(NUSI_EPARAM, "response fit: data and theta must not be NULL");
    const size_t nn = (size_t)ntab * Q, nmu = nn * pl->det_C, nth = nn * (1 + pl->fit_K);
    return events_host(pl, R, ntab,
                       {{theta, nth, sizeof(double)}, {nll, nn, sizeof(double)}, {mu, nmu, sizeof(double)}, {status, nn, sizeof(int)}},
                       "response fit", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_fit(pl, dI, ntab, S, Q, data, (double*)d[0], (double*)d[1], (double*)d[2],
                                                         (int*)d[3], nullptr);
                       });
}

// The fit with J signal components per (table, spectrum) (nusi_detector.hip k_components_fit).  The size limits are a
// pure function, which the call applies with the detector's C and the plan's K.
int nusi_fit_components_shape(int C, int J, int K, int ntab, int Q, long long* records)
{
    const std::string w = "response fit components: ";
    if (C < 1 || C > NUSI_DETECTOR_BINS_MAX) return fail(NUSI_EPARAM, w + "C outside 1 .. NUSI_DETECTOR_BINS_MAX");
    if (J < 2 || J > NUSI_FIT_SIGNALS_MAX) return fail(NUSI_EPARAM, w + "J outside 2 .. NUSI_FIT_SIGNALS_MAX (J = 1 is nusi_plan_response_fit / _profile)");
    if (K < 0 || K > NUSI_FIT_TEMPLATES_MAX) return fail(NUSI_EPARAM, w + "K outside 0 .. NUSI_FIT_TEMPLATES_MAX");
    if (ntab < 1 || Q < 1 || Q > (1 << 19)) return fail(NUSI_EPARAM, w + "need ntab >= 1 and 1 <= Q <= 2^19");
    const long long nn = (long long)ntab * Q;
    const long long widest = C > J + K ? C : J + K;   // (mu [C] or theta [J + K]: the largest output)
    if (nn >= (1ll << 31) || nn * widest >= (1ll << 31))
        return fail(NUSI_EPARAM, w + "too many records (ntab Q, or an output's elements, >= 2^31)");
    if (records) *records = nn;
    return NUSI_OK;
}

int nusi_plan_response_fit_components(nusi_plan* pl, const double* d_R3, int ntab, int J, const double* S, int Q,
                                      const double* data, double* d_theta, double* d_nll, double* d_mu, int* d_status,
                                      void* stream)
{
    if (int r = detector_plan(pl, "response fit components")) return r;
    if (int r = nusi_fit_components_shape(pl->det_C, J, pl->fit_K, ntab, Q, nullptr)) return r;
    if (!data || !d_theta) return fail(NUSI_EPARAM, "response fit components: data and theta must not be NULL");
    EventsArgs a;
    if (int r = events_begin(pl, "response fit components", d_R3, ntab, S, Q, nullptr, data, 1, stream, a)) return r;
    HIPCHECK(nusi::launch_components_fit(pl->gd, d_R3, ntab, J, a.S, Q, a.data, a.bg, pl->det_C, pl->fit_K, pl->d_tpl,
                                         pl->fit_m, pl->fit_w, d_theta, d_nll, d_mu, d_status, a.s));
    return detector_mark(pl, a.s);
}

int nusi_plan_response_fit_components_host(nusi_plan* pl, const double* R3, int ntab, int J, const double* S, int Q,
                                           const double* data, double* theta, double* nll, double* mu, int* status)
{
    if (int r = detector_plan(pl, "response fit components")) return r;
    if (int r = nusi_fit_components_shape(pl->det_C, J, pl->fit_K, ntab, Q, nullptr)) return r;
    if (!R3) return fail(NUSI_EPARAM, "response fit components: R3 must not be NULL");
    if (!data || !theta) return fail(NUSI_EPARAM, "response fit components: data and theta must not be NULL");
    const size_t nn = (size_t)ntab * Q, nmu = nn * pl->det_C, nth = nn * (J + pl->fit_K);
    // (R3 is ntab J folded matrices in a row)
    return events_host(pl, R3, ntab * J,
                       {{theta, nth, sizeof(double)}, {nll, nn, sizeof(double)}, {mu, nmu, sizeof(double)}, {status, nn, sizeof(int)}},
                       "response fit components", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_fit_components(pl, dI, ntab, J, S, Q, data, (double*)d[0], (double*)d[1],
                                                                    (double*)d[2], (int*)d[3], nullptr);
                       });
}

// The ensemble (nusi_detector.hip k_ensemble_profile / k_ensemble_fit / k_ensemble_best).  The grid is (tables,
// q-slices, p-slices).  Automatic slices: the grid should hold kEnsBlocksPerCU blocks per compute unit, several rounds
// of what is resident at once, so that the last round's tail is short (measured: DESIGN.md sec. 4).  Spectrum blocks
// are split first -- a q-slice repeats no work, it costs P ntab records of scratch and the merge -- as far as the
// spectrum blocks and kEnsScratchBytes of scratch allow; the data sets are split only where that leaves the grid short,
// and into slices of at least kEnsSliceDatasets, since every p-slice repeats the front half.  An option > 0 holds
// instead, capped only by what there is to split.
constexpr size_t kEnsScratchBytes = size_t(256) << 20;
constexpr int kEnsBlocksPerCU = 32, kEnsSliceDatasets = 16;
static int ensemble_slices(nusi_plan* pl, int ntab, int Q, int P, int& qs, int& ps)
{
    const int nqb = nusi::ensemble_blocks(pl->det_C, pl->fit_K, Q);
    int ncu = 0;
    HIPCHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device));
    const long long want = (long long)kEnsBlocksPerCU * (ncu > 0 ? ncu : 1);
    if (pl->ens_qslices > 0) {
        qs = std::min(pl->ens_qslices, nqb);
    } else {
        const size_t per = (size_t)P * ntab * nusi::ensemble_record_bytes(pl->fit_K);
        const long long fit = (long long)(kEnsScratchBytes / per);
        qs = (int)std::min<long long>(std::min<long long>(nqb, 65535), (want + ntab - 1) / ntab);
        if (qs > fit) qs = fit > 1 ? (int)fit : 1;
    }
    if (pl->ens_pslices > 0) {
        ps = std::min(pl->ens_pslices, P);
    } else {
        const long long have = (long long)ntab * qs;
        ps = (int)std::min<long long>(std::max(P / kEnsSliceDatasets, 1), (want + have - 1) / have);
    }
    return NUSI_OK;
}

int nusi_plan_response_ensemble(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* data, int P,
                                int* d_q, double* d_nll, double* d_theta, int* d_status, void* stream)
{
    if (int r = detector_plan(pl, "response ensemble")) return r;
    if (!data || !d_q || !d_nll) return fail(NUSI_EPARAM, "response ensemble: data, q and nll must not be NULL");
    if (P < 1 || P > NUSI_ENSEMBLE_DATASETS_MAX) return fail(NUSI_EPARAM, "response ensemble: P outside 1 .. NUSI_ENSEMBLE_DATASETS_MAX");
    if ((long long)ntab * P > (long long)INT_MAX) return fail(NUSI_EPARAM, "response ensemble: too many records (P ntab >= 2^31)");
    EventsArgs a;
    if (int r = events_begin(pl, "response ensemble", d_R, ntab, S, Q, nullptr, data, P, stream, a)) return r;
    int qs = 1, ps = 1;
    if (int r = ensemble_slices(pl, ntab, Q, P, qs, ps)) return r;
    if (qs > 1) {   // (every earlier detector call has finished: events_stage)
        const size_t need = (size_t)qs * P * ntab * nusi::ensemble_record_bytes(pl->fit_K);
        if (pl->ens_bytes < need) {
            hipFree(pl->d_ens);
            pl->d_ens = nullptr;
            pl->ens_bytes = 0;
            HIPCHECK(hipMalloc(&pl->d_ens, need));
            pl->ens_bytes = need;
        }
    }
    HIPCHECK(nusi::launch_detector_ensemble(pl->gd, d_R, ntab, a.S, Q, a.data, P, a.bg, pl->det_C, pl->fit_K, pl->d_tpl,
                                            pl->fit_m, pl->fit_w, qs, ps, pl->d_ens, d_q, d_nll, d_theta, d_status, a.s));
    return detector_mark(pl, a.s);
}

int nusi_plan_response_ensemble_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* data,
                                     int P, int* q, double* nll, double* theta, int* status)
{
    if (int r = detector_plan(pl, "response ensemble")) return r;
    if (!R || ntab < 1 || Q < 1) return fail(NUSI_EPARAM, "response ensemble: R must not be NULL, ntab and Q >= 1");
    if (!data || !q || !nll) return fail(NUSI_EPARAM, "response ensemble: data, q and nll must not be NULL");
    if (P < 1 || P > NUSI_ENSEMBLE_DATASETS_MAX) return fail(NUSI_EPARAM, "response ensemble: P outside 1 .. NUSI_ENSEMBLE_DATASETS_MAX");
    const size_t nn = (size_t)P * ntab, nth = nn * (1 + pl->fit_K);
    return events_host(pl, R, ntab,
                       {{q, nn, sizeof(int)}, {nll, nn, sizeof(double)}, {theta, nth, sizeof(double)}, {status, nn, sizeof(int)}},
                       "response ensemble", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_ensemble(pl, dI, ntab, S, Q, data, P, (int*)d[0], (double*)d[1],
                                                              (double*)d[2], (int*)d[3], nullptr);
                       });
}

// The conditional fit (nusi_detector.hip k_conditional_fit): the fit's templates with the signal's scale held.  The
// scales ride in the slot events_stage has for the events call's.
static int fit_fixed_plan(const nusi_plan* pl)
{
    if (int r = detector_plan(pl, "response fit_fixed")) return r;
    if (!pl->fit_K) return fail(NUSI_ESTATE, "response fit_fixed: the plan has no templates (nusi_plan_set_templates; without them: nusi_plan_response_events)");
    return NUSI_OK;
}

int nusi_plan_response_fit_fixed(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* scale,
                                 const double* data, double* d_theta, double* d_nll, double* d_mu, int* d_status, void* stream)
{
    if (int r = fit_fixed_plan(pl)) return r;
    if (!scale || !data || !d_theta) return fail(NUSI_EPARAM, "response fit_fixed: scale, data and theta must not be NULL");
    EventsArgs a;
    if (int r = events_begin(pl, "response fit_fixed", d_R, ntab, S, Q, scale, data, 1, stream, a)) return r;
    HIPCHECK(nusi::launch_conditional_fit(pl->gd, d_R, ntab, a.S, Q, a.scale, a.data, a.bg, pl->det_C, pl->fit_K, pl->d_tpl,
                                          pl->fit_m, pl->fit_w, d_theta, d_nll, d_mu, d_status, a.s));
    return detector_mark(pl, a.s);
}

int nusi_plan_response_fit_fixed_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* scale,
                                      const double* data, double* theta, double* nll, double* mu, int* status)
{
    if (int r = fit_fixed_plan(pl)) return r;
    if (!R || ntab < 1 || Q < 1) return fail(NUSI_EPARAM, "response fit_fixed: R must not be NULL, ntab and Q >= 1");
    if (!scale || !data || !theta) return fail(NUSI_EPARAM, "response fit_fixed: scale, data and theta must not be NULL");
    const size_t nn = (size_t)ntab * Q, nmu = nn * pl->det_C, nth = nn * (1 + pl->fit_K);
    return events_host(pl, R, ntab,
                       {{theta, nth, sizeof(double)}, {nll, nn, sizeof(double)}, {mu, nmu, sizeof(double)}, {status, nn, sizeof(int)}},
                       "response fit_fixed", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_fit_fixed(pl, dI, ntab, S, Q, scale, data, (double*)d[0], (double*)d[1],
                                                               (double*)d[2], (int*)d[3], nullptr);
                       });
}

// The limits on the signal's scale (nusi_detector.hip k_interval): with or without templates.
static int limit_check(const nusi_plan* pl, const double* data, double delta, int which, const void* lo, const void* hi)
{
    if (int r = detector_plan(pl, "response limit")) return r;
    if (!data) return fail(NUSI_EPARAM, "response limit: data must not be NULL");
    if (!std::isfinite(delta) || !(delta > 0.0)) return fail(NUSI_EPARAM, "response limit: delta must be finite and > 0");
    if (which < 1 || which > 3) return fail(NUSI_EPARAM, "response limit: which outside NUSI_LIMIT_LOWER | NUSI_LIMIT_UPPER");
    if (((which & NUSI_LIMIT_LOWER) && !lo) || ((which & NUSI_LIMIT_UPPER) && !hi))
        return fail(NUSI_EPARAM, "response limit: the output of a side asked for is NULL");
    return NUSI_OK;
}

int nusi_plan_response_limit(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* data,
                             double delta, int which, double* d_lo, double* d_hi, double* d_theta_hat, double* d_nll_hat,
                             int* d_status, void* stream)
{
    if (int r = limit_check(pl, data, delta, which, d_lo, d_hi)) return r;
    EventsArgs a;
    if (int r = events_begin(pl, "response limit", d_R, ntab, S, Q, nullptr, data, 1, stream, a)) return r;
    HIPCHECK(nusi::launch_detector_limit(pl->gd, d_R, ntab, a.S, Q, a.data, a.bg, pl->det_C, pl->fit_K, pl->d_tpl, pl->fit_m,
                                         pl->fit_w, delta, which, d_lo, d_hi, d_theta_hat, d_nll_hat, d_status, a.s));
    return detector_mark(pl, a.s);
}

int nusi_plan_response_limit_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* data,
                                  double delta, int which, double* lo, double* hi, double* theta_hat, double* nll_hat,
                                  int* status)
{
    if (int r = limit_check(pl, data, delta, which, lo, hi)) return r;
    if (!R || ntab < 1 || Q < 1) return fail(NUSI_EPARAM, "response limit: R must not be NULL, ntab and Q >= 1");
    const size_t nn = (size_t)ntab * Q, nth = nn * (1 + pl->fit_K);
    return events_host(pl, R, ntab,
                       {{lo, nn, sizeof(double)}, {hi, nn, sizeof(double)}, {theta_hat, nth, sizeof(double)},
                        {nll_hat, nn, sizeof(double)}, {status, 3 * nn, sizeof(int)}},
                       "response limit", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_limit(pl, dI, ntab, S, Q, data, delta, which, (double*)d[0], (double*)d[1],
                                                           (double*)d[2], (double*)d[3], (int*)d[4], nullptr);
                       });
}

// The limits of an ensemble and their bands (nusi_detector.hip k_toys_limit / k_toys_band).  A unit is one table and one
// block of QB spectra; a side asked for whose raw array the caller does not give keeps its limits in the plan's scratch,
// QB P doubles per unit, and the call runs in chunks of the units that fit the budget: per chunk one launch of each
// kernel, on the call's stream.  The p-slices of a chunk: NUSI_OPT_ENSEMBLE_PSLICES, or automatic by the ensemble's own
// rule (kEnsBlocksPerCU blocks per compute unit wanted, slices of at least kEnsSliceDatasets).
constexpr size_t kToysScratchBytes = kEnsScratchBytes;
constexpr int kToysChunkSpectra = 1 << 22;   // a chunk holds at most so many spectra (units QB): k_toys_limit's grid of units and
                                             // k_toys_band's of spectra, 256 threads a block, stay below 2^32 threads a launch
struct ToysPlan {
    int QB, units, upc, nscr;   // spectra per unit, units of the call, units per chunk, sides kept in scratch
    bool lo_scr, hi_scr;
};
static int toys_check(const nusi_plan* pl, const double* data, int P, double delta, int which, const int* rank, int NR,
                      const void* band_lo, const void* band_hi, const void* tally, const void* lo_all, const void* hi_all,
                      const void* words_all)
{
    if (int r = detector_plan(pl, "response ensemble_limit")) return r;
    if (!data) return fail(NUSI_EPARAM, "response ensemble_limit: data must not be NULL");
    if (P < 1 || P > NUSI_BAND_DATASETS_MAX) return fail(NUSI_EPARAM, "response ensemble_limit: P outside 1 .. NUSI_BAND_DATASETS_MAX");
    if (NR < 0 || NR > NUSI_BAND_RANKS_MAX) return fail(NUSI_EPARAM, "response ensemble_limit: NR outside 0 .. NUSI_BAND_RANKS_MAX");
    if (NR > 0 && !rank) return fail(NUSI_EPARAM, "response ensemble_limit: rank must not be NULL with NR > 0");
    for (int k = 0; k < NR; ++k)
        if (rank[k] < 0 || rank[k] >= P) return fail(NUSI_EPARAM, "response ensemble_limit: a rank outside 0 .. P - 1");
    if (!std::isfinite(delta) || !(delta > 0.0)) return fail(NUSI_EPARAM, "response ensemble_limit: delta must be finite and > 0");
    if (which < 1 || which > 3) return fail(NUSI_EPARAM, "response ensemble_limit: which outside NUSI_LIMIT_LOWER | NUSI_LIMIT_UPPER");
    if (NR > 0 && (((which & NUSI_LIMIT_LOWER) && !band_lo) || ((which & NUSI_LIMIT_UPPER) && !band_hi)))
        return fail(NUSI_EPARAM, "response ensemble_limit: the band of a side asked for is NULL");
    if (NR == 0 && !tally && !lo_all && !hi_all && !words_all)
        return fail(NUSI_EPARAM, "response ensemble_limit: NR = 0 and no tally or raw output: nothing to do");
    return NUSI_OK;
}
static int toys_plan(const nusi_plan* pl, int ntab, int Q, int P, int which, int NR, const void* lo_all, const void* hi_all,
                     ToysPlan& tp)
{
    tp.QB = nusi::toys_limit_block(pl->det_C);
    const long long nqb = (Q + tp.QB - 1) / tp.QB, units = (long long)ntab * nqb;
    if (units > (long long)INT_MAX / tp.QB) return fail(NUSI_EPARAM, "response ensemble_limit: too many spectra (ntab Q >= 2^31)");
    tp.units = (int)units;
    tp.lo_scr = NR > 0 && (which & NUSI_LIMIT_LOWER) && !lo_all;
    tp.hi_scr = NR > 0 && (which & NUSI_LIMIT_UPPER) && !hi_all;
    tp.nscr = (tp.lo_scr ? 1 : 0) + (tp.hi_scr ? 1 : 0);
    tp.upc = std::min(tp.units, std::max(kToysChunkSpectra / tp.QB, 1));   // (also with the raw arrays given)
    if (tp.nscr) {
        const size_t budget = pl->toys_b > 0 ? (size_t)pl->toys_b : pl->toys_mb > 0 ? (size_t)pl->toys_mb << 20 : kToysScratchBytes;
        const size_t per = (size_t)tp.QB * P * sizeof(double) * tp.nscr;
        if (budget < per)
            return fail(NUSI_EPARAM, "response ensemble_limit: NUSI_OPT_ENSEMBLE_LIMIT_MB / _BYTES is below one unit's scratch (QB P 8 bytes per side)");
        tp.upc = (int)std::min<size_t>(budget / per, (size_t)tp.upc);
    }
    return NUSI_OK;
}

int nusi_plan_response_ensemble_limit(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* data,
                                      int P, double delta, int which, const int* rank, int NR, double* d_band_lo,
                                      double* d_band_hi, int* d_tally, double* d_lo_all, double* d_hi_all, int* d_words_all,
                                      void* stream)
{
    if (int r = detector_plan(pl, "response ensemble_limit")) return r;
    if (!d_R || !S || ntab < 1 || Q < 1 || Q > (1 << 19))   // (events_check's, before Q enters toys_plan)
        return fail(NUSI_EPARAM, "response ensemble_limit: R and S must not be NULL, need ntab >= 1 and 1 <= Q <= 2^19");
    if (int r = toys_check(pl, data, P, delta, which, rank, NR, d_band_lo, d_band_hi, d_tally, d_lo_all, d_hi_all, d_words_all)) return r;
    ToysPlan tp;
    if (int r = toys_plan(pl, ntab, Q, P, which, NR, d_lo_all, d_hi_all, tp)) return r;
    EventsArgs a;
    if (int r = events_begin(pl, "response ensemble_limit", d_R, ntab, S, Q, nullptr, data, P, stream, a)) return r;
    // (every earlier detector call has finished: events_stage -- the scratch and the ranks are free)
    const size_t rows = (size_t)tp.upc * tp.QB, need = rows * P * sizeof(double) * tp.nscr;
    if (pl->toys_bytes < need) {
        hipFree(pl->d_toys);
        pl->d_toys = nullptr;
        pl->toys_bytes = 0;
        HIPCHECK(hipMalloc(&pl->d_toys, need));
        pl->toys_bytes = need;
    }
    if (NR > 0) {
        if (!pl->d_rank) HIPCHECK(hipMalloc(&pl->d_rank, sizeof(pl->h_rank)));
        memcpy(pl->h_rank, rank, sizeof(int) * NR);
        HIPCHECK(hipMemcpyAsync(pl->d_rank, pl->h_rank, sizeof(int) * NR, hipMemcpyHostToDevice, a.s));
    }
    const size_t nn = (size_t)ntab * Q;
    if (d_tally) HIPCHECK(hipMemsetAsync(d_tally, 0, sizeof(int) * nn * 8, a.s));
    double* lo = tp.lo_scr ? pl->d_toys : d_lo_all;
    double* hi = tp.hi_scr ? pl->d_toys + (tp.lo_scr ? rows * P : 0) : d_hi_all;
    int ncu = 0;
    HIPCHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device));
    const long long want = (long long)kEnsBlocksPerCU * (ncu > 0 ? ncu : 1);
    for (int u0 = 0; u0 < tp.units; u0 += tp.upc) {
        const int nu = std::min(tp.upc, tp.units - u0);
        const int ps = pl->ens_pslices > 0 ? std::min(pl->ens_pslices, P)
                                           : (int)std::min<long long>(std::max(P / kEnsSliceDatasets, 1), (want + nu - 1) / nu);
        HIPCHECK(nusi::launch_toys_limit(pl->gd, d_R, a.S, Q, a.data, P, a.bg, pl->det_C, pl->fit_K, pl->d_tpl, pl->fit_m,
                                         pl->fit_w, delta, which, u0, nu, ps, lo, tp.lo_scr, hi, tp.hi_scr, d_words_all, d_tally,
                                         a.s));
        if (NR > 0)
            HIPCHECK(nusi::launch_toys_band(pl->det_C, Q, P, u0, nu, lo, tp.lo_scr, hi, tp.hi_scr, d_band_lo, d_band_hi,
                                            pl->d_rank, NR, a.s));
    }
    return detector_mark(pl, a.s);
}

int nusi_plan_response_ensemble_limit_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* data,
                                           int P, double delta, int which, const int* rank, int NR, double* band_lo,
                                           double* band_hi, int* tally, double* lo_all, double* hi_all, int* words_all)
{
    if (int r = toys_check(pl, data, P, delta, which, rank, NR, band_lo, band_hi, tally, lo_all, hi_all, words_all)) return r;
    if (!R || !S || ntab < 1 || Q < 1 || Q > (1 << 19))
        return fail(NUSI_EPARAM, "response ensemble_limit: R and S must not be NULL, need ntab >= 1 and 1 <= Q <= 2^19");
    ToysPlan tp;   // (the budget's refusal too, before the device buffers)
    if (int r = toys_plan(pl, ntab, Q, P, which, NR, lo_all, hi_all, tp)) return r;
    const size_t nn = (size_t)ntab * Q;
    return events_host(pl, R, ntab,
                       {{band_lo, nn * NR, sizeof(double)}, {band_hi, nn * NR, sizeof(double)}, {tally, nn * 8, sizeof(int)},
                        {lo_all, nn * P, sizeof(double)}, {hi_all, nn * P, sizeof(double)}, {words_all, nn * P * 2, sizeof(int)}},
                       "response ensemble_limit", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_ensemble_limit(pl, dI, ntab, S, Q, data, P, delta, which, rank, NR,
                                                                    (double*)d[0], (double*)d[1], (int*)d[2], (double*)d[3],
                                                                    (double*)d[4], (int*)d[5], nullptr);
                       });
}

// nusi_plan_draw_counts: the checks, then mu staged into the plan's d_draw on s (the earlier draw has finished with it)
static int draw_check(const nusi_plan* pl, const double* mu, int rows, int C, int P, const void* out)
{
    if (!pl) return no_plan();
    if (!mu || !out) return fail(NUSI_EPARAM, "draw counts: mu and the output must not be NULL");
    if (rows < 1 || C < 1 || C > NUSI_DETECTOR_BINS_MAX || P < 1 || P > NUSI_DRAW_DATASETS_MAX)
        return fail(NUSI_EPARAM, "draw counts: need rows >= 1, 1 <= C <= NUSI_DETECTOR_BINS_MAX and 1 <= P <= NUSI_DRAW_DATASETS_MAX");
    if ((unsigned long long)rows * P * C > (unsigned long long)NUSI_DRAW_COUNTS_MAX)
        return fail(NUSI_EPARAM, "draw counts: rows P C above NUSI_DRAW_COUNTS_MAX");
    for (size_t e = 0; e < (size_t)rows * C; ++e)
        if (!(mu[e] >= 0.0) || !std::isfinite(mu[e])) return fail(NUSI_EPARAM, "draw counts: an expectation is negative or not finite");
    return NUSI_OK;
}

int nusi_plan_draw_counts(nusi_plan* pl, const double* mu, int rows, int C, int P, unsigned long long seed, unsigned stream_id,
                          double* d_out, void* stream)
{
    if (int r = draw_check(pl, mu, rows, C, P, d_out)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    if (pl->draw_ran) HIPCHECK(hipEventSynchronize(pl->ev_draw));
    const size_t need = (size_t)rows * C;
    if (pl->draw_doubles < need) {
        hipFree(pl->d_draw);
        pl->d_draw = nullptr;
        pl->draw_doubles = 0;
        HIPCHECK(hipMalloc(&pl->d_draw, sizeof(double) * need));
        pl->draw_doubles = need;
    }
    pl->h_draw.assign(mu, mu + need);
    HIPCHECK(hipMemcpyAsync(pl->d_draw, pl->h_draw.data(), sizeof(double) * need, hipMemcpyHostToDevice, s));
    HIPCHECK(nusi::launch_poisson_draw(pl->d_draw, rows, C, P, seed, stream_id, d_out, s));
    if (!pl->ev_draw) HIPCHECK(hipEventCreateWithFlags(&pl->ev_draw, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(pl->ev_draw, s));
    pl->draw_ran = true;
    return NUSI_OK;
}

int nusi_plan_draw_counts_host(nusi_plan* pl, const double* mu, int rows, int C, int P, unsigned long long seed,
                               unsigned stream_id, double* out)
{
    if (int r = draw_check(pl, mu, rows, C, P, out)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    const size_t n = (size_t)rows * P * C;
    double* dO = nullptr;
    if (hipMalloc(&dO, sizeof(double) * n) != hipSuccess) return fail(NUSI_EHIP, "draw counts: no device memory");
    int r = nusi_plan_draw_counts(pl, mu, rows, C, P, seed, stream_id, dO, nullptr);
    if (!r && hipStreamSynchronize(pl->stream) != hipSuccess) r = fail(NUSI_EHIP, "draw counts: the stream failed");
    if (!r && hipMemcpy(out, dO, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess)
        r = fail(NUSI_EHIP, "draw counts: copy to the host failed");
    hipFree(dO);
    return r;
}

// nusi_plan_draw_normals: nusi_plan_draw_counts' checks, staging (center, then sigma, in d_draw) and ordering
static int normals_check(const nusi_plan* pl, const double* center, const double* sigma, int rows, int J, int P, const void* out)
{
    if (!pl) return no_plan();
    if (!center || !sigma || !out) return fail(NUSI_EPARAM, "draw normals: center, sigma and the output must not be NULL");
    if (rows < 1 || J < 1 || J > NUSI_DETECTOR_BINS_MAX || P < 1 || P > NUSI_DRAW_DATASETS_MAX)
        return fail(NUSI_EPARAM, "draw normals: need rows >= 1, 1 <= J <= NUSI_DETECTOR_BINS_MAX and 1 <= P <= NUSI_DRAW_DATASETS_MAX");
    if ((unsigned long long)rows * P * J > (unsigned long long)NUSI_DRAW_COUNTS_MAX)
        return fail(NUSI_EPARAM, "draw normals: rows P J above NUSI_DRAW_COUNTS_MAX");
    for (size_t e = 0; e < (size_t)rows * J; ++e)
        if (!(center[e] >= 0.0) || !std::isfinite(center[e])) return fail(NUSI_EPARAM, "draw normals: a center is negative or not finite");
    for (int j = 0; j < J; ++j)
        if (!(sigma[j] > 0.0)) return fail(NUSI_EPARAM, "draw normals: a sigma is NaN or not > 0");
    return NUSI_OK;
}

int nusi_plan_draw_normals(nusi_plan* pl, const double* center, const double* sigma, int rows, int J, int P,
                           unsigned long long seed, unsigned stream_id, double* d_out, void* stream)
{
    if (int r = normals_check(pl, center, sigma, rows, J, P, d_out)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    if (pl->draw_ran) HIPCHECK(hipEventSynchronize(pl->ev_draw));
    const size_t nc = (size_t)rows * J, need = nc + (size_t)J;
    if (pl->draw_doubles < need) {
        hipFree(pl->d_draw);
        pl->d_draw = nullptr;
        pl->draw_doubles = 0;
        HIPCHECK(hipMalloc(&pl->d_draw, sizeof(double) * need));
        pl->draw_doubles = need;
    }
    pl->h_draw.assign(center, center + nc);
    pl->h_draw.insert(pl->h_draw.end(), sigma, sigma + J);
    HIPCHECK(hipMemcpyAsync(pl->d_draw, pl->h_draw.data(), sizeof(double) * need, hipMemcpyHostToDevice, s));
    HIPCHECK(nusi::launch_normal_draw(pl->d_draw, rows, J, P, seed, stream_id, d_out, s));
    if (!pl->ev_draw) HIPCHECK(hipEventCreateWithFlags(&pl->ev_draw, hipEventDisableTiming));
    HIPCHECK(hipEventRecord(pl->ev_draw, s));
    pl->draw_ran = true;
    return NUSI_OK;
}

int nusi_plan_draw_normals_host(nusi_plan* pl, const double* center, const double* sigma, int rows, int J, int P,
                                unsigned long long seed, unsigned stream_id, double* out)
{
    if (int r = normals_check(pl, center, sigma, rows, J, P, out)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    const size_t n = (size_t)rows * P * J;
    double* dO = nullptr;
    if (hipMalloc(&dO, sizeof(double) * n) != hipSuccess) return fail(NUSI_EHIP, "draw normals: no device memory");
    int r = nusi_plan_draw_normals(pl, center, sigma, rows, J, P, seed, stream_id, dO, nullptr);
    if (!r && hipStreamSynchronize(pl->stream) != hipSuccess) r = fail(NUSI_EHIP, "draw normals: the stream failed");
    if (!r && hipMemcpy(out, dO, sizeof(double) * n, hipMemcpyDeviceToHost) != hipSuccess)
        r = fail(NUSI_EHIP, "draw normals: copy to the host failed");
    hipFree(dO);
    return r;
}

// The calibration call (nusi_detector.hip k_inject, then k_toys_band): the ensemble limit's units, chunks, scratch budget
// and p-slices; the toys are drawn in the kernel.  The host vectors ride in d_evt behind the spectra (evt_layout): a_inj
// in the scales' place, then a_test [Q] and q_obs [ntab][Q] (with exceed) as the extra vectors.
struct InjectPlan {
    int QB, units, upc, nscr;
    bool th_scr, st_scr;
};
static int inject_check(const nusi_plan* pl, const void* R, int ntab, const double* S, int Q, const double* a_inj,
                        const double* theta_inj, const double* a_test, int P, int mode, const int* rank, int NR,
                        const double* q_obs, const void* band_theta, const void* band_stat, const void* tally,
                        const void* exceed, const void* theta_all, const void* stat_all, const void* words_all,
                        const void* data_all)
{
    const std::string w = "response inject: ";
    if (int r = detector_plan(pl, "response inject")) return r;
    if (!R || !S || !a_inj) return fail(NUSI_EPARAM, w + "R, S and a_inj must not be NULL");
    if (ntab < 1 || Q < 1 || Q > (1 << 19)) return fail(NUSI_EPARAM, w + "need ntab >= 1 and 1 <= Q <= 2^19");
    if (P < 1 || P > NUSI_BAND_DATASETS_MAX) return fail(NUSI_EPARAM, w + "P outside 1 .. NUSI_BAND_DATASETS_MAX");
    if (NR < 0 || NR > NUSI_BAND_RANKS_MAX) return fail(NUSI_EPARAM, w + "NR outside 0 .. NUSI_BAND_RANKS_MAX");
    if (NR > 0 && !rank) return fail(NUSI_EPARAM, w + "rank must not be NULL with NR > 0");
    for (int k = 0; k < NR; ++k)
        if (rank[k] < 0 || rank[k] >= P) return fail(NUSI_EPARAM, w + "a rank outside 0 .. P - 1");
    if (mode < NUSI_INJECT_TWO_SIDED || mode > NUSI_INJECT_DISCOVERY) return fail(NUSI_EPARAM, w + "mode outside 0 .. 2");
    if (NR > 0 && !band_theta && !band_stat) return fail(NUSI_EPARAM, w + "NR > 0 needs a band");
    if ((q_obs != nullptr) != (exceed != nullptr)) return fail(NUSI_EPARAM, w + "q_obs and exceed come together");
    if (NR == 0 && !tally && !exceed && !theta_all && !stat_all && !words_all && !data_all)
        return fail(NUSI_EPARAM, w + "NR = 0 and no tally, exceed or raw output: nothing to do");
    for (int q = 0; q < Q; ++q) {
        if (!(a_inj[q] >= 0.0) || !std::isfinite(a_inj[q])) return fail(NUSI_EPARAM, w + "an a_inj is negative or not finite");
        if (a_test && (!(a_test[q] >= 0.0) || !std::isfinite(a_test[q]))) return fail(NUSI_EPARAM, w + "an a_test is negative or not finite");
    }
    if (theta_inj)
        for (int j = 0; j < pl->fit_K; ++j)
            if (!(theta_inj[j] >= 0.0) || !std::isfinite(theta_inj[j])) return fail(NUSI_EPARAM, w + "a theta_inj is negative or not finite");
    return NUSI_OK;
}
static int inject_plan(const nusi_plan* pl, int ntab, int Q, int P, int NR, const void* band_theta, const void* band_stat,
                       const void* theta_all, const void* stat_all, InjectPlan& ip)
{
    ip.QB = nusi::toys_limit_block(pl->det_C);
    const long long nqb = (Q + ip.QB - 1) / ip.QB, units = (long long)ntab * nqb;
    if (units > (long long)INT_MAX / ip.QB) return fail(NUSI_EPARAM, "response inject: too many spectra (ntab Q >= 2^31)");
    ip.units = (int)units;
    ip.th_scr = NR > 0 && band_theta && !theta_all;
    ip.st_scr = NR > 0 && band_stat && !stat_all;
    ip.nscr = (ip.th_scr ? 1 : 0) + (ip.st_scr ? 1 : 0);
    ip.upc = std::min(ip.units, std::max(kToysChunkSpectra / ip.QB, 1));   // (also with the raw arrays given)
    if (ip.nscr) {
        const size_t budget = pl->toys_b > 0 ? (size_t)pl->toys_b : pl->toys_mb > 0 ? (size_t)pl->toys_mb << 20 : kToysScratchBytes;
        const size_t per = (size_t)ip.QB * P * sizeof(double) * ip.nscr;
        if (budget < per)
            return fail(NUSI_EPARAM, "response inject: NUSI_OPT_ENSEMBLE_LIMIT_MB / _BYTES is below one unit's scratch (QB P 8 bytes per series)");
        ip.upc = (int)std::min<size_t>(budget / per, (size_t)ip.upc);
    }
    return NUSI_OK;
}

int nusi_plan_response_inject(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* a_inj,
                              const double* theta_inj, const double* a_test, int P, unsigned long long seed, int mode,
                              const int* rank, int NR, const double* q_obs, double* d_band_theta, double* d_band_stat,
                              int* d_tally, int* d_exceed, double* d_theta_all, double* d_stat_all, int* d_words_all,
                              double* d_data_all, void* stream)
{
    if (int r = inject_check(pl, d_R, ntab, S, Q, a_inj, theta_inj, a_test, P, mode, rank, NR, q_obs, d_band_theta, d_band_stat,
                             d_tally, d_exceed, d_theta_all, d_stat_all, d_words_all, d_data_all))
        return r;
    InjectPlan ip;
    if (int r = inject_plan(pl, ntab, Q, P, NR, d_band_theta, d_band_stat, d_theta_all, d_stat_all, ip)) return r;
    const size_t nn = (size_t)ntab * Q;
    // a_test [Q] and q_obs [ntab][Q] travel behind the spectra and a_inj as events_stage's extra vectors (evt_layout)
    std::vector<double> extra((size_t)Q + (q_obs ? nn : 0));
    memcpy(extra.data(), a_test ? a_test : a_inj, sizeof(double) * Q);
    if (q_obs) memcpy(extra.data() + Q, q_obs, sizeof(double) * nn);
    if (int r = events_check(pl, "response inject", d_R, ntab, S, Q, a_inj, nullptr, 0)) return r;
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    const int C = pl->det_C;
    if (int r = events_stage(pl, S, Q, a_inj, nullptr, 0, s, extra.data(), extra.size())) return r;
    const EvtLayout l = evt_layout(pl, Q, 0, extra.size());
    const double* dS = pl->d_evt;
    const double* d_ainj = pl->d_evt + l.scale;
    const double* d_atest = pl->d_evt + l.extra;
    const double* d_qobs = q_obs ? d_atest + Q : nullptr;
    // (every earlier detector call has finished: events_stage -- the scratch and the ranks are free)
    const size_t rows = (size_t)ip.upc * ip.QB, need = rows * P * sizeof(double) * ip.nscr;
    if (pl->toys_bytes < need) {
        hipFree(pl->d_toys);
        pl->d_toys = nullptr;
        pl->toys_bytes = 0;
        HIPCHECK(hipMalloc(&pl->d_toys, need));
        pl->toys_bytes = need;
    }
    if (NR > 0) {
        if (!pl->d_rank) HIPCHECK(hipMalloc(&pl->d_rank, sizeof(pl->h_rank)));
        memcpy(pl->h_rank, rank, sizeof(int) * NR);
        HIPCHECK(hipMemcpyAsync(pl->d_rank, pl->h_rank, sizeof(int) * NR, hipMemcpyHostToDevice, s));
    }
    if (d_tally) HIPCHECK(hipMemsetAsync(d_tally, 0, sizeof(int) * nn * 4, s));
    if (d_exceed) HIPCHECK(hipMemsetAsync(d_exceed, 0, sizeof(int) * nn, s));
    // a series is kept where its band or its raw array is asked for
    double* th = ip.th_scr ? pl->d_toys : d_theta_all;
    double* st = ip.st_scr ? pl->d_toys + (ip.th_scr ? rows * P : 0) : d_stat_all;
    double th_inj[NUSI_FIT_TEMPLATES_MAX] = {};
    for (int j = 0; j < pl->fit_K; ++j) th_inj[j] = theta_inj ? theta_inj[j] : pl->fit_m[j];
    int ncu = 0;
    HIPCHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device));
    const long long want = (long long)kEnsBlocksPerCU * (ncu > 0 ? ncu : 1);
    for (int u0 = 0; u0 < ip.units; u0 += ip.upc) {
        const int nu = std::min(ip.upc, ip.units - u0);
        const int ps = pl->ens_pslices > 0 ? std::min(pl->ens_pslices, P)
                                           : (int)std::min<long long>(std::max(P / kEnsSliceDatasets, 1), (want + nu - 1) / nu);
        HIPCHECK(nusi::launch_inject(pl->gd, d_R, dS, Q, d_ainj, d_atest, th_inj, d_qobs, P, seed, mode, detector_bg(pl), C,
                                     pl->fit_K, pl->d_tpl, pl->fit_m, pl->fit_w, pl->fit_s, pl->toy_nuis, u0, nu, ps, th, ip.th_scr, st, ip.st_scr,
                                     d_words_all, d_tally, d_exceed, d_data_all, s));
        if (NR > 0)
            HIPCHECK(nusi::launch_toys_band(C, Q, P, u0, nu, d_band_theta ? th : nullptr, ip.th_scr, d_band_stat ? st : nullptr,
                                            ip.st_scr, d_band_theta, d_band_stat, pl->d_rank, NR, s));
    }
    return detector_mark(pl, s);
}

int nusi_plan_response_inject_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* a_inj,
                                   const double* theta_inj, const double* a_test, int P, unsigned long long seed, int mode,
                                   const int* rank, int NR, const double* q_obs, double* band_theta, double* band_stat,
                                   int* tally, int* exceed, double* theta_all, double* stat_all, int* words_all,
                                   double* data_all)
{
    if (int r = inject_check(pl, R, ntab, S, Q, a_inj, theta_inj, a_test, P, mode, rank, NR, q_obs, band_theta, band_stat, tally,
                             exceed, theta_all, stat_all, words_all, data_all))
        return r;
    InjectPlan ip;   // (the budget's refusal too, before the device buffers)
    if (int r = inject_plan(pl, ntab, Q, P, NR, band_theta, band_stat, theta_all, stat_all, ip)) return r;
    const size_t nn = (size_t)ntab * Q;
    return events_host(pl, R, ntab,
                       {{band_theta, nn * NR, sizeof(double)}, {band_stat, nn * NR, sizeof(double)}, {tally, nn * 4, sizeof(int)},
                        {exceed, nn, sizeof(int)}, {theta_all, nn * P, sizeof(double)}, {stat_all, nn * P, sizeof(double)},
                        {words_all, nn * P * 2, sizeof(int)}, {data_all, nn * P * pl->det_C, sizeof(double)}},
                       "response inject", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_inject(pl, dI, ntab, S, Q, a_inj, theta_inj, a_test, P, seed, mode, rank, NR,
                                                            q_obs, (double*)d[0], (double*)d[1], (int*)d[2], (int*)d[3],
                                                            (double*)d[4], (double*)d[5], (int*)d[6], (double*)d[7], nullptr);
                       });
}

// The toy-calibrated interval (nusi_detector.hip k_belt, then k_belt_accept).  The size limits are a pure function, which
// the call applies with the detector's C.  data rides in events_stage's data slot (P = 1), frac [G] and ref [ntab][Q]
// (where given) as its extra vectors.  The interval needs exceed, tally and words_obs: one the caller does not give
// lives in the plan's scratch (d_toys), and the call then runs in chunks of whole (t, q) pairs.
int nusi_belt_shape(int C, int ntab, int Q, int G, int P, long long* units)
{
    const std::string w = "response belt: ";
    if (C < 1 || C > NUSI_DETECTOR_BINS_MAX) return fail(NUSI_EPARAM, w + "C outside 1 .. NUSI_DETECTOR_BINS_MAX");
    if (ntab < 1 || Q < 1 || Q > (1 << 19)) return fail(NUSI_EPARAM, w + "need ntab >= 1 and 1 <= Q <= 2^19");
    if (G < 1 || G > NUSI_BELT_GRID_MAX) return fail(NUSI_EPARAM, w + "G outside 1 .. NUSI_BELT_GRID_MAX");
    if (P < 1 || P > NUSI_DRAW_DATASETS_MAX) return fail(NUSI_EPARAM, w + "P outside 1 .. NUSI_DRAW_DATASETS_MAX");
    const long long rows = (long long)Q * G;   // (<= 2^25)
    if ((long long)ntab * rows >= (1ll << 31)) return fail(NUSI_EPARAM, w + "too many records (ntab Q G >= 2^31)");
    const long long QB = nusi::belt_block(C);
    if (units) *units = (long long)ntab * ((rows + QB - 1) / QB);
    return NUSI_OK;
}

struct BeltPlan {
    int pairs, ppc;                       // the (t, q) pairs of the call and of a chunk
    bool accept, ex_scr, ty_scr, wo_scr;  // the interval is asked for; what it needs from the scratch
    size_t per;                           // the scratch's bytes a pair
};
static int belt_check(const nusi_plan* pl, const void* R, int ntab, const double* S, int Q, const double* data,
                      const double* frac, int G, int P, int mode, double alpha, bool any_out)
{
    const std::string w = "response belt: ";
    if (int r = detector_plan(pl, "response belt")) return r;
    if (int r = nusi_belt_shape(pl->det_C, ntab, Q, G, P, nullptr)) return r;
    if (pl->toy_nuis == NUSI_TOYS_PRIOR)
        return fail(NUSI_EPARAM, w + "NUSI_OPT_TOY_NUISANCE = NUSI_TOYS_PRIOR: the profile construction has no such variant (FIXED or GLOBAL)");
    if (!R || !S || !data || !frac) return fail(NUSI_EPARAM, w + "R, S, data and frac must not be NULL");
    for (int g = 0; g < G; ++g)
        if (!(frac[g] >= 0.0) || !std::isfinite(frac[g]) || (g > 0 && !(frac[g] > frac[g - 1])))
            return fail(NUSI_EPARAM, w + "frac must be finite, >= 0 and strictly ascending");
    if (mode != NUSI_INJECT_TWO_SIDED && mode != NUSI_INJECT_UPPER)
        return fail(NUSI_EPARAM, w + "mode must be NUSI_INJECT_TWO_SIDED or NUSI_INJECT_UPPER");
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(NUSI_EPARAM, w + "alpha must lie in (0, 1)");
    if (!any_out) return fail(NUSI_EPARAM, w + "every output is NULL: nothing to do");
    return events_check(pl, "response belt", (const double*)R, ntab, S, Q, nullptr, data, 1);
}
static int belt_plan(const nusi_plan* pl, int ntab, int Q, int G, bool accept, const void* exceed, const void* tally,
                     const void* words_obs, BeltPlan& bp)
{
    bp.pairs = ntab * Q;   // (< 2^31: nusi_belt_shape)
    bp.accept = accept;
    bp.ex_scr = accept && !exceed;
    bp.ty_scr = accept && !tally;
    bp.wo_scr = accept && !words_obs;
    bp.per = sizeof(int) * ((bp.ex_scr ? (size_t)G : 0) + (bp.ty_scr ? (size_t)4 * G : 0) + (bp.wo_scr ? (size_t)G + 1 : 0));
    bp.ppc = std::min(bp.pairs, std::max(kToysChunkSpectra / G, 1));   // (also with every array given)
    if (bp.per) {
        const size_t budget = pl->toys_b > 0 ? (size_t)pl->toys_b : pl->toys_mb > 0 ? (size_t)pl->toys_mb << 20 : kToysScratchBytes;
        if (budget < bp.per)
            return fail(NUSI_EPARAM, "response belt: NUSI_OPT_ENSEMBLE_LIMIT_MB / _BYTES is below one (t, q) pair's scratch (4 G, 16 G and 4 (1 + G) bytes for exceed, tally and words_obs)");
        bp.ppc = (int)std::min<size_t>(budget / bp.per, (size_t)bp.ppc);
    }
    return NUSI_OK;
}

int nusi_plan_response_belt(nusi_plan* pl, const double* d_R, int ntab, const double* S, int Q, const double* data,
                            const double* frac, int G, const double* ref, int P, unsigned long long seed, int mode,
                            double alpha, double* d_lo, double* d_hi, int* d_idx, int* d_status, int* d_exceed, int* d_tally,
                            double* d_q_obs, double* d_theta_obs, int* d_words_obs, double* d_theta_all, double* d_stat_all,
                            int* d_words_all, double* d_data_all, void* stream)
{
    const bool accept = d_lo || d_hi || d_idx || d_status;
    const bool any_out = accept || d_exceed || d_tally || d_q_obs || d_theta_obs || d_words_obs || d_theta_all || d_stat_all ||
                         d_words_all || d_data_all;
    if (int r = belt_check(pl, d_R, ntab, S, Q, data, frac, G, P, mode, alpha, any_out)) return r;
    BeltPlan bp;
    if (int r = belt_plan(pl, ntab, Q, G, accept, d_exceed, d_tally, d_words_obs, bp)) return r;
    const size_t nn = (size_t)ntab * Q;
    std::vector<double> extra((size_t)G + (ref ? nn : 0));
    memcpy(extra.data(), frac, sizeof(double) * G);
    if (ref) memcpy(extra.data() + G, ref, sizeof(double) * nn);
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    const int C = pl->det_C;
    if (int r = events_stage(pl, S, Q, nullptr, data, 1, s, extra.data(), extra.size())) return r;
    const EvtLayout l = evt_layout(pl, Q, 1, extra.size());
    const double* dS = pl->d_evt;
    const double* d_data = pl->d_evt + l.data;
    const double* d_frac = pl->d_evt + l.extra;
    const double* d_ref = ref ? d_frac + G : nullptr;
    // (every earlier detector call has finished: events_stage -- the scratch is free)
    const size_t need = bp.per * (size_t)bp.ppc;
    if (pl->toys_bytes < need) {
        hipFree(pl->d_toys);
        pl->d_toys = nullptr;
        pl->toys_bytes = 0;
        HIPCHECK(hipMalloc(&pl->d_toys, need));
        pl->toys_bytes = need;
    }
    // the scratch of a chunk: exceed [ppc][G], tally [ppc][G][4], words_obs [ppc][1 + G], those of them that live there
    int* scr = (int*)pl->d_toys;
    int* ex = d_exceed;
    int* ty = d_tally;
    int* wo = d_words_obs;
    size_t off = 0;
    if (bp.ex_scr) ex = scr + off, off += (size_t)bp.ppc * G;
    if (bp.ty_scr) ty = scr + off, off += (size_t)bp.ppc * G * 4;
    if (bp.wo_scr) wo = scr + off, off += (size_t)bp.ppc * (G + 1);
    if (d_exceed) HIPCHECK(hipMemsetAsync(d_exceed, 0, sizeof(int) * nn * G, s));
    if (d_tally) HIPCHECK(hipMemsetAsync(d_tally, 0, sizeof(int) * nn * G * 4, s));
    int ncu = 0;
    HIPCHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device));
    const long long want = (long long)kEnsBlocksPerCU * (ncu > 0 ? ncu : 1);
    const int QB = nusi::belt_block(C);
    for (int pr0 = 0; pr0 < bp.pairs; pr0 += bp.ppc) {
        const int pr1 = pr0 + std::min(bp.ppc, bp.pairs - pr0);
        const long long nu = ((long long)(pr1 - pr0) * G + QB - 1) / QB;
        const int ps = pl->ens_pslices > 0 ? std::min(pl->ens_pslices, P)
                                           : (int)std::min<long long>(std::max(P / kEnsSliceDatasets, 1), (want + nu - 1) / nu);
        if (bp.ex_scr || bp.ty_scr)   // (the counts in the scratch are one block: exceed, then tally)
            HIPCHECK(hipMemsetAsync(scr, 0, sizeof(int) * (size_t)bp.ppc * G * ((bp.ex_scr ? 1 : 0) + (bp.ty_scr ? 4 : 0)), s));
        HIPCHECK(nusi::launch_belt(pl->gd, d_R, dS, Q, d_data, d_frac, G, d_ref, P, seed, mode, detector_bg(pl), C, pl->fit_K,
                                   pl->d_tpl, pl->fit_m, pl->fit_w, pl->fit_s, pl->toy_nuis, pr0, pr1, ps, ex, bp.ex_scr, ty, bp.ty_scr, wo, bp.wo_scr,
                                   d_q_obs, d_theta_obs, d_theta_all, d_stat_all, d_words_all, d_data_all, s));
        if (accept)
            HIPCHECK(nusi::launch_belt_accept(d_frac, G, d_ref, P, alpha, pr0, pr1, ex, bp.ex_scr, ty, bp.ty_scr, wo, bp.wo_scr,
                                              d_lo, d_hi, d_idx, d_status, s));
    }
    return detector_mark(pl, s);
}

int nusi_plan_response_belt_host(nusi_plan* pl, const double* R, int ntab, const double* S, int Q, const double* data,
                                 const double* frac, int G, const double* ref, int P, unsigned long long seed, int mode,
                                 double alpha, double* lo, double* hi, int* idx, int* status, int* exceed, int* tally,
                                 double* q_obs, double* theta_obs, int* words_obs, double* theta_all, double* stat_all,
                                 int* words_all, double* data_all)
{
    const bool accept = lo || hi || idx || status;
    const bool any_out = accept || exceed || tally || q_obs || theta_obs || words_obs || theta_all || stat_all || words_all ||
                         data_all;
    if (int r = belt_check(pl, R, ntab, S, Q, data, frac, G, P, mode, alpha, any_out)) return r;
    BeltPlan bp;   // (the budget's refusal too, before the device buffers)
    if (int r = belt_plan(pl, ntab, Q, G, accept, exceed, tally, words_obs, bp)) return r;
    const size_t nn = (size_t)ntab * Q, ng = nn * G, NC = (size_t)pl->fit_K + 1;
    return events_host(pl, R, ntab,
                       {{lo, nn, sizeof(double)}, {hi, nn, sizeof(double)}, {idx, nn * 2, sizeof(int)}, {status, nn, sizeof(int)},
                        {exceed, ng, sizeof(int)}, {tally, ng * 4, sizeof(int)}, {q_obs, ng, sizeof(double)},
                        {theta_obs, nn * (G + 1) * NC, sizeof(double)}, {words_obs, nn * (G + 1), sizeof(int)},
                        {theta_all, ng * P, sizeof(double)}, {stat_all, ng * P, sizeof(double)},
                        {words_all, ng * P * 2, sizeof(int)}, {data_all, ng * P * pl->det_C, sizeof(double)}},
                       "response belt", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_belt(pl, dI, ntab, S, Q, data, frac, G, ref, P, seed, mode, alpha,
                                                          (double*)d[0], (double*)d[1], (int*)d[2], (int*)d[3], (int*)d[4],
                                                          (int*)d[5], (double*)d[6], (double*)d[7], (int*)d[8], (double*)d[9],
                                                          (double*)d[10], (int*)d[11], (double*)d[12], nullptr);
                       });
}

// The toy-calibrated region of the flavour composition (nusi_detector.hip k_composition_belt, then
// k_composition_accept).  The size limits are a pure function, which the call applies with the detector's C and the
// plan's K.  data rides in events_stage's data slot (P = 1) and phi as its extra vector.  No plan scratch: the mask needs
// exceed, tally, q_obs and words_obs from the caller.
int nusi_composition_belt_shape(int C, int K, int ntab, int Q, int G, int P, long long* units)
{
    const std::string w = "response composition belt: ";
    if (C < 1 || C > NUSI_DETECTOR_BINS_MAX) return fail(NUSI_EPARAM, w + "C outside 1 .. NUSI_DETECTOR_BINS_MAX");
    if (K < 0 || K > NUSI_FIT_TEMPLATES_MAX) return fail(NUSI_EPARAM, w + "K outside 0 .. NUSI_FIT_TEMPLATES_MAX");
    if (ntab < 1 || Q < 1 || Q > (1 << 19)) return fail(NUSI_EPARAM, w + "need ntab >= 1 and 1 <= Q <= 2^19");
    if (G < 1 || G > NUSI_REGION_GRID_MAX) return fail(NUSI_EPARAM, w + "G outside 1 .. NUSI_REGION_GRID_MAX");
    if (P < 1 || P > NUSI_DRAW_DATASETS_MAX) return fail(NUSI_EPARAM, w + "P outside 1 .. NUSI_DRAW_DATASETS_MAX");
    const long long rows = (long long)Q * G;   // (<= 2^29)
    if ((long long)ntab * rows >= (1ll << 31)) return fail(NUSI_EPARAM, w + "too many records (ntab Q G >= 2^31)");
    // (theta_obs [ntab][Q][1 + G][3 + K] is the widest of the observed side's outputs; ntab Q (1 + G) < 2^32, 3 + K <= 6)
    if ((long long)ntab * Q * (1 + G) * (3 + K) >= (1ll << 31))
        return fail(NUSI_EPARAM, w + "too many records (an output's elements, ntab Q (1 + G) (3 + K), >= 2^31)");
    const long long QB = nusi::composition_belt_block(C);
    if (units) *units = (long long)ntab * ((rows + QB - 1) / QB);
    return NUSI_OK;
}

static int composition_belt_check(const nusi_plan* pl, const void* R3, int ntab, const double* S, int Q, const double* data,
                                  const double* phi, int phi_tables, int G, int P, double alpha, bool any_out, bool mask,
                                  bool mask_inputs)
{
    const std::string w = "response composition belt: ";
    if (int r = detector_plan(pl, "response composition belt")) return r;
    if (int r = nusi_composition_belt_shape(pl->det_C, pl->fit_K, ntab, Q, G, P, nullptr)) return r;
    if (pl->toy_nuis != NUSI_TOYS_FIXED) {
        bool constrained = false;
        for (int j = 0; j < pl->fit_K; ++j) constrained = constrained || pl->fit_w[j] > 0.0;
        if (constrained)
            return fail(NUSI_EPARAM, w + "NUSI_OPT_TOY_NUISANCE is not NUSI_TOYS_FIXED and a template is constrained: only the FIXED toy ensemble is built");
    }
    if (!R3 || !S || !data || !phi) return fail(NUSI_EPARAM, w + "R3, S, data and phi must not be NULL");
    const size_t np = (size_t)(phi_tables ? ntab : 1) * G;
    for (size_t e = 0; e < np; ++e) {
        const double* f = phi + 3 * e;
        for (int j = 0; j < 3; ++j)
            if (!(f[j] >= 0.0) || !std::isfinite(f[j])) return fail(NUSI_EPARAM, w + "an entry of phi is negative or not finite");
        if (f[0] == 0.0 && f[1] == 0.0 && f[2] == 0.0) return fail(NUSI_EPARAM, w + "a point of phi has all three weights zero");
    }
    if (!(alpha > 0.0 && alpha < 1.0)) return fail(NUSI_EPARAM, w + "alpha must lie in (0, 1)");
    if (!any_out) return fail(NUSI_EPARAM, w + "every output is NULL: nothing to do");
    if (mask && !mask_inputs) return fail(NUSI_EPARAM, w + "accept, status and best need exceed, tally, q_obs and words_obs");
    return events_check(pl, "response composition belt", (const double*)R3, ntab, S, Q, nullptr, data, 1);
}

int nusi_plan_response_composition_belt(nusi_plan* pl, const double* d_R3, int ntab, const double* S, int Q, const double* data,
                                        const double* phi, int phi_tables, int G, int P, unsigned long long seed, double alpha,
                                        int* d_accept, int* d_status, int* d_best, int* d_exceed, int* d_tally, double* d_q_obs,
                                        double* d_theta_obs, int* d_words_obs, double* d_theta_all, double* d_stat_all,
                                        int* d_words_all, double* d_data_all, void* stream)
{
    const bool mask = d_accept || d_status || d_best;
    const bool any_out = mask || d_exceed || d_tally || d_q_obs || d_theta_obs || d_words_obs || d_theta_all || d_stat_all ||
                         d_words_all || d_data_all;
    if (int r = composition_belt_check(pl, d_R3, ntab, S, Q, data, phi, phi_tables, G, P, alpha, any_out, mask,
                                       d_exceed && d_tally && d_q_obs && d_words_obs))
        return r;
    const size_t nn = (size_t)ntab * Q, np = (size_t)(phi_tables ? ntab : 1) * G * 3;
    HIPCHECK(hipSetDevice(pl->device));
    hipStream_t s = stream ? (hipStream_t)stream : pl->stream;
    const int C = pl->det_C;
    if (int r = events_stage(pl, S, Q, nullptr, data, 1, s, phi, np)) return r;
    const EvtLayout l = evt_layout(pl, Q, 1, np);
    const double* dS = pl->d_evt;
    const double* d_data = pl->d_evt + l.data;
    const double* d_phi = pl->d_evt + l.extra;
    if (d_exceed) HIPCHECK(hipMemsetAsync(d_exceed, 0, sizeof(int) * nn * G, s));
    if (d_tally) HIPCHECK(hipMemsetAsync(d_tally, 0, sizeof(int) * nn * G * 4, s));
    int ncu = 0;
    HIPCHECK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, pl->device));
    const long long want = (long long)kEnsBlocksPerCU * (ncu > 0 ? ncu : 1);
    const long long QB = nusi::composition_belt_block(C), nu = (long long)ntab * (((long long)Q * G + QB - 1) / QB);
    const int ps = pl->ens_pslices > 0 ? std::min(pl->ens_pslices, P)
                                       : (int)std::min<long long>(std::max(P / kEnsSliceDatasets, 1), (want + nu - 1) / nu);
    HIPCHECK(nusi::launch_composition_belt(pl->gd, d_R3, ntab, dS, Q, d_data, d_phi, phi_tables != 0, G, P, seed,
                                           detector_bg(pl), C, pl->fit_K, pl->d_tpl, pl->fit_m, pl->fit_w, ps, d_exceed, d_tally,
                                           d_words_obs, d_q_obs, d_theta_obs, d_theta_all, d_stat_all, d_words_all, d_data_all,
                                           s));
    if (mask)
        HIPCHECK(nusi::launch_composition_accept((int)nn, G, P, alpha, d_exceed, d_tally, d_words_obs, d_q_obs, d_accept,
                                                 d_status, d_best, s));
    return detector_mark(pl, s);
}

int nusi_plan_response_composition_belt_host(nusi_plan* pl, const double* R3, int ntab, const double* S, int Q,
                                             const double* data, const double* phi, int phi_tables, int G, int P,
                                             unsigned long long seed, double alpha, int* accept, int* status, int* best,
                                             int* exceed, int* tally, double* q_obs, double* theta_obs, int* words_obs,
                                             double* theta_all, double* stat_all, int* words_all, double* data_all)
{
    const bool mask = accept || status || best;
    const bool any_out = mask || exceed || tally || q_obs || theta_obs || words_obs || theta_all || stat_all || words_all ||
                         data_all;
    if (int r = composition_belt_check(pl, R3, ntab, S, Q, data, phi, phi_tables, G, P, alpha, any_out, mask,
                                       exceed && tally && q_obs && words_obs))
        return r;
    const size_t nn = (size_t)ntab * Q, ng = nn * G, NC = (size_t)pl->fit_K + 3;
    // (R3 is ntab 3 folded matrices in a row)
    return events_host(pl, R3, ntab * 3,
                       {{accept, ng, sizeof(int)}, {status, nn, sizeof(int)}, {best, nn, sizeof(int)}, {exceed, ng, sizeof(int)},
                        {tally, ng * 4, sizeof(int)}, {q_obs, ng, sizeof(double)}, {theta_obs, nn * (G + 1) * NC, sizeof(double)},
                        {words_obs, nn * (G + 1), sizeof(int)}, {theta_all, ng * P * NC, sizeof(double)},
                        {stat_all, ng * P, sizeof(double)}, {words_all, ng * P * 2, sizeof(int)},
                        {data_all, ng * P * pl->det_C, sizeof(double)}},
                       "response composition belt", [&](const double* dI, void* const* d) {
                           return nusi_plan_response_composition_belt(pl, dI, ntab, S, Q, data, phi, phi_tables, G, P, seed, alpha,
                                                                      (int*)d[0], (int*)d[1], (int*)d[2], (int*)d[3], (int*)d[4],
                                                                      (double*)d[5], (double*)d[6], (int*)d[7], (double*)d[8],
                                                                      (double*)d[9], (int*)d[10], (double*)d[11], nullptr);
                       });
}

int nusi_plan_profile_begin(nusi_plan* pl, int max_calls)
{
    HIPCHECK(hipSetDevice(pl->device));
    if (max_calls < 0) return fail(NUSI_EPARAM, "max_calls < 0");
    if ((int)pl->prof_ev.size() < 4 * max_calls) {
        const size_t old = pl->prof_ev.size();
        pl->prof_ev.resize(4 * (size_t)max_calls, nullptr);
        for (size_t k = old; k < pl->prof_ev.size(); ++k) HIPCHECK(hipEventCreate(&pl->prof_ev[k]));
    }
    pl->prof_max = max_calls;
    pl->prof_n = 0;
    return NUSI_OK;
}

int nusi_plan_profile_end(nusi_plan* pl, double* sum_ms3, int* ncalls)
{
    HIPCHECK(hipSetDevice(pl->device));
    for (int k = 0; k < 3; ++k) sum_ms3[k] = 0.0;
    for (int c = 0; c < pl->prof_n; ++c) {
        hipEvent_t* e = &pl->prof_ev[4 * (size_t)c];
        HIPCHECK(hipEventSynchronize(e[3]));
        for (int k = 0; k < 3; ++k) {
            float ms = 0.f;
            HIPCHECK(hipEventElapsedTime(&ms, e[k], e[k + 1]));
            sum_ms3[k] += ms;
        }
    }
    *ncalls = pl->prof_n;
    pl->prof_max = 0;
    pl->prof_n = 0;
    return NUSI_OK;
}

int nusi_plan_stage_ms(nusi_plan* pl, float* ms3)
{
    if (!pl->ran) return fail(NUSI_ESTATE, "no evolve has run on this plan");
    HIPCHECK(hipSetDevice(pl->device));
    HIPCHECK(hipEventSynchronize(pl->last_ev[3]));
    for (int k = 0; k < 3; ++k) HIPCHECK(hipEventElapsedTime(&ms3[k], pl->last_ev[k], pl->last_ev[k + 1]));
    return NUSI_OK;
}

int nusi_plan_set_cascade(nusi_plan* pl, int kind)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    if (kind < NUSI_CASCADE_AUTO || kind > NUSI_CASCADE_MFMA) return fail(NUSI_EPARAM, "unknown cascade kind");
    pl->cascade_kind = kind;
    return NUSI_OK;
}

int nusi_plan_set_option(nusi_plan* pl, int option, int value)
{
    if (!pl) return fail(NUSI_EPARAM, "plan is NULL");
    switch (option) {
    case NUSI_OPT_ALPHA_BATCH:
        if (value < 0 || value > 255) return fail(NUSI_EPARAM, "NUSI_OPT_ALPHA_BATCH outside [0, 255]");
        pl->alpha_batch = value;
        return NUSI_OK;
    case NUSI_OPT_ALPHA_KERNEL:
        if (value < 0 || value > 2) return fail(NUSI_EPARAM, "NUSI_OPT_ALPHA_KERNEL outside [0, 2]");
        pl->alpha_kind = value;
        return NUSI_OK;
    case NUSI_OPT_CASCADE_RHS:
        if (value < 0 || value > 16) return fail(NUSI_EPARAM, "NUSI_OPT_CASCADE_RHS outside [0, 16]");
        pl->cascade_rhs = value;
        return NUSI_OK;
    case NUSI_OPT_STEP_PASSES:
        if (value < 0 || value > 1) return fail(NUSI_EPARAM, "NUSI_OPT_STEP_PASSES outside [0, 1]");
        pl->step_passes = value;
        return NUSI_OK;
    case NUSI_OPT_CASCADE_SYNC:
        if (value < 0 || value > 2) return fail(NUSI_EPARAM, "NUSI_OPT_CASCADE_SYNC outside [0, 2]");
        if (value == 1)   // the per-stage kernels (k_cascade_ws / gb / wsp) were removed in round 5
            return fail(NUSI_EPARAM, "NUSI_OPT_CASCADE_SYNC = 1: the per-stage cascade kernels are gone; k_cascade_bs is the MFMA cascade");
        pl->cascade_sync = value;
        return NUSI_OK;
    case NUSI_OPT_REFO_CORNER_MB:
        if (value < 0 || value > (1 << 20)) return fail(NUSI_EPARAM, "NUSI_OPT_REFO_CORNER_MB outside [0, 2^20]");
        pl->corner_mb = value;
        return NUSI_OK;
    case NUSI_OPT_GA_BATCH:
        if (value < 0 || value > 2) return fail(NUSI_EPARAM, "NUSI_OPT_GA_BATCH outside [0, 2]");
        pl->ga_batch = value;
        return NUSI_OK;
    case NUSI_OPT_GA_PRE_MB:
        if (value < 0 || value > (1 << 20)) return fail(NUSI_EPARAM, "NUSI_OPT_GA_PRE_MB outside [0, 2^20]");
        pl->ga_pre_mb = value;
        return NUSI_OK;
    case NUSI_OPT_GA_PRE_KB:
        if (value < 0 || value > (1 << 30)) return fail(NUSI_EPARAM, "NUSI_OPT_GA_PRE_KB outside [0, 2^30]");
        pl->ga_pre_kb = value;
        return NUSI_OK;
    case NUSI_OPT_RESPONSE_FIFO_KB:
        if (value < 0 || value > (1 << 30)) return fail(NUSI_EPARAM, "NUSI_OPT_RESPONSE_FIFO_KB outside [0, 2^30]");
        pl->response_fifo_kb = value;
        return NUSI_OK;
    case NUSI_OPT_ENSEMBLE_QSLICES:
        if (value < 0 || value > 65535) return fail(NUSI_EPARAM, "NUSI_OPT_ENSEMBLE_QSLICES outside [0, 65535]");
        pl->ens_qslices = value;
        return NUSI_OK;
    case NUSI_OPT_ENSEMBLE_PSLICES:
        if (value < 0 || value > 65535) return fail(NUSI_EPARAM, "NUSI_OPT_ENSEMBLE_PSLICES outside [0, 65535]");
        pl->ens_pslices = value;
        return NUSI_OK;
    case NUSI_OPT_ENSEMBLE_LIMIT_MB:
        if (value < 0 || value > (1 << 20)) return fail(NUSI_EPARAM, "NUSI_OPT_ENSEMBLE_LIMIT_MB outside [0, 2^20]");
        pl->toys_mb = value;
        return NUSI_OK;
    case NUSI_OPT_ENSEMBLE_LIMIT_BYTES:
        if (value < 0 || value > (1 << 30)) return fail(NUSI_EPARAM, "NUSI_OPT_ENSEMBLE_LIMIT_BYTES outside [0, 2^30]");
        pl->toys_b = value;
        return NUSI_OK;
    case NUSI_OPT_TOY_NUISANCE:
        if (value < NUSI_TOYS_FIXED || value > NUSI_TOYS_PRIOR) return fail(NUSI_EPARAM, "NUSI_OPT_TOY_NUISANCE outside [0, 2]");
        pl->toy_nuis = value;
        return NUSI_OK;
    case NUSI_OPT_REFERENCE_ORDER:
        if (value < 0 || value > 1) return fail(NUSI_EPARAM, "NUSI_OPT_REFERENCE_ORDER outside [0, 1]");
        pl->ref_order = value;
        return NUSI_OK;
    case NUSI_OPT_SHIFT_REUSE:
        if (value < 0 || value > 128) return fail(NUSI_EPARAM, "NUSI_OPT_SHIFT_REUSE outside [0, 128]");
        if (value != pl->shift_max && pl->shift) {   // the base plan's axis follows K
            if (pl->ran) {
                HIPCHECK(hipSetDevice(pl->device));
                HIPCHECK(hipEventSynchronize(pl->ev_done));
            }
            nusi_plan_destroy(pl->shift);
            pl->shift = nullptr;
        }
        pl->shift_max = value;
        return NUSI_OK;
    default:
        return fail(NUSI_EPARAM, "unknown plan option");
    }
}

int nusi_plan_warnings(nusi_plan* pl, int* out, int n)
{
    if (!pl->ran) return fail(NUSI_ESTATE, "no evolve has run on this plan");
    if (n > pl->last_n) n = pl->last_n;
    if (pl->warn_host_valid) {   // (fetched by nusi_plan_evolve_host with the fluxes)
        for (int i = 0; i < n; ++i) out[i] = pl->warn_host[pl->slot_of[i]];
        return NUSI_OK;
    }
    HIPCHECK(hipSetDevice(pl->device));
    HIPCHECK(hipEventSynchronize(pl->last_ev[3]));
    std::vector<int> w(pl->last_ntab);
    HIPCHECK(hipMemcpy(w.data(), pl->d_warn, sizeof(int) * w.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) out[i] = w[pl->slot_of[i]];
    return NUSI_OK;
}

int nusi_plan_kernels(const nusi_plan* pl, const char** alpha, const char** cascade)
{
    if (!pl->ran) return fail(NUSI_ESTATE, "no evolve has run on this plan");
    if (alpha) *alpha = pl->alpha_kernel;
    if (cascade) *cascade = pl->cascade_kernel;
    return NUSI_OK;
}

int nusi_plan_ga_kernel(const nusi_plan* pl, const char** ga)
{
    if (!pl->ran) return fail(NUSI_ESTATE, "no evolve has run on this plan");
    if (ga) *ga = pl->ga_kernel;
    return NUSI_OK;
}

int nusi_plan_tables(nusi_plan* pl, int i, double* G, double* At, double* A)
{
    if (!pl->ran) return fail(NUSI_ESTATE, "no evolve has run on this plan");
    if (i < 0 || i >= pl->last_n) return fail(NUSI_EPARAM, "point index out of range");
    HIPCHECK(hipSetDevice(pl->device));
    HIPCHECK(hipEventSynchronize(pl->last_ev[3]));
    const size_t T = (size_t)pl->gd.T, PT = (size_t)pl->gd.PT, j = (size_t)pl->slot_of[i];
    if (G) HIPCHECK(hipMemcpy(G, pl->tabs.G + T * j, sizeof(double) * T, hipMemcpyDeviceToHost));
    if (At) HIPCHECK(hipMemcpy(At, pl->tabs.At + T * j, sizeof(double) * T, hipMemcpyDeviceToHost));
    if (A) HIPCHECK(hipMemcpy(A, pl->tabs.A + PT * j, sizeof(double) * PT, hipMemcpyDeviceToHost));
    return NUSI_OK;
}

int nusi_plan_evolve_host(nusi_plan* pl, const nusi_params* pts, int n, double* flux, double* fla)
{
    int r = nusi_plan_evolve(pl, pts, n, nullptr, nullptr, nullptr);
    if (r) return r;
    const size_t N3 = (size_t)3 * pl->grid.N, fb = sizeof(double) * N3 * n;
    const size_t wb = (sizeof(int) * pl->last_ntab + 255) & ~(size_t)255;
    hipStream_t s = pl->stream;
    const double* dflux = pl->d_scratch;
    const double* dfla = pl->d_scratch + N3 * pl->max_points;
    pl->warn_host.resize(pl->last_ntab);
    if (wb + 2 * fb <= kStageBytes) {
        // small calls (the object API's single propagation): the warnings and both flux arrays into one pinned
        // staging buffer, one synchronisation, then host copies (pageable hipMemcpy round trips cost ~20 us each)
        if (pl->h_out_bytes < wb + 2 * fb) {
            if (pl->h_out) HIPCHECK(hipHostFree(pl->h_out));
            pl->h_out = nullptr;
            pl->h_out_bytes = 0;
            HIPCHECK(hipHostMalloc((void**)&pl->h_out, wb + 2 * fb, hipHostMallocDefault));
            pl->h_out_bytes = wb + 2 * fb;
        }
        HIPCHECK(hipMemcpyAsync(pl->h_out, pl->d_warn, sizeof(int) * pl->last_ntab, hipMemcpyDeviceToHost, s));
        if (n == pl->max_points)   // flux and flux_fla adjacent in d_scratch
            HIPCHECK(hipMemcpyAsync(pl->h_out + wb, dflux, 2 * fb, hipMemcpyDeviceToHost, s));
        else {
            HIPCHECK(hipMemcpyAsync(pl->h_out + wb, dflux, fb, hipMemcpyDeviceToHost, s));
            HIPCHECK(hipMemcpyAsync(pl->h_out + wb + fb, dfla, fb, hipMemcpyDeviceToHost, s));
        }
        HIPCHECK(hipStreamSynchronize(s));
        memcpy(pl->warn_host.data(), pl->h_out, sizeof(int) * pl->last_ntab);
        if (flux) memcpy(flux, pl->h_out + wb, fb);
        if (fla) memcpy(fla, pl->h_out + wb + fb, fb);
    } else {
        HIPCHECK(hipStreamSynchronize(s));
        HIPCHECK(hipMemcpy(pl->warn_host.data(), pl->d_warn, sizeof(int) * pl->last_ntab, hipMemcpyDeviceToHost));
        if (flux) HIPCHECK(hipMemcpy(flux, dflux, fb, hipMemcpyDeviceToHost));
        if (fla) HIPCHECK(hipMemcpy(fla, dfla, fb, hipMemcpyDeviceToHost));
    }
    pl->warn_host_valid = true;
    int bad = 0;
    for (int v : pl->warn_host) bad |= (v & nusi::kWarnSplineOOB);
    if (bad) return fail(NUSI_EINTERP, "Error at interp: a phi-phi table lookup fell outside the node range");
    return NUSI_OK;
}

int nusi_evolve_batch(int device, const nusi_params* pts, int n, double* flux, double* fla)
{
    if (n < 1) return fail(NUSI_EPARAM, "n must be >= 1");
    nusi_plan* pl = nullptr;
    int r = nusi_plan_create(device, pts[0].N_bins_E, pts[0].lEmin, pts[0].lEmax, pts[0].zmax, n, &pl);
    if (r) return r;
    r = nusi_plan_evolve_host(pl, pts, n, flux, fla);
    nusi_plan_destroy(pl);
    return r;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// object API
// ---------------------------------------------------------------------------
// One-point plans of destroyed objects are kept for the next object on the same device and grid (the reference
// builds a calculate_flux per parameter point in its own usage, test.py: a fresh plan costs ~a dozen device
// allocations, a stream and the grid upload).  A plan is handed out with the options at their defaults and no
// phi-phi tables; its buffers are overwritten by the next evolve.  At most kPlanPoolMax are kept; the pool is never
// torn down (process exit reclaims the device).
namespace {
constexpr size_t kPlanPoolMax = 8;
struct PlanPool {
    std::mutex mu;
    std::vector<nusi_plan*> free;
};
PlanPool& plan_pool()
{
    static PlanPool* p = new PlanPool;
    return *p;
}
nusi_plan* pool_take(int dev, int N, double lEmin, double lEmax, double zmax)
{
    PlanPool& pp = plan_pool();
    std::lock_guard<std::mutex> lock(pp.mu);
    for (size_t i = 0; i < pp.free.size(); ++i) {
        nusi_plan* pl = pp.free[i];
        const HostGrid& G = pl->grid;
        if (pl->device == dev && G.N == N && G.lEmin == lEmin && G.lEmax == lEmax && G.zmax_in == zmax) {
            pp.free.erase(pp.free.begin() + (long)i);
            return pl;
        }
    }
    return nullptr;
}
void pool_give(nusi_plan* pl)
{
    if (!pl) return;
    if (pl->max_points == 1 && !pl->shift) {
        // the defaults of nusi_plan_create
        pl->alpha_batch = pl->alpha_kind = pl->cascade_rhs = pl->step_passes = pl->shift_max = 0;
        pl->cascade_sync = pl->corner_mb = pl->ga_batch = pl->ga_pre_mb = pl->ga_pre_kb = 0;
        pl->ref_order = 1;
        pl->cascade_kind = NUSI_CASCADE_AUTO;
        pl->prof_max = pl->prof_n = 0;
        std::fill(pl->slot_set.begin(), pl->slot_set.end(), 0);   // no tabulated sources
        pl->spl.reset();
        PlanPool& pp = plan_pool();
        std::lock_guard<std::mutex> lock(pp.mu);
        if (pp.free.size() < kPlanPoolMax) {
            pp.free.push_back(pl);
            return;
        }
    }
    nusi_plan_destroy(pl);
}
}  // namespace

struct nusi_handle {
    nusi_params p{};
    nusi_plan* plan = nullptr;
    std::vector<double> flux, fla;
    double norm_total = 0.0;   // of the last evolve() (stale in check_energy_conservation)
    bool evolved = false;      // an evolve() has run (norm_total is set)
    int warn = 0;
    std::map<int, int> opts;   // the last value nusi_set_option set per option, replayed by nusi_copy
    // nusi_set_source: the tabulated source in slot 0 of the plan (kept for nusi_copy) and the constructor's
    // source_model, to which S == NULL returns
    bool tab = false, tab_w = false;
    int source0 = NUSI_SOURCE_DSNB;
    std::vector<double> tab_S, tab_wv;
    std::string alpha_kernel, cascade_kernel;   // what this object's last evolve() launched (copied by nusi_copy;
                                                // the pooled plan of a copy may have run another object's call)
    ~nusi_handle() { pool_give(plan); }
};

extern "C" {

static int open_handle(const nusi_params* p, const std::shared_ptr<SplineStore>* share, nusi_handle** out)
{
    *out = nullptr;
    if (p->flav < 0 || p->flav > 2) return fail(NUSI_EPARAM, "flav must be 0, 1 or 2");
    int dev = 0;
    if (const char* e = getenv("NUSI_DEVICE")) dev = atoi(e);
    std::unique_ptr<nusi_handle> h(new nusi_handle);
    h->p = *p;
    h->source0 = p->source_model;
    int r = NUSI_OK;
    h->plan = pool_take(dev, p->N_bins_E, p->lEmin, p->lEmax, p->zmax);
    if (!h->plan) r = nusi_plan_create(dev, p->N_bins_E, p->lEmin, p->lEmax, p->zmax, 1, &h->plan);
    if (r) return r;
    if (p->non_resonant && p->phiphi) {   // nuSIprop.hpp:166-170
        if (share && *share) h->plan->spl = *share;
        else {
            std::string dir = "xsec";
            if (const char* e = getenv("NUSI_XSEC_DIR")) dir = e;
            r = nusi_plan_load_phiphi(h->plan, (dir + "/alphatilde_phiphi.bin").c_str(), nullptr,
                                      (dir + "/alpha_phiphi.bin").c_str(), nullptr);
            if (r) return r;
        }
    }
    h->flux.assign((size_t)3 * p->N_bins_E, 0.0);
    h->fla.assign((size_t)3 * p->N_bins_E, 0.0);
    *out = h.release();
    return NUSI_OK;
}

int nusi_create(const nusi_params* p, nusi_handle** out) { return open_handle(p, nullptr, out); }

int nusi_copy(const nusi_handle* src, nusi_handle** out)
{
    int r = open_handle(&src->p, &src->plan->spl, out);
    if (r) return r;
    (*out)->flux = src->flux;
    (*out)->fla = src->fla;
    (*out)->norm_total = src->norm_total;
    (*out)->evolved = src->evolved;
    (*out)->warn = src->warn;
    (*out)->alpha_kernel = src->alpha_kernel;
    (*out)->cascade_kernel = src->cascade_kernel;
    for (const auto& o : src->opts) {
        r = nusi_set_option(*out, o.first, o.second);
        if (r) {
            nusi_destroy(*out);
            *out = nullptr;
            return r;
        }
    }
    (*out)->source0 = src->source0;
    if (src->tab) {   // the copy's own plan gets the source
        r = nusi_set_source(*out, src->tab_S.data(), src->tab_w ? src->tab_wv.data() : nullptr);
        if (r) {
            nusi_destroy(*out);
            *out = nullptr;
            return r;
        }
    }
    return NUSI_OK;
}

int nusi_source_axis(const nusi_handle* h, int* M, double* lo, double* hi, double* z)
{
    return nusi_plan_source_axis(h->plan, M, lo, hi, z);
}

int nusi_set_source(nusi_handle* h, const double* S, const double* w)
{
    const int r = nusi_plan_set_source(h->plan, 0, S, w);
    if (r) return r;
    h->tab = S != nullptr;
    h->tab_w = S && w;
    if (S) {
        const HostGrid& G = h->plan->grid;
        h->tab_S.assign(S, S + G.T + 1);
        if (w) h->tab_wv.assign(w, w + G.Nz);
        h->p.source_model = NUSI_SOURCE_TABULATED;
    } else {
        h->p.source_model = h->source0;
    }
    return NUSI_OK;
}

void nusi_destroy(nusi_handle* h) { delete h; }

int nusi_set_params(nusi_handle* h, double mphi, double g, double mntot, double si, double norm)
{
    h->p.mphi = mphi;
    h->p.g = g;
    h->p.mntot = mntot;
    h->p.si = si;
    h->p.norm = norm;
    return NUSI_OK;
}

int nusi_get_params(const nusi_handle* h, double* v)
{
    v[0] = h->p.mphi;
    v[1] = h->p.g;
    v[2] = h->p.mntot;
    v[3] = h->p.si;
    v[4] = h->p.norm;
    return NUSI_OK;
}

int nusi_evolve(nusi_handle* h)
{
    int r = nusi_plan_evolve_host(h->plan, &h->p, 1, h->flux.data(), h->fla.data());
    if (r) return r;
    h->norm_total = h->plan->h_pts[0].norm_total;
    h->evolved = true;
    h->alpha_kernel = h->plan->alpha_kernel;
    h->cascade_kernel = h->plan->cascade_kernel;
    int w = 0;
    r = nusi_plan_warnings(h->plan, &w, 1);
    h->warn = w & (NUSI_WARN_GAMMA | NUSI_WARN_ALPHATILDE | NUSI_WARN_ALPHA);
    return r;
}

// The response matrix of the object's parameter point (nusi_plan_response_host on its plan): the object's fluxes,
// source and slot 0 are untouched.
int nusi_response(nusi_handle* h, const double* w, double* G, double* G_fla)
{
    if (!h) return fail(NUSI_EPARAM, "object is NULL");
    return nusi_plan_response_host(h->plan, &h->p, 1, w, G, G_fla);
}
// ... and its mass-resolved response (nusi_plan_response_mass_host)
int nusi_response_mass(nusi_handle* h, const double* w, double* G3, double* G3_fla)
{
    if (!h) return fail(NUSI_EPARAM, "object is NULL");
    return nusi_plan_response_mass_host(h->plan, &h->p, 1, w, G3, G3_fla);
}

int nusi_check_energy_conservation(nusi_handle* h, double* out)
{
    const HostGrid& G = h->plan->grid;
    if (h->p.source_model >= NUSI_SOURCE_TABULATED)
        return fail(NUSI_EPARAM, "check_energy_conservation: not defined for a tabulated source (the free-streaming "
                                 "energy is the power law's; bin integrals do not determine the spectrum's energy integral)");
    // the reference evaluates E_FS with the previous evolve()'s norm_total (nuSIprop.hpp:341-343)
    const bool unset = !h->evolved;
    const double E_FS = energy_fs(h->p.si, h->norm_total, G.zmax_eff, G.lEmin, G.lEmax);
    int r = nusi_evolve(h);
    if (r) return r;
    if (unset) {   // deliberate difference: the reference reads an uninitialised member here (inf / garbage)
        *out = NAN;
        return fail(NUSI_ESTATE, "check_energy_conservation before any evolve(): norm_total is not set "
                                 "(the reference reads it uninitialised); evolved now, result NaN");
    }
    double E_int = 0;
    const int N = G.N;
    for (int i = 0; i < N; ++i)
        for (int k = 0; k < 3; ++k) E_int += (log(G.Emax[i]) - log(G.Emin[i])) * sq(G.Enu[i]) * h->flux[(size_t)k * N + i];
    *out = (E_int - E_FS) / E_FS;
    return NUSI_OK;
}

int nusi_get_flux(const nusi_handle* h, double* out)
{
    memcpy(out, h->flux.data(), sizeof(double) * h->flux.size());
    return NUSI_OK;
}
int nusi_get_flux_fla(const nusi_handle* h, double* out)
{
    memcpy(out, h->fla.data(), sizeof(double) * h->fla.size());
    return NUSI_OK;
}
int nusi_get_energies(const nusi_handle* h, double* out)
{
    memcpy(out, h->plan->grid.Enu.data(), sizeof(double) * h->plan->grid.N);
    return NUSI_OK;
}
int nusi_get_N_bins_E(const nusi_handle* h) { return h->plan->grid.N; }
int nusi_get_N_steps_z(const nusi_handle* h) { return h->plan->grid.Nz; }
int nusi_get_warnings(const nusi_handle* h) { return h->warn; }
int nusi_set_option(nusi_handle* h, int option, int value)
{
    const int r = nusi_plan_set_option(h->plan, option, value);
    if (r == NUSI_OK) h->opts[option] = value;
    return r;
}

int nusi_get_kernels(const nusi_handle* h, const char** alpha, const char** cascade)
{
    if (!h->evolved) return fail(NUSI_ESTATE, "no evolve has run on this object");
    if (alpha) *alpha = h->alpha_kernel.c_str();
    if (cascade) *cascade = h->cascade_kernel.c_str();
    return NUSI_OK;
}

}  // extern "C"
