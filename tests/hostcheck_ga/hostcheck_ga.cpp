// TEST INFRASTRUCTURE ONLY: the job map of k_ga_dilogs_batch on the host (tests/test_ga_batch_host.py).  A stand-alone
// program: for a table axis with shared and unshared edges and batches of nb tables it runs every job of the
// producer's grid as the kernel does (ga_batch_job, ga_batch_value, ga_batch_field), then checks that
//   * every field ga_pre_load_batch hands to gamma_k / alphat_k was written by exactly one job, and no job wrote
//     anywhere else or outside the blocks;
//   * its value is bit-equal to ga_pre_slot's for that (point, k, bin, slot) -- the per-table path's value, the
//     |t + 1| < 1e-7 nudge included (m_phi is placed so that one edge's t lies inside it);
//   * ga_batch_need holds for every value that gamma_edge_need / alphat_edge_need / alphat_bin_need of a bin say the
//     bin reads, and a resonant-only batch needs nothing.
// Exit status 0 and a line "ok ..." per case; 1 and the first mismatches otherwise.  Never linked into libnusi.so.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nusi_physics.hpp"

using namespace nusi;

namespace {

int g_bad = 0;
#define CHECK(c, ...)                                       \
    do {                                                    \
        if (!(c)) {                                         \
            if (g_bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } \
        }                                                   \
    } while (0)

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

Point make_point(double mphi, double g, bool majorana, bool non_resonant)
{
    Point P;
    memset(&P, 0, sizeof P);
    P.mphi = mphi;
    P.g = g;
    P.Ga = majorana ? g * g * mphi / (16.0 * M_PI) : g * g * mphi / (8.0 * M_PI);
    P.mn[0] = 0.0218;
    P.mn[1] = 0.0234;
    P.mn[2] = 0.0548;
    for (int k = 0; k < 3; ++k) P.u[k] = 1.0 / 3;
    P.majorana = majorana;
    P.non_resonant = non_resonant;
    P.norm = P.norm_total = 1.0;
    point_derive(P);
    return P;
}

// the table axis: Nc core bins sharing edges from 10^lE0 on (ratio r), then Ne bins with edges of their own
void make_axis(int Nc, int Ne, double lE0, double r, std::vector<double>& lo, std::vector<double>& hi)
{
    lo.clear();
    hi.clear();
    double e = pow(10.0, lE0);
    for (int b = 0; b < Nc; ++b) {
        lo.push_back(e);
        e *= r;
        hi.push_back(e);
    }
    const double l0 = lo[Nc - 1], h0 = hi[Nc - 1];
    for (int b = 1; b <= Ne; ++b) {
        lo.push_back(l0 * (1 + 0.11 * b));
        hi.push_back(h0 * (1 + 0.11 * b));
    }
}

int run_case(int Nc, int Ne, int nb, bool majorana, bool non_resonant, bool nudge)
{
    const int before = g_bad;
    std::vector<double> lo, hi;
    make_axis(Nc, Ne, 12.0, 1.3, lo, hi);
    const int T = Nc + Ne;
    std::vector<int> eu(2 * T), ub;
    std::vector<double> ue(2 * T);
    const int U = edge_numbers(T, lo.data(), hi.data(), eu.data(), ue.data());
    ue.resize(U);
    ub.resize(2 * U);
    edge_bins(T, eu.data(), U, ub.data());
    CHECK(U == Nc + 1 + 2 * Ne, "U = %d", U);
    // m_phi: state 2's t at core edge 5 is -1 - 3e-8, inside alphat_t's nudge window (or clear of it)
    double mphi = sqrt(2 * 0.0548 * ue[5] / (1 + 3e-8));
    if (!nudge) mphi *= 1.01;
    std::vector<Point> pts;
    for (int q = 0; q < nb; ++q) pts.push_back(make_point(mphi, pow(10.0, -3.0 + 3.0 * q / (nb > 1 ? nb - 1 : 1)), majorana, non_resonant));
    if (nudge) {
        const double t = -2 * pts[0].mn[2] * ue[5] / (mphi * mphi);
        CHECK(fabs(t + 1) < 1e-7 && t != -1.0, "edge 5 is not inside the nudge window: t + 1 = %g", t + 1);
        CHECK(alphat_t(pts[0].mn[2], ue[5], mphi * mphi) != t, "the nudge did not move t");
    }

    const size_t GS = ga_gdep_doubles(T, U), SS = ga_shared_doubles(T, U);
    std::vector<double> gd(3 * GS * nb, 0.0), sh(3 * SS, 0.0);
    std::vector<int> ngd(gd.size(), 0), nsh(sh.size(), 0);   // writes per double
    std::vector<unsigned char> needed_gd(gd.size(), 0), needed_sh(sh.size(), 0);
    const int nblk = ga_batch_blocks(nb, T, U);
    long long jobs = 0, needed = 0;
    for (int k = 0; k < 3; ++k)
        for (int blk = 0; blk < nblk + 2; ++blk)   // (two blocks past the grid: they must hold no job)
            for (int lane = 0; lane < 64; ++lane) {
                int vk, item, q;
                if (!ga_batch_job(blk, lane, nb, T, U, &vk, &item, &q)) continue;
                CHECK(blk < nblk, "a job in block %d >= %d", blk, nblk);
                CHECK(vk >= 0 && vk < kGaKinds && q >= 0 && q < nb && item >= 0 && item < (ga_kind_edge(vk) ? U : T),
                      "job out of range: vk %d item %d q %d", vk, item, q);
                CHECK(vk < kGaGdepKinds || q == 0, "a shared kind with q = %d", q);
                ++jobs;
                const Point& P = pts[q];
                const bool edge = ga_kind_edge(vk);
                double v[2] = {0, 0};
                const int nv = ga_batch_value(P, k, vk, edge ? ue[item] : 0.0, edge ? 0.0 : lo[item], edge ? 0.0 : hi[item], v);
                int st;
                const size_t f = ga_batch_field(vk, item, T, U, &st);
                const bool need = ga_batch_need(P, k, vk, item, lo.data(), hi.data(), ub.data());
                needed += need;
                const size_t o = vk < kGaGdepKinds ? (size_t)(q * 3 + k) * GS + f : (size_t)k * SS + f;
                std::vector<double>& dst = vk < kGaGdepKinds ? gd : sh;
                std::vector<int>& cnt = vk < kGaGdepKinds ? ngd : nsh;
                std::vector<unsigned char>& nd = vk < kGaGdepKinds ? needed_gd : needed_sh;
                const size_t blockend = vk < kGaGdepKinds ? (size_t)(q * 3 + k + 1) * GS : (size_t)(k + 1) * SS;
                CHECK(o + (nv == 2 ? st : 0) < blockend, "job writes past its block: vk %d item %d", vk, item);
                if (o + (nv == 2 ? st : 0) >= dst.size()) continue;
                dst[o] = v[0];
                ++cnt[o];
                nd[o] = need;
                if (nv == 2) { dst[o + st] = v[1]; ++cnt[o + st]; nd[o + st] = need; }
            }
    for (size_t i = 0; i < ngd.size(); ++i) CHECK(ngd[i] == 1, "g-dependent double %zu written %d times", i, ngd[i]);
    for (size_t i = 0; i < nsh.size(); ++i) CHECK(nsh[i] == 1, "shared double %zu written %d times", i, nsh[i]);
    if (!non_resonant) CHECK(needed == 0, "a resonant-only batch needs %lld values", needed);

    // every field the consumer loads, against the per-table path's slot value
    long long fields = 0;
    for (int q = 0; q < nb; ++q)
        for (int k = 0; k < 3; ++k)
            for (int n = 0; n < T; ++n) {
                GammaEdgePair ge;
                AlphatEdgePair ae;
                AlphatBinVals bv;
                ga_pre_load_batch(gd.data() + (size_t)(q * 3 + k) * GS, sh.data() + (size_t)k * SS, T, U, n, eu[2 * n],
                                  eu[2 * n + 1], ge, ae, bv);
                double got[kGaPreFields] = {
                    ge.lo.ls, ge.lo.l1s, ge.lo.cz.r, ge.lo.cz.i, ge.hi.ls, ge.hi.l1s, ge.hi.cz.r, ge.hi.cz.i,
                    ae.lo.e78.r, ae.lo.e78.i, ae.lo.e51.r, ae.lo.e51.i, ae.lo.e1o, ae.lo.e1p,
                    ae.hi.e78.r, ae.hi.e78.i, ae.hi.e51.r, ae.hi.e51.i, ae.hi.e1o, ae.hi.e1p,
                    bv.d26a.r, bv.d26a.i, bv.d26b.r, bv.d26b.i, bv.d43a.r, bv.d43a.i, bv.d43b.r, bv.d43b.i,
                    bv.c1, bv.c2, bv.c3, bv.c4};
                for (int slot = 0; slot < kGaPreSlots; ++slot) {
                    double v[2] = {0, 0};
                    int f = -1;
                    const int nv = ga_pre_slot(pts[q], k, lo[n], hi[n], slot, v, &f);
                    for (int c = 0; c < nv; ++c) {
                        ++fields;
                        CHECK(same_bits(got[f + c], v[c]) || (std::isnan(got[f + c]) && std::isnan(v[c])),
                              "table %d k %d bin %d field %d: %.17g, the slot value is %.17g", q, k, n, f + c, got[f + c], v[c]);
                    }
                }
                // what the bin reads is needed: the masks of the consumer's branches against the jobs' predicate
                const unsigned gm = gamma_edge_need<-1>(pts[q], k, lo[n], hi[n]), am = alphat_edge_need<-1>(pts[q], k, lo[n], hi[n]);
                const unsigned bm = alphat_bin_need(pts[q], k, lo[n], hi[n]);
                const int vks[15] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14};
                for (int vk : vks) {
                    const bool edge = ga_kind_edge(vk);
                    const bool reads = vk == 0 ? gm & kGeCz : vk == 4 ? gm & kGeLs : vk == 5 ? gm & kGeL1s : vk == 1 ? am & kAe51
                                       : vk == 6 ? am & kAe78 : vk == 7 ? am & kAe1o : vk == 8 ? am & kAe1p
                                       : vk == 2 || vk == 3 ? bm & kAbD43 : vk == 9 || vk == 10 ? bm & kAbD26 : bm & kAbC;
                    if (!reads) continue;
                    for (int side = 0; side < (edge ? 2 : 1); ++side) {
                        const int item = edge ? eu[2 * n + side] : n;
                        CHECK(ga_batch_need(pts[vk < kGaGdepKinds ? q : 0], k, vk, item, lo.data(), hi.data(), ub.data()),
                              "table %d k %d bin %d reads kind %d (side %d) that no job evaluates", q, k, n, vk, side);
                    }
                }
            }
    printf("%s T %d (U %d) nb %d maj %d nr %d nudge %d: %lld jobs (%lld needed), %lld fields\n", g_bad == before ? "ok" : "FAILED", T, U,
           nb, (int)majorana, (int)non_resonant, (int)nudge, jobs, needed, fields);
    return g_bad - before;
}

}  // namespace

int main()
{
    const int nbs[4] = {1, 3, 32, 64};
    for (int nb : nbs) {
        run_case(45, 46, nb, true, true, true);     // T = 91: 46 shared edges, 46 bins with edges of their own
        run_case(70, 3, nb, true, true, false);     // T = 73: more than a block of shared edges
    }
    run_case(45, 46, 3, false, true, true);         // Dirac
    run_case(45, 46, 3, true, false, true);         // resonant-only: nothing needed
    run_case(130, 0, 5, true, true, true);          // no unshared edge at all; nb not dividing 64
    if (g_bad) printf("%d mismatches\n", g_bad);
    return g_bad ? 1 : 0;
}
