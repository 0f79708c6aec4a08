// TEST INFRASTRUCTURE ONLY: host build of the member-corner kernel's call chain (alpha_member_ref_dc_inl: Smith's
// division by nusi_div.hpp's forms, GSL's complex dilogarithm inline with the member window's branches), for
// tests/test_alpha_mcorner_div.py.  Never linked into libnusi.so.
#include "nusi_physics.hpp"

extern "C" {

// Dc of n member corners (S, t) at coupling gr, and whether the call's vote put it inside the member window
void hc_member_dc_inl_n(int n, const double* S, const double* t, const double* gr, double* re, double* im, int* win)
{
    for (int i = 0; i < n; ++i) {
        const nusi::cd z = nusi::alpha_member_ref_dc_inl(S[i], t[i], gr[i]);
        re[i] = z.r;
        im[i] = z.i;
        win[i] = nusi::alpha_member_win(1 + S[i] + t[i]) && nusi::alpha_member_win(2 + t[i]) && nusi::alpha_member_win(-gr[i]);
    }
}
// the out-of-line chain on the same corners (alpha_member_ref_dc: operator/ and gsl_cli2)
void hc_member_dc_n(int n, const double* S, const double* t, const double* gr, double* re, double* im)
{
    for (int i = 0; i < n; ++i) {
        const nusi::cd z = nusi::alpha_member_ref_dc(S[i], t[i], gr[i]);
        re[i] = z.r;
        im[i] = z.i;
    }
}
// nusi_div.hpp on the host (the plain division behind the same interface)
void hc_div_shared2_n(int n, const double* a0, const double* a1, const double* b, double* q0, double* q1)
{
    for (int i = 0; i < n; ++i) nusi::nm::div_shared2(a0[i], a1[i], b[i], q0[i], q1[i]);
}

}  // extern "C"
