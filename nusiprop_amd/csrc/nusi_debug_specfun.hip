// nuSIprop MI355X -- TEST ONLY (tests/test_specfun_device_gpu.py): the special functions of the table kernels, one at a
// time, on arrays of arguments on the device.  Not declared in nusi.h; no product path launches these kernels.
//
// A translation unit of its own: inside nusi_kernels.hip the new callers moved k_alpha_mcorner, k_alpha and cli2 (the
// inliner's single-caller bonus), so the kernels live here and are built with the flags nusi_kernels.o is built with
// (Makefile) -- the same headers, the same compiler and options, but this unit's own instances of the out-of-line
// functions (gsl_cli2, gsl_li2, dilog_xge0, clausen, fundamental, nm::log ...).
#include <hip/hip_runtime.h>

#include "nusi_debug_specfun.hpp"

namespace nusi {

// One special function (nusi_debug_specfun.hpp, FN) on arrays of arguments -- element i is lane i % 64 of wave i / 64.
// A lane with active[i] == 0 skips the call inside a divergent branch (its exec bit is off during the call, so the
// callee's wave votes and ballots do not see it) and stores nothing.  One instance per function, each holding only its
// own call
template <int FN>
__global__ __launch_bounds__(256) void k_debug_specfun(const double* __restrict__ a, const double* __restrict__ b,
                                                       const double* __restrict__ c, const int* __restrict__ active,
                                                       int n, double* __restrict__ o0, double* __restrict__ o1)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (active[i] != 0) {
        double r0, r1;
        debug_specfun<FN>(a[i], b[i], c[i], r0, r1);
        o0[i] = r0;
        o1[i] = r1;
    }
}

template <int FN = 0>
static bool launch_debug_specfun(int fn, const double* a, const double* b, const double* c, const int* active, int n,
                                 double* o0, double* o1)
{
    if constexpr (FN < kDsCount) {
        if (fn != FN) return launch_debug_specfun<FN + 1>(fn, a, b, c, active, n, o0, o1);
        hipLaunchKernelGGL(k_debug_specfun<FN>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, a, b, c, active, n,
                           o0, o1);
        return true;
    } else {
        return false;
    }
}

}  // namespace nusi

// Host arrays of n arguments through k_debug_specfun<fn> on the current device.  Every byte of both outputs is set to
// 0xff before the launch (a NaN with every bit set, the sentinel), which is what an inactive element's outputs come
// back as.  -1: n <= 0 or no such fn
extern "C" int nusi_debug_specfun(int fn, const double* a, const double* b, const double* c, const int* active, int n,
                                  double* o0, double* o1)
{
    if (n <= 0 || fn < 0 || fn >= nusi::kDsCount) return -1;
    const size_t N = (size_t)n, nb = sizeof(double) * N, ni = sizeof(int) * N;
    double* d = nullptr;
    int* f = nullptr;
    if (hipMalloc(&d, 5 * nb) != hipSuccess) return -2;
    if (hipMalloc(&f, ni) != hipSuccess) {
        hipFree(d);
        return -2;
    }
    bool ok = hipMemcpy(d, a, nb, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + N, b, nb, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d + 2 * N, c, nb, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(f, active, ni, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(d + 3 * N, 0xff, 2 * nb) == hipSuccess;
    if (ok)
        ok = nusi::launch_debug_specfun(fn, d, d + N, d + 2 * N, f, n, d + 3 * N, d + 4 * N) &&
             hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    ok = ok && hipMemcpy(o0, d + 3 * N, nb, hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(o1, d + 4 * N, nb, hipMemcpyDeviceToHost) == hipSuccess;
    hipFree(d);
    hipFree(f);
    return ok ? 0 : -5;
}
