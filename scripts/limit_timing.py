#!/usr/bin/env python3
"""Timing of the limit call on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line per measurement.

    python scripts/limit_timing.py [--tables 1024] [--reps 3] [--spectra 1000] [--templates 0,1,3] [--limit 300]

For K = 0, 1 and 3 templates at C = 32, the upper limit at delta = 2.706:

  limit   nusi_plan_response_limit, which = NUSI_LIMIT_UPPER, the outputs hi, theta_hat, nll_hat and status
  fit     measured beside it in the same process: the existing nusi_plan_response_fit (K = 0:
          nusi_plan_response_profile) at the same shape, the first output and the status

The yardstick is (1 + mean outer steps) x the existing call's time: what a host-driven search through per-call fits
would cost at best -- the best fit, then one conditional fit per evaluation of the statistic, each paying the front half
s = sum_n R S again (and fetching ntab Q records, which is not counted).  Each `limit` line gives the ms, the mean outer
and inner step counts over all (t, q), the yardstick and the call's ratio to it.  The data are scripts/fit_timing.py's:
Poisson counts around one (table, spectrum) at a scale of 300 signal events in its fullest bin plus the templates at
normalisation 1 plus the fixed background.  Every figure is the wall clock around the call and a device synchronisation
(median; the first repetition, with its allocations and code-object load, is left out).

The measurements of one K run in a child process of their own under `timeout` (--limit seconds), and after a child
that fails or runs out of time nothing more is started.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DELTA = 2.706


def child(a, K):
    import nusiprop_amd as nu
    from nusiprop_amd import detector, scan
    from scripts.detector_timing import GRID, hip, timed
    nu.load()
    H = hip()
    n, Q, C = a.tables, a.spectra, 32
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=n)
    N, M = plan.N, plan.T + 1
    dGf, dR, dTh, dSt, dHi, dNll = (ctypes.c_void_p() for _ in range(6))
    assert H.hipMalloc(ctypes.byref(dGf), n * M * 3 * N * 8) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * C * 8) == 0
    assert H.hipMalloc(ctypes.byref(dTh), n * Q * 4 * 8) == 0 and H.hipMalloc(ctypes.byref(dSt), n * Q * 3 * 4) == 0
    assert H.hipMalloc(ctypes.byref(dHi), n * Q * 8) == 0 and H.hipMalloc(ctypes.byref(dNll), n * Q * 8) == 0
    plan.response_device(plan.params_array(pts), None, dGf.value)
    H.hipDeviceSynchronize()
    lo, hi, _ = plan.source_axis()
    rng = np.random.default_rng(1)
    B = rng.random(C) + 0.1
    plan.set_detector(0.5 + 1.5 * rng.random((C, 3, N)), background=B)
    plan.fold_response_device(dGf.value, n, dR.value)
    H.hipDeviceSynchronize()
    H.hipFree(dGf)
    S = np.array([nu.sources.power_law_integrals(lo, hi, 2.0 + 0.001 * q) for q in range(Q)])
    R0 = np.zeros((M, C))
    assert H.hipMemcpy(R0.ctypes.data, dR, R0.nbytes, 2) == 0
    s = detector.events_host(R0, S[Q // 2])
    x = np.linspace(0.0, 3.0, C)
    T3 = np.stack([40.0 * np.exp(-0.5 * x), 15.0 * np.exp(-1.5 * x) + 1.0, 5.0 + 0.0 * x])
    data = detector.pseudo_data(300.0 / s.max() * s + T3.sum(axis=0) + B, 1, rng)[0]
    if K:
        plan.set_templates(T3[:K])
    L, dp = nu._lib.load(), ctypes.POINTER(ctypes.c_double)
    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    single = L.nusi_plan_response_fit if K else L.nusi_plan_response_profile

    def fit():
        nu._lib.check(single(plan._h, dR, n, Sp, Q, datap, dTh, None, None, dSt, None))

    def limit():
        nu._lib.check(L.nusi_plan_response_limit(plan._h, dR, n, Sp, Q, datap, ctypes.c_double(DELTA), nu._lib.LIMIT_UPPER,
                                                 None, dHi, dTh, dNll, dSt, None))

    t_fit, t_fit_min = timed(H, a.reps, fit)
    st1 = np.zeros(n * Q, dtype=np.int32)
    assert H.hipMemcpy(st1.ctypes.data, dSt, st1.nbytes, 2) == 0
    print(json.dumps({"what": "fit" if K else "profile", "tables": n, "C": C, "Q": Q, "K": K, "ms": t_fit, "ms_min": t_fit_min,
                      "steps_mean": float((st1 & nu._lib.FIT_STEPS_MASK).mean())}), flush=True)
    t_lim, t_lim_min = timed(H, a.reps, limit)
    st = np.zeros((n * Q, 3), dtype=np.int32)
    assert H.hipMemcpy(st.ctypes.data, dSt, st.nbytes, 2) == 0
    up = st[:, 2]
    outer = float((up & nu._lib.LIMIT_STEPS_MASK).mean())
    inner = float(((up >> nu._lib.LIMIT_INNER_SHIFT) & nu._lib.LIMIT_INNER_MASK).mean())
    flags = nu._lib.LIMIT_NOT_CONVERGED | nu._lib.LIMIT_NO_FIT | nu._lib.LIMIT_UNBOUNDED
    yard = (1.0 + outer) * t_fit
    print(json.dumps({"what": "limit", "tables": n, "C": C, "Q": Q, "K": K, "delta": DELTA, "which": "upper", "ms": t_lim,
                      "ms_min": t_lim_min, "outer_mean": outer, "outer_max": int((up & nu._lib.LIMIT_STEPS_MASK).max()),
                      "inner_mean": inner, "flagged": int(np.count_nonzero(up & flags)), "yardstick_ms": yard,
                      "ratio_to_yardstick": t_lim / yard, "ratio_to_fit": t_lim / t_fit}), flush=True)
    for d in (dR, dTh, dSt, dHi, dNll):
        H.hipFree(d)
    plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spectra", type=int, default=1000)
    ap.add_argument("--templates", default="0,1,3")
    ap.add_argument("--limit", type=int, default=300, help="seconds a K's measurements may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    for K in (int(x) for x in a.templates.split(",")):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(K),
               "--tables", str(a.tables), "--reps", str(a.reps), "--spectra", str(a.spectra)]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"what": "stopped", "K": K, "exit": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
