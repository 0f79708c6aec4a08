#!/usr/bin/env python3
"""Timing of the ensemble call on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line per
measurement.

    python scripts/ensemble_timing.py [--tables 1024] [--reps 3] [--spectra 1000] [--datasets 1,16,256] [--limit 300]

For K = 0 (the profile's iteration), 1 and 3 templates, at C = 32, and for every P of --datasets:

  ensemble   nusi_plan_response_ensemble of P Poisson data sets, every output
  separate   the yardstick, measured beside it in the same process: P calls of nusi_plan_response_profile (K = 0) or
             nusi_plan_response_fit, one per data set, with every output NULL but the first -- what a caller did before
             the ensemble call (and then still had to fetch and reduce (ntab, Q) arrays, which is not counted)

Each line gives ms, ms per data set, for the ensemble the ratio to the yardstick and the slices the automatic choice
took, and the mean Newton steps over all (t, q) of data set 0.  The data are Poisson counts around one (table, spectrum)
at a scale of 300 signal events in its fullest bin plus the templates at normalisation 1 plus the fixed background
(scripts/fit_timing.py's).  Every figure is the wall clock around the call(s) and a device synchronisation (median; the
first repetition, with its allocations and code-object load, is left out).

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


def child(a, K):
    import nusiprop_amd as nu
    from nusiprop_amd import detector, scan
    from scripts.detector_timing import GRID, hip, timed
    nu.load()
    H = hip()
    n, Q, C = a.tables, a.spectra, 32
    Ps = [int(x) for x in a.datasets.split(",")]
    Pmax = max(Ps)
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=n)
    N, M = plan.N, plan.T + 1
    dGf, dR, dTh, dSt, dQ, dNll, dEt = (ctypes.c_void_p() for _ in range(7))
    assert H.hipMalloc(ctypes.byref(dGf), n * M * 3 * N * 8) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * C * 8) == 0
    assert H.hipMalloc(ctypes.byref(dTh), n * Q * 4 * 8) == 0 and H.hipMalloc(ctypes.byref(dSt), n * max(Q, Pmax) * 4) == 0
    assert H.hipMalloc(ctypes.byref(dQ), n * Pmax * 4) == 0 and H.hipMalloc(ctypes.byref(dNll), n * Pmax * 8) == 0
    assert H.hipMalloc(ctypes.byref(dEt), n * Pmax * 4 * 8) == 0
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
    toys = detector.pseudo_data(300.0 / s.max() * s + T3.sum(axis=0) + B, Pmax, rng)
    if K:
        plan.set_templates(T3[:K])
    L, dp = nu._lib.load(), ctypes.POINTER(ctypes.c_double)
    Sp = S.ctypes.data_as(dp)
    single = L.nusi_plan_response_fit if K else L.nusi_plan_response_profile

    def one(p, status):
        nu._lib.check(single(plan._h, dR, n, Sp, Q, toys[p].ctypes.data_as(dp), dTh, None, None, status, None))

    one(0, dSt)
    H.hipDeviceSynchronize()
    st = np.zeros(n * Q, dtype=np.int32)
    assert H.hipMemcpy(st.ctypes.data, dSt, st.nbytes, 2) == 0
    steps = float((st & nu._lib.FIT_STEPS_MASK).mean())
    nqb = -(-Q // (8 * (1 if K else 4)))            # spectrum blocks per table at C = 32
    for P in Ps:
        data = np.ascontiguousarray(toys[:P])
        t_sep, t_sep_min = timed(H, a.reps, lambda: [one(p, None) for p in range(P)])
        print(json.dumps({"what": "separate", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "ms": t_sep, "ms_min": t_sep_min,
                          "ms_per_data_set": t_sep / P, "steps_mean": steps}), flush=True)
        for qs, ps in ((0, 0),) + (((1, 1), (nqb, 1)) if a.slices else ()):
            plan.set_option(nu._lib.OPT_ENSEMBLE_QSLICES, qs)
            plan.set_option(nu._lib.OPT_ENSEMBLE_PSLICES, ps)
            t, tmin = timed(H, a.reps, lambda: nu._lib.check(L.nusi_plan_response_ensemble(
                plan._h, dR, n, Sp, Q, data.ctypes.data_as(dp), P, dQ, dNll, dEt, dSt, None)))
            print(json.dumps({"what": "ensemble", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "qslices": qs, "pslices": ps,
                              "ms": t, "ms_min": tmin, "ms_per_data_set": t / P, "ratio_to_separate": t / t_sep,
                              "steps_mean": steps}), flush=True)
    for d in (dR, dTh, dSt, dQ, dNll, dEt):
        H.hipFree(d)
    plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spectra", type=int, default=1000)
    ap.add_argument("--datasets", default="1,16,256")
    ap.add_argument("--templates", default="0,1,3")
    ap.add_argument("--slices", action="store_true", help="also time forced slices: (1, 1) and (every spectrum block, 1)")
    ap.add_argument("--limit", type=int, default=300, help="seconds a K's measurements may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    for K in (int(x) for x in a.templates.split(",")):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(K),
               "--tables", str(a.tables), "--reps", str(a.reps), "--spectra", str(a.spectra), "--datasets", a.datasets]
        rc = subprocess.run(cmd + (["--slices"] if a.slices else [])).returncode
        if rc != 0:
            print(json.dumps({"what": "stopped", "K": K, "exit": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
