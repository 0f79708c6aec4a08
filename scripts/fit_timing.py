#!/usr/bin/env python3
"""Timing of the fit with floating templates on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line
per measurement.

    python scripts/fit_timing.py [--tables 1024] [--reps 5] [--spectra 1000]

  profile  nusi_plan_response_profile of Q spectra on the n folded matrices (C = 32), every output: the yardstick,
           measured in the same session
  fit      nusi_plan_response_fit at the same shape with K = 1 and K = 3 templates, without and with priors, every
           output: ms, the ratio to the profile line, and from the status words the mean and the largest number of
           Newton steps and of halvings and the number of fits flagged singular or not converged

The data are Poisson counts around one (table, spectrum) at a scale of 300 signal events in its fullest bin plus the
templates at normalisation 1 plus the fixed background, so every other (table, spectrum) fits a scale of that order.
Every figure is the wall clock around the call and a device synchronisation (median; the first repetition, with its
allocations and code-object load, is left out).
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nusiprop_amd as nu            # noqa: E402
from nusiprop_amd import detector, scan        # noqa: E402
from scripts.detector_timing import GRID, hip, timed        # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spectra", type=int, default=1000)
    a = ap.parse_args()
    nu.load()
    H = hip()
    n, Q, C = a.tables, a.spectra, 32
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=n)
    N, M = plan.N, plan.T + 1
    dGf, dR, dTh, dMu, dNll, dSt = (ctypes.c_void_p() for _ in range(6))
    assert H.hipMalloc(ctypes.byref(dGf), n * M * 3 * N * 8) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * C * 8) == 0
    assert H.hipMalloc(ctypes.byref(dTh), n * Q * 4 * 8) == 0 and H.hipMalloc(ctypes.byref(dMu), n * Q * C * 8) == 0
    assert H.hipMalloc(ctypes.byref(dNll), n * Q * 8) == 0 and H.hipMalloc(ctypes.byref(dSt), n * Q * 4) == 0
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
    data = rng.poisson(300.0 / s.max() * s + T3.sum(axis=0) + B).astype(np.float64)
    L, dp = nu._lib.load(), ctypes.POINTER(ctypes.c_double)
    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    st = np.zeros(n * Q, dtype=np.int32)
    t_prof, tmin = timed(H, a.reps, lambda: nu._lib.check(L.nusi_plan_response_profile(
        plan._h, dR, n, Sp, Q, datap, dTh, dNll, dMu, dSt, None)))
    assert H.hipMemcpy(st.ctypes.data, dSt, st.nbytes, 2) == 0
    steps = st & nu._lib.FIT_STEPS_MASK
    print(json.dumps({"what": "profile", "tables": n, "C": C, "Q": Q, "ms": t_prof, "ms_min": tmin,
                      "steps_mean": float(steps.mean()), "steps_max": int(steps.max())}), flush=True)
    for K in (1, 3):
        for priors in (False, True):
            plan.set_templates(T3[:K], prior=(np.full(K, 1.1), np.array([0.2, 0.5, 0.05][:K])) if priors else None)
            t, tmin = timed(H, a.reps, lambda: nu._lib.check(L.nusi_plan_response_fit(
                plan._h, dR, n, Sp, Q, datap, dTh, dNll, dMu, dSt, None)))
            assert H.hipMemcpy(st.ctypes.data, dSt, st.nbytes, 2) == 0
            steps = st & nu._lib.FIT_STEPS_MASK
            halv = (st >> nu._lib.FIT_TRIALS_SHIFT) & nu._lib.FIT_TRIALS_MASK
            print(json.dumps({"what": "fit", "tables": n, "C": C, "Q": Q, "K": K, "priors": priors, "ms": t, "ms_min": tmin,
                              "ratio_to_profile": t / t_prof, "steps_mean": float(steps.mean()), "steps_max": int(steps.max()),
                              "halvings_mean": float(halv.mean()), "halvings_max": int(halv.max()),
                              "singular": int(np.count_nonzero(st & nu._lib.FIT_SINGULAR)),
                              "not_converged": int(np.count_nonzero(st & nu._lib.FIT_NOT_CONVERGED)),
                              "signal_at_zero": int(np.count_nonzero(st & nu._lib.FIT_BOUNDARY))}), flush=True)
    for d in (dR, dTh, dMu, dNll, dSt):
        H.hipFree(d)
    plan.close()


if __name__ == "__main__":
    main()
