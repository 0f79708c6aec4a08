#!/usr/bin/env python3
"""Timing of the detector calls on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line per
measurement.

    python scripts/detector_timing.py [--tables 1024] [--reps 7]

  fold     nusi_plan_response_fold of the n resident G_fla at C = 16, 32 and 64: ms and GB/s against the bytes of G_fla
           the kernel reads (the bins b < n0 + 16 of each 16-row tile) and against all of G_fla
  events   nusi_plan_response_events of Q = 1000 spectra on the n folded matrices (C = 32), mu only and mu + nll
  profile  nusi_plan_response_profile at the same shape, every output: its ratio to the events' mu + nll line (the same
           bytes and the same front half) and the mean Newton step count from the status words
  apply    nusi_plan_response_apply at Q = 8 in the same session: it reads the same bytes of G_fla in one accumulator
           chunk, so it is the fold's yardstick

Every figure is the wall clock around the call and a device synchronisation (median; the first repetition, with its
allocations and code-object load, is left out).
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nusiprop_amd as nu            # noqa: E402
from nusiprop_amd import scan        # noqa: E402

GRID = (300, 12.0, 17.0, 5.0)


def hip():
    H = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so.7")      # the runtime libnusi.so links
    vp = ctypes.c_void_p
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    return H


def timed(H, reps, call):
    ts = []
    for _ in range(reps + 1):
        H.hipDeviceSynchronize()
        t0 = time.perf_counter()
        call()
        H.hipDeviceSynchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts[1:])), float(np.min(ts[1:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--spectra", type=int, default=1000)
    a = ap.parse_args()
    nu.load()
    H = hip()
    n = a.tables
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=n)
    N, M = plan.N, plan.T + 1
    nbytes = n * M * 3 * N * 8
    read = sum(3 * min(N, n0 + 16) * min(16, M - n0) for n0 in range(0, M, 16)) * 8 * n      # the fold's bytes of G_fla
    Q = a.spectra
    dGf, dR, dO, dMu, dNll = (ctypes.c_void_p() for _ in range(5))
    assert H.hipMalloc(ctypes.byref(dGf), nbytes) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * 64 * 8) == 0
    assert H.hipMalloc(ctypes.byref(dO), n * 8 * 3 * N * 8) == 0
    assert H.hipMalloc(ctypes.byref(dMu), n * Q * 32 * 8) == 0 and H.hipMalloc(ctypes.byref(dNll), n * Q * 8) == 0
    plan.response_device(plan.params_array(pts), None, dGf.value)
    H.hipDeviceSynchronize()
    lo, hi, _ = plan.source_axis()
    rng = np.random.default_rng(1)
    for C in (16, 32, 64):
        plan.set_detector(0.5 + 1.5 * rng.random((C, 3, N)), background=rng.random(C))
        t, tmin = timed(H, a.reps, lambda: plan.fold_response_device(dGf.value, n, dR.value))
        print(json.dumps({"what": "fold", "tables": n, "C": C, "ms": t, "ms_min": tmin, "GBps_of_read": read / t * 1e-6,
                          "GBps_of_G": nbytes / t * 1e-6, "read_fraction": read / nbytes,
                          "TFLOPs": 2.0 * (read / 8) * C / t * 1e-9}), flush=True)
    C = 32
    plan.set_detector(0.5 + 1.5 * rng.random((C, 3, N)), background=rng.random(C) + 0.1)
    plan.fold_response_device(dGf.value, n, dR.value)
    S = np.array([nu.sources.power_law_integrals(lo, hi, 2.0 + 0.001 * q) for q in range(Q)])
    data = np.floor(10 * rng.random(C))
    # (the C entry point itself: the call's own validation and copy of S are inside, Python's handling of 1000 spectra is not)
    L, dp = nu._lib.load(), ctypes.POINTER(ctypes.c_double)
    sc = np.full(Q, 1e-8)
    for label, dat, nll in (("mu", None, None), ("mu+nll", data.ctypes.data_as(dp), dNll)):
        t, tmin = timed(H, a.reps, lambda: nu._lib.check(L.nusi_plan_response_events(
            plan._h, dR, n, S.ctypes.data_as(dp), Q, sc.ctypes.data_as(dp), dat, dMu, nll, None)))
        print(json.dumps({"what": "events", "tables": n, "C": C, "Q": Q, "outputs": label, "ms": t, "ms_min": tmin}),
              flush=True)
    t_events = t
    dAhat, dSt = ctypes.c_void_p(), ctypes.c_void_p()
    assert H.hipMalloc(ctypes.byref(dAhat), n * Q * 8) == 0 and H.hipMalloc(ctypes.byref(dSt), n * Q * 4) == 0
    t, tmin = timed(H, a.reps, lambda: nu._lib.check(L.nusi_plan_response_profile(
        plan._h, dR, n, S.ctypes.data_as(dp), Q, data.ctypes.data_as(dp), dAhat, dNll, dMu, dSt, None)))
    st = np.zeros(n * Q, dtype=np.int32)
    assert H.hipMemcpy(st.ctypes.data, dSt, st.nbytes, 2) == 0
    steps = st & nu._lib.FIT_STEPS_MASK
    print(json.dumps({"what": "profile", "tables": n, "C": C, "Q": Q, "outputs": "ahat+nll+mu+status", "ms": t, "ms_min": tmin,
                      "ratio_to_events_mu_nll": t / t_events, "steps_mean": float(steps.mean()), "steps_max": int(steps.max()),
                      "flagged": int(np.count_nonzero(st & ~nu._lib.FIT_STEPS_MASK))}), flush=True)
    for d in (dAhat, dSt):
        H.hipFree(d)
    S8 = S[:8]
    t, tmin = timed(H, a.reps, lambda: plan.apply_response_device(dGf.value, n, S8, dO.value))
    print(json.dumps({"what": "apply", "tables": n, "Q": 8, "ms": t, "ms_min": tmin, "GBps_of_G": nbytes / t * 1e-6}),
          flush=True)
    for d in (dGf, dR, dO, dMu, dNll):
        H.hipFree(d)
    plan.close()


if __name__ == "__main__":
    main()
