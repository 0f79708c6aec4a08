#!/usr/bin/env python3
"""Timing of the response matrices on the C4 grid (N_E = 300, lE 12 -> 17): one JSON line per measurement.

    python scripts/response_timing.py [--tables 1024] [--reps 5] [--gamma-tables 256]

  response   stage_ms of an n-table nusi_plan_response (both outputs, device-resident), the cascade stage per
             workgroup of k_cascade_bs_impulse (ceil(T / 16) workgroups per table)
  gamma      for comparison, the cascade stage per workgroup of the power-law gamma batch k_cascade_bs_gamma:
             --gamma-tables tables x 16 spectral indices through nusi_plan_evolve (one workgroup per table)
  apply      nusi_plan_response_apply of Q = 1 and 16 spectra over the n resident matrices: ms (wall clock around the
             call and a device synchronisation, median) and GB/s against the bytes of G

The medians leave out the first repetition (allocations, code-object load).
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
    return H


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--gamma-tables", type=int, default=256)
    a = ap.parse_args()
    nu.load()
    H = hip()
    n = a.tables
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=max(n, 16 * a.gamma_tables))
    N, M, T = plan.N, plan.T + 1, plan.T
    ngrp = -(-T // 16)
    nbytes = n * M * 3 * N * 8
    dG, dGf, dO = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert H.hipMalloc(ctypes.byref(dG), nbytes) == 0 and H.hipMalloc(ctypes.byref(dGf), nbytes) == 0
    assert H.hipMalloc(ctypes.byref(dO), n * 16 * 3 * N * 8) == 0
    arr = plan.params_array(pts)
    ms = []
    for _ in range(a.reps):
        plan.response_device(arr, dG.value, dGf.value)
        ms.append(plan.stage_ms())
    med = [float(np.median([m[k] for m in ms[1:]])) for k in range(3)]
    print(json.dumps({"what": "response", "tables": n, "N_E": N, "M": M, "kernels": plan.kernels(),
                      "stage_ms": med, "workgroups": n * ngrp, "cascade_us_per_workgroup": 1e3 * med[2] / (n * ngrp),
                      "G_bytes_per_array": nbytes}), flush=True)
    if a.gamma_tables:
        gpts = [dict(p, si=2.0 + 0.05 * k) for p in pts[:a.gamma_tables] for k in range(16)]
        garr = plan.params_array(gpts)
        ms = []
        for _ in range(a.reps):
            plan.evolve_device(garr, dG.value, dGf.value)      # (16 x 3 N doubles per table: far inside the buffers)
            ms.append(plan.stage_ms())
        gm = float(np.median([m[2] for m in ms[1:]]))
        print(json.dumps({"what": "gamma", "tables": a.gamma_tables, "points": len(gpts), "kernels": plan.kernels(),
                          "cascade_ms": gm, "cascade_us_per_workgroup": 1e3 * gm / a.gamma_tables}), flush=True)
        plan.response_device(arr, dG.value, dGf.value)          # G again (the evolve wrote into its head)
    lo, hi, _ = plan.source_axis()
    for Q in (1, 16):
        S = [nu.sources.power_law_integrals(lo, hi, 2.0 + 0.05 * q) for q in range(Q)]
        ts = []
        for _ in range(a.reps + 2):
            H.hipDeviceSynchronize()
            t0 = time.perf_counter()
            plan.apply_response_device(dGf.value, n, S, dO.value)
            H.hipDeviceSynchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        t = float(np.median(ts[1:]))
        print(json.dumps({"what": "apply", "tables": n, "Q": Q, "ms": t, "GBps_of_G": nbytes / t * 1e-6}), flush=True)
    for d in (dG, dGf, dO):
        H.hipFree(d)
    plan.close()


if __name__ == "__main__":
    main()
