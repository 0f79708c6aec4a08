#!/usr/bin/env python3
"""Timing of the calibration call on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line per measurement.

    python scripts/inject_timing.py [--tables 1024] [--reps 3] [--spectra 1000] [--templates 0,1,3] [--datasets 16,256]
                                    [--limit 400]

For K = 0, 1 and 3 templates at C = 32 and P = 16 and 256 toys:

  ensemble_limit  nusi_plan_response_ensemble_limit at the same shape (the upper limit at delta = 2.706 on host toys around
                  the background, the band and the tally, no raw arrays), measured beside the call in the same process: a
                  whole search per toy where the calibration call does one conditional fit, so its natural ceiling
  inject          nusi_plan_response_inject with background-only toys (a_inj = 0, the templates at 1) tested at a_test[q] =
                  the median over the tables of that call's median expected limit, mode NUSI_INJECT_UPPER: both bands and
                  the tally, no raw arrays
  draw            nusi_plan_draw_counts of rows P C counts around the same expectations, as the generator's share.  All
                  tables x spectra rows need rows P C 8 bytes of output, so at most 2^29 counts are drawn and the time is
                  scaled to the call's tables x spectra rows ("rows_drawn", "scale"); the same call at P = 1 is reported
                  as "ms_staging", the cost of copying the expectations, and is taken off before the scaling

Each line gives ms and ms per toy (ms / P); the `inject` line also the ratios to the two others.  Every figure is the wall
clock around the call and a device synchronisation (median of --reps; the first repetition, with its allocations and
code-object load, is left out).

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
SEED = 0x0123456789ABCDEF


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
    NR = 5
    dGf, dR, dBand, dBand2, dTally, dDraw = (ctypes.c_void_p() for _ in range(6))
    draw_max = 1 << 29
    assert H.hipMalloc(ctypes.byref(dGf), n * M * 3 * N * 8) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * C * 8) == 0
    assert H.hipMalloc(ctypes.byref(dBand), n * Q * NR * 8) == 0 and H.hipMalloc(ctypes.byref(dBand2), n * Q * NR * 8) == 0
    assert H.hipMalloc(ctypes.byref(dTally), n * Q * 8 * 4) == 0 and H.hipMalloc(ctypes.byref(dDraw), draw_max * 8) == 0
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
    x = np.linspace(0.0, 3.0, C)
    T3 = np.stack([40.0 * np.exp(-0.5 * x), 15.0 * np.exp(-1.5 * x) + 1.0, 5.0 + 0.0 * x])
    if K:
        plan.set_templates(T3[:K])
    base = T3[:K].sum(axis=0) + B
    L = nu._lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    Sp, d = S.ctypes.data_as(dp), ctypes.c_double(DELTA)
    UP = nu._lib.LIMIT_UPPER
    a_inj, th_inj = np.zeros(Q), np.ones(max(K, 1))
    for P in (int(v) for v in a.datasets.split(",")):
        toys = detector.pseudo_data(base, P, np.random.default_rng(2))
        ranks = detector.band_ranks(P)
        tp, rp = toys.ctypes.data_as(dp), ranks.ctypes.data_as(ip)

        def ens():
            nu._lib.check(L.nusi_plan_response_ensemble_limit(plan._h, dR, n, Sp, Q, tp, P, d, UP, rp, NR, None, dBand, dTally,
                                                              None, None, None, None))

        t_ens, t_ens_min = timed(H, a.reps, ens)
        print(json.dumps({"what": "ensemble_limit", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "ms": t_ens,
                          "ms_min": t_ens_min, "ms_per_toy": t_ens / P}), flush=True)
        band = np.zeros((n, Q, NR))
        assert H.hipMemcpy(band.ctypes.data, dBand, band.nbytes, 2) == 0
        med = band[..., 2]
        a_test = np.ascontiguousarray(np.median(np.where(np.isfinite(med), med, 0.0), axis=0))

        def inj():
            nu._lib.check(L.nusi_plan_response_inject(plan._h, dR, n, Sp, Q, a_inj.ctypes.data_as(dp), th_inj.ctypes.data_as(dp),
                                                      a_test.ctypes.data_as(dp), P, SEED, nu._lib.INJECT_UPPER, rp, NR, None,
                                                      dBand, dBand2, dTally, None, None, None, None, None, None))

        t_inj, t_inj_min = timed(H, a.reps, inj)
        tally = np.zeros((n, Q, 4), dtype=np.int32)
        assert H.hipMemcpy(tally.ctypes.data, dTally, tally.nbytes, 2) == 0
        rows = min(n * Q, draw_max // (P * C))
        mu = np.ascontiguousarray(base[None, :] * (1.0 + (np.arange(rows) % 7)[:, None] / 7.0))
        mp = mu.ctypes.data_as(dp)

        def drw(Pd):
            return lambda: nu._lib.check(L.nusi_plan_draw_counts(plan._h, mp, rows, C, Pd, SEED, 0, dDraw, None))

        t_drw, t_drw_min = timed(H, a.reps, drw(P))
        t_stage, _ = timed(H, a.reps, drw(1))
        scale = n * Q / rows
        t_gen = max(t_drw - t_stage, 0.0) * scale
        print(json.dumps({"what": "draw", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "rows_drawn": rows, "scale": scale,
                          "ms_measured": t_drw, "ms_staging": t_stage, "ms": t_gen, "ms_per_toy": t_gen / P,
                          "mu_min": float(mu.min()), "mu_max": float(mu.max())}), flush=True)
        print(json.dumps({"what": "inject", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "mode": "upper", "ms": t_inj,
                          "ms_min": t_inj_min, "ms_per_toy": t_inj / P, "ratio_to_ensemble_limit": t_inj / t_ens,
                          "draw_share": t_gen / t_inj, "a_test_median": float(np.median(a_test)),
                          "toys_failed": int(tally[..., :2].sum()), "toys_at_zero": int(tally[..., 2].sum())}), flush=True)
    for ptr in (dR, dBand, dBand2, dTally, dDraw):
        H.hipFree(ptr)
    plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spectra", type=int, default=1000)
    ap.add_argument("--templates", default="0,1,3")
    ap.add_argument("--datasets", default="16,256")
    ap.add_argument("--limit", type=int, default=400, help="seconds a K's measurements may take")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    for K in (int(x) for x in a.templates.split(",")):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(K),
               "--tables", str(a.tables), "--reps", str(a.reps), "--spectra", str(a.spectra), "--datasets", a.datasets]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(json.dumps({"what": "stopped", "K": K, "exit": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
