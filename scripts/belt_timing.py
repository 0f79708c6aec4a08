#!/usr/bin/env python3
"""Timing of the toy-calibrated interval on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line per
measurement.

    python scripts/belt_timing.py [--tables 1024] [--reps 3] [--spectra 64] [--grid 16] [--templates 0,1,3]
                                  [--datasets 16,256] [--limit 400] [--out FILE]

For K = 0, 1 and 3 templates at C = 32, Q = 64 spectra x G = 16 grid points (1024 records a table, inject_timing's count)
and P = 16 and 256 toys:

  belt    nusi_plan_response_belt, mode NUSI_INJECT_UPPER, alpha = 0.1, on data drawn around the background (the templates
          at 1), ref[q] = the median over the tables of nusi_plan_response_limit's upper limit at delta = 2.706, frac = G
          points from 0 to 2: the interval, exceed and the tally, no raw arrays (words_obs lives in the plan's scratch)
  inject  nusi_plan_response_inject beside it in the same process on the G-times repeated spectrum list (entry q G + g =
          S[q]) with a_inj = a_test = frac[g] ref[q], theta_inj = 1, the same P, seed and mode: the tally and exceed, no
          band and no raw arrays -- the same toys' two fits without the observed pass and the acceptance

Each line gives ms and ms per toy (ms / P); the `belt` line also ratio_to_inject = belt / inject, the figure to report: the
belt adds one observed record per block and p-slice (about 1 / P of a slice's work) and the acceptance pass.  Every figure
is the wall clock around the call and a device synchronisation (median of --reps; the first repetition, with its
allocations and code-object load, is left out).

The measurements of one K run in a child process of their own under `timeout` (--limit seconds), and after a child that
fails or runs out of time nothing more is started.  --out appends the lines to a file as well.
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
ALPHA = 0.1
SEED = 0x0123456789ABCDEF


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def child(a, K):
    import nusiprop_amd as nu
    from nusiprop_amd import detector, scan
    from scripts.detector_timing import GRID, hip, timed
    nu.load()
    H = hip()
    n, Q, G, C = a.tables, a.spectra, a.grid, 32
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=n)
    N, M = plan.N, plan.T + 1
    nn, ng = n * Q, n * Q * G
    dGf, dR, dLo, dHi, dIdx, dSt, dEx, dTy, dEx2, dTy2 = (ctypes.c_void_p() for _ in range(10))
    assert H.hipMalloc(ctypes.byref(dGf), n * M * 3 * N * 8) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * C * 8) == 0
    for ptr, nbytes in ((dLo, nn * 8), (dHi, nn * 8), (dIdx, nn * 8), (dSt, nn * 4), (dEx, ng * 4), (dTy, ng * 16),
                        (dEx2, ng * 4), (dTy2, ng * 16)):
        assert H.hipMalloc(ctypes.byref(ptr), nbytes) == 0
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
    data = np.ascontiguousarray(detector.pseudo_data(base, 1, np.random.default_rng(2))[0])
    # the reference scale per spectrum: the median over the tables of the observed upper limit
    plan.limit_device(dR.value, n, S, data, DELTA, "upper", None, dHi.value)
    H.hipDeviceSynchronize()
    up = np.zeros((n, Q))
    assert H.hipMemcpy(up.ctypes.data, dHi, up.nbytes, 2) == 0
    ref_q = np.median(np.where(np.isfinite(up), up, 0.0), axis=0)
    ref = np.ascontiguousarray(np.broadcast_to(ref_q, (n, Q)))
    frac = np.linspace(0.0, 2.0, G)
    a_rep = np.ascontiguousarray((frac[None, :] * ref_q[:, None]).reshape(-1))      # entry q G + g
    S_rep = np.ascontiguousarray(np.repeat(S, G, axis=0))
    q_obs = np.ones((n, Q * G))
    th_inj = np.ones(max(K, 1))
    L = nu._lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    for P in (int(v) for v in a.datasets.split(",")):
        def belt():
            nu._lib.check(L.nusi_plan_response_belt(plan._h, dR, n, S.ctypes.data_as(dp), Q, data.ctypes.data_as(dp),
                                                    frac.ctypes.data_as(dp), G, ref.ctypes.data_as(dp), P, SEED,
                                                    nu._lib.INJECT_UPPER, ALPHA, dLo, dHi, dIdx, dSt, dEx, dTy, None, None, None,
                                                    None, None, None, None, None))

        def inj():
            nu._lib.check(L.nusi_plan_response_inject(plan._h, dR, n, S_rep.ctypes.data_as(dp), Q * G, a_rep.ctypes.data_as(dp),
                                                      th_inj.ctypes.data_as(dp), a_rep.ctypes.data_as(dp), P, SEED,
                                                      nu._lib.INJECT_UPPER, None, 0, q_obs.ctypes.data_as(dp), None, None, dTy2,
                                                      dEx2, None, None, None, None, None))

        t_inj, t_inj_min = timed(H, a.reps, inj)
        t_belt, t_belt_min = timed(H, a.reps, belt)
        tally, tally2 = np.zeros((n, Q, G, 4), dtype=np.int32), np.zeros((n, Q * G, 4), dtype=np.int32)
        status, idx = np.zeros((n, Q), dtype=np.int32), np.zeros((n, Q, 2), dtype=np.int32)
        assert H.hipMemcpy(tally.ctypes.data, dTy, tally.nbytes, 2) == 0 and H.hipMemcpy(tally2.ctypes.data, dTy2, tally2.nbytes, 2) == 0
        assert H.hipMemcpy(status.ctypes.data, dSt, status.nbytes, 2) == 0 and H.hipMemcpy(idx.ctypes.data, dIdx, idx.nbytes, 2) == 0
        emit(a, {"what": "inject", "tables": n, "C": C, "Q": Q * G, "K": K, "P": P, "mode": "upper", "ms": t_inj,
                 "ms_min": t_inj_min, "ms_per_toy": t_inj / P, "toys_failed": int(tally2[..., :2].sum())})
        emit(a, {"what": "belt", "tables": n, "C": C, "Q": Q, "G": G, "K": K, "P": P, "mode": "upper", "alpha": ALPHA,
                 "ms": t_belt, "ms_min": t_belt_min, "ms_per_toy": t_belt / P, "ratio_to_inject": t_belt / t_inj,
                 "toys_failed": int(tally[..., :2].sum()), "status_or": int(np.bitwise_or.reduce(status.reshape(-1))),
                 "pairs_empty": int(np.sum((status & detector.BELT_EMPTY) != 0)),
                 "pairs_at_hi_edge": int(np.sum((status & detector.BELT_HI_EDGE) != 0)),
                 "median_last_accepted": float(np.median(idx[..., 1]))})
    for ptr in (dR, dLo, dHi, dIdx, dSt, dEx, dTy, dEx2, dTy2):
        H.hipFree(ptr)
    plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spectra", type=int, default=64)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--templates", default="0,1,3")
    ap.add_argument("--datasets", default="16,256")
    ap.add_argument("--limit", type=int, default=400, help="seconds a K's measurements may take")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    for K in (int(x) for x in a.templates.split(",")):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(K),
               "--tables", str(a.tables), "--reps", str(a.reps), "--spectra", str(a.spectra), "--grid", str(a.grid),
               "--datasets", a.datasets] + (["--out", a.out] if a.out else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            emit(a, {"what": "stopped", "K": K, "exit": rc})
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
