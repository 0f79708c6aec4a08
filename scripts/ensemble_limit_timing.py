#!/usr/bin/env python3
"""Timing of the ensemble limit on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line per measurement.

    python scripts/ensemble_limit_timing.py [--tables 1024] [--reps 3] [--spectra 1000] [--templates 0,1,3]
                                            [--datasets 16,256] [--limit 400]

For K = 0, 1 and 3 templates at C = 32 and P = 16 and 256 background-only toys, the upper limit at delta = 2.706:

  ensemble_limit  nusi_plan_response_ensemble_limit with the default budget: the band of detector.band_ranks(P) and the
                  tally, no raw arrays (the limits live in the plan's scratch)
  no_band         the same call with NR = 0 and the tally alone: k_toys_limit without the stores of the limits and without
                  k_toys_band; 1 - no_band / ensemble_limit is reported as the selection's share (the stores included)
  separate        measured beside it in the same process: P calls of the existing nusi_plan_response_limit, one per toy,
                  every output NULL but hi -- what the band costs today before the P ntab Q limits are fetched and sorted
                  on the host (which is not counted)

Each `ensemble_limit` line gives the ms, the ratio to the separate calls, the selection's share and the mean outer steps
of the upper side over all (t, q) and the first 16 toys (from an untimed call that fetches their side words).  The toys
are Poisson counts around the templates at normalisation 1 plus the fixed background (scripts/limit_timing.py's).  Every
figure is the wall clock around the call and a device synchronisation (median; the first repetition, with its
allocations and code-object load, is left out).

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
    NR = 5
    dGf, dR, dHi, dBand, dTally, dWords = (ctypes.c_void_p() for _ in range(6))
    assert H.hipMalloc(ctypes.byref(dGf), n * M * 3 * N * 8) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * C * 8) == 0
    assert H.hipMalloc(ctypes.byref(dHi), n * Q * 8) == 0 and H.hipMalloc(ctypes.byref(dBand), n * Q * NR * 8) == 0
    assert H.hipMalloc(ctypes.byref(dTally), n * Q * 8 * 4) == 0 and H.hipMalloc(ctypes.byref(dWords), n * Q * 16 * 2 * 4) == 0
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
    L = nu._lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    Sp, d = S.ctypes.data_as(dp), ctypes.c_double(DELTA)
    UP = nu._lib.LIMIT_UPPER
    for P in (int(v) for v in a.datasets.split(",")):
        toys = detector.pseudo_data(T3[:K].sum(axis=0) + B, P, np.random.default_rng(2))
        ranks = detector.band_ranks(P)
        assert len(ranks) == NR
        tp, rp = toys.ctypes.data_as(dp), ranks.ctypes.data_as(ip)

        def ens():
            nu._lib.check(L.nusi_plan_response_ensemble_limit(plan._h, dR, n, Sp, Q, tp, P, d, UP, rp, NR, None, dBand, dTally,
                                                              None, None, None, None))

        def no_band():
            nu._lib.check(L.nusi_plan_response_ensemble_limit(plan._h, dR, n, Sp, Q, tp, P, d, UP, None, 0, None, None, dTally,
                                                              None, None, None, None))

        def separate():
            for p in range(P):
                nu._lib.check(L.nusi_plan_response_limit(plan._h, dR, n, Sp, Q, toys[p].ctypes.data_as(dp), d, UP, None, dHi,
                                                         None, None, None, None))

        P16 = min(P, 16)                                # the outer steps: the side words of the first toys, untimed
        nu._lib.check(L.nusi_plan_response_ensemble_limit(plan._h, dR, n, Sp, Q, tp, P16, d, UP, None, 0, None, None, dTally,
                                                          None, None, dWords, None))
        H.hipDeviceSynchronize()
        w = np.zeros((n * Q, P16, 2), dtype=np.int32)
        assert H.hipMemcpy(w.ctypes.data, dWords, w.nbytes, 2) == 0
        up = w[..., 1]
        outer = float((up & nu._lib.LIMIT_STEPS_MASK).mean())
        inner = float(((up >> nu._lib.LIMIT_INNER_SHIFT) & nu._lib.LIMIT_INNER_MASK).mean())
        flags = nu._lib.LIMIT_NOT_CONVERGED | nu._lib.LIMIT_NO_FIT | nu._lib.LIMIT_UNBOUNDED
        flagged = int(np.count_nonzero(up & flags))
        t_sep, t_sep_min = timed(H, a.reps, separate)
        print(json.dumps({"what": "separate", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "ms": t_sep, "ms_min": t_sep_min,
                          "ms_per_call": t_sep / P}), flush=True)
        t_nb, t_nb_min = timed(H, a.reps, no_band)
        print(json.dumps({"what": "no_band", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "ms": t_nb, "ms_min": t_nb_min}),
              flush=True)
        t_ens, t_ens_min = timed(H, a.reps, ens)
        print(json.dumps({"what": "ensemble_limit", "tables": n, "C": C, "Q": Q, "K": K, "P": P, "delta": DELTA,
                          "which": "upper", "ranks": [int(r) for r in ranks], "ms": t_ens, "ms_min": t_ens_min,
                          "ratio_to_separate": t_ens / t_sep, "selection_share": 1.0 - t_nb / t_ens, "outer_mean": outer,
                          "inner_mean": inner, "flagged_of_first_toys": flagged}), flush=True)
    for ptr in (dR, dHi, dBand, dTally, dWords):
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
