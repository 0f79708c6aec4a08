#!/usr/bin/env python3
"""Timing of the toys' ensembles (NUSI_OPT_TOY_NUISANCE) on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one
JSON line per measurement.

    python scripts/toy_nuisance_timing.py [--tables 1024] [--reps 3] [--templates 1,3] [--datasets 256] [--limit 400]
                                          [--out FILE]

At scripts/inject_timing.py's and scripts/belt_timing.py's shapes and settings (C = 32; inject: 1000 spectra,
background-only toys tested at the median expected limit, mode upper, both bands and the tally; belt: 64 spectra x 16 grid
points, mode upper, alpha = 0.1, the interval, exceed and the tally; no raw arrays), with every template under a prior of
mean 1 and width 0.2 -- without a prior no ensemble differs from FIXED and FIXED's kernels run:

  inject  nusi_plan_response_inject under NUSI_TOYS_FIXED, _GLOBAL and _PRIOR
  belt    nusi_plan_response_belt under NUSI_TOYS_FIXED and _GLOBAL

The ensembles of one call are measured in the same process, alternating: repetition i runs FIXED, GLOBAL, PRIOR in turn
(after one untimed round of the three, which loads the code objects and allocates); a line gives the median and the least
of --reps wall-clock times around the call and a device synchronisation, and the ratio to FIXED's median.

The measurements of one K run in a child process of their own under `timeout` (--limit seconds), and after a child that
fails or runs out of time nothing more is started.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DELTA = 2.706
ALPHA = 0.1
SEED = 0x0123456789ABCDEF
NAMES = ("fixed", "global", "prior")


def emit(a, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def alternating(H, plan, opt, reps, call, modes):
    """{mode: (median ms, least ms)} of `call` under each mode, the modes in turn within a repetition; the first round is
    not timed."""
    ts = {m: [] for m in modes}
    for r in range(reps + 1):
        for m in modes:
            plan.set_option(opt, m)
            H.hipDeviceSynchronize()
            t0 = time.perf_counter()
            call()
            H.hipDeviceSynchronize()
            if r:
                ts[m].append(1e3 * (time.perf_counter() - t0))
    return {m: (float(np.median(v)), float(np.min(v))) for m, v in ts.items()}


def child(a, K):
    import nusiprop_amd as nu
    from nusiprop_amd import detector, scan
    from scripts.detector_timing import GRID, hip
    nu.load()
    H = hip()
    n, C, NR = a.tables, 32, 5
    Qi, Qb, G = a.spectra, a.belt_spectra, a.grid
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=n)
    N, M = plan.N, plan.T + 1
    nn, nb, ng = n * Qi, n * Qb, n * Qb * G
    dGf, dR, dBand, dBand2, dTally, dLo, dHi, dIdx, dSt, dEx, dTy = (ctypes.c_void_p() for _ in range(11))
    assert H.hipMalloc(ctypes.byref(dGf), n * M * 3 * N * 8) == 0 and H.hipMalloc(ctypes.byref(dR), n * M * C * 8) == 0
    for ptr, nbytes in ((dBand, nn * NR * 8), (dBand2, nn * NR * 8), (dTally, nn * 8 * 4), (dLo, nb * 8), (dHi, max(nb, nn) * 8),
                        (dIdx, nb * 8), (dSt, nb * 4), (dEx, ng * 4), (dTy, ng * 16)):
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
    S = np.array([nu.sources.power_law_integrals(lo, hi, 2.0 + 0.001 * q) for q in range(Qi)])
    x = np.linspace(0.0, 3.0, C)
    T3 = np.stack([40.0 * np.exp(-0.5 * x), 15.0 * np.exp(-1.5 * x) + 1.0, 5.0 + 0.0 * x])
    plan.set_templates(T3[:K], prior=(np.ones(K), np.full(K, 0.2)))
    base = T3[:K].sum(axis=0) + B
    L = nu._lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    OPT = nu._lib.OPT_TOY_NUISANCE
    data = np.ascontiguousarray(detector.pseudo_data(base, 1, np.random.default_rng(2))[0])
    # the test scales: the median over the tables of the observed upper limit (inject: a_test; belt: ref)
    plan.limit_device(dR.value, n, S, data, DELTA, "upper", None, dHi.value)
    H.hipDeviceSynchronize()
    up = np.zeros((n, Qi))
    assert H.hipMemcpy(up.ctypes.data, dHi, up.nbytes, 2) == 0
    a_test = np.ascontiguousarray(np.median(np.where(np.isfinite(up), up, 0.0), axis=0))
    a_inj, th_inj = np.zeros(Qi), np.ones(K)
    Sb = np.ascontiguousarray(S[:Qb])
    ref = np.ascontiguousarray(np.broadcast_to(a_test[:Qb], (n, Qb)))
    frac = np.linspace(0.0, 2.0, G)
    for P in (int(v) for v in a.datasets.split(",")):
        ranks = detector.band_ranks(P)
        rp = ranks.ctypes.data_as(ip)

        def inj():
            nu._lib.check(L.nusi_plan_response_inject(plan._h, dR, n, S.ctypes.data_as(dp), Qi, a_inj.ctypes.data_as(dp),
                                                      th_inj.ctypes.data_as(dp), a_test.ctypes.data_as(dp), P, SEED,
                                                      nu._lib.INJECT_UPPER, rp, NR, None, dBand, dBand2, dTally, None, None, None,
                                                      None, None, None))

        def belt():
            nu._lib.check(L.nusi_plan_response_belt(plan._h, dR, n, Sb.ctypes.data_as(dp), Qb, data.ctypes.data_as(dp),
                                                    frac.ctypes.data_as(dp), G, ref.ctypes.data_as(dp), P, SEED,
                                                    nu._lib.INJECT_UPPER, ALPHA, dLo, dHi, dIdx, dSt, dEx, dTy, None, None, None,
                                                    None, None, None, None, None))

        for what, call, modes, extra in (("inject", inj, (0, 1, 2), {"Q": Qi}), ("belt", belt, (0, 1), {"Q": Qb, "G": G})):
            t = alternating(H, plan, OPT, a.reps, call, modes)
            for m in modes:
                emit(a, dict({"what": what, "nuisance": NAMES[m], "tables": n, "C": C, "K": K, "P": P, "sigma": 0.2,
                              "ms": t[m][0], "ms_min": t[m][1], "ms_per_toy": t[m][0] / P, "ratio_to_fixed": t[m][0] / t[0][0]},
                             **extra))
        plan.set_option(OPT, 0)
    for ptr in (dR, dBand, dBand2, dTally, dLo, dHi, dIdx, dSt, dEx, dTy):
        H.hipFree(ptr)
    plan.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--spectra", type=int, default=1000, help="inject's spectra")
    ap.add_argument("--belt-spectra", type=int, default=64)
    ap.add_argument("--grid", type=int, default=16)
    ap.add_argument("--templates", default="1,3")
    ap.add_argument("--datasets", default="256")
    ap.add_argument("--limit", type=int, default=400, help="seconds a K's measurements may take")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(a, a.child)
    for K in (int(x) for x in a.templates.split(",")):
        if K < 1:
            continue                                                # no template, no prior: FIXED alone
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child", str(K),
               "--tables", str(a.tables), "--reps", str(a.reps), "--spectra", str(a.spectra), "--belt-spectra",
               str(a.belt_spectra), "--grid", str(a.grid), "--datasets", a.datasets] + (["--out", a.out] if a.out else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            emit(a, {"what": "stopped", "K": K, "exit": rc})
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
