#!/usr/bin/env python3
"""Timing of the toy-calibrated region of the flavour composition on the C4 grid (N_E = 300, lE 12 -> 17) with resident
tables: one JSON line per measurement.

    python scripts/composition_belt_timing.py [--tables 1024] [--reps 5] [--spectra 16] [--step 10] [--toys 256] [--chunk 128]

  belt        nusi_plan_response_composition_belt of Q spectra, the G points of the flavour triangle at step 1 / --step
              (66 at 10) and P toys on the n resident stacks R3 [n][3][M][C] (C = 32), the mask and the observed side
              and no raw array, for K = 0, 1, 3 templates: ms, the accepted share and the tallies
  host route  beside each, at equal K and in the same process, ALTERNATING with it: what driving the toys from the host
              would cost at best -- per (point, toy) one nusi_plan_response_fit_components call on the stacks plus one
              nusi_plan_response_fit (K >= 1) or nusi_plan_response_profile (K = 0) call on n composed matrices, Q spectra
              each: the two calls' ms times G P (the composing, the draws, the statistic and the counting not counted)
  steps       from a second call on the first --stat-tables tables with words_all: the mean Newton steps and halvings a
              toy, of the free fit and of the held fit

The stacks are scripts/fit_components_timing.py's: the mass-resolved response of the C4 scan's points composed onto the
pure flavours, with a detector that tells the flavours apart.  The data are Poisson counts around table 0's middle
spectrum at the composition (1, 2, 0) / 3 (300 events in the fullest bin) plus the templates at normalisation 1 plus the
fixed background.  Every figure is the wall clock around the call and a device synchronisation (median; the first
repetition of each, with its allocations and code-object load, is left out).
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
from nusiprop_amd import detector, scan, sources        # noqa: E402
from scripts.detector_timing import GRID, hip        # noqa: E402


def once(H, call):
    H.hipDeviceSynchronize()
    t0 = time.perf_counter()
    call()
    H.hipDeviceSynchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tables", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spectra", type=int, default=16)
    ap.add_argument("--step", type=int, default=10)
    ap.add_argument("--toys", type=int, default=256)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--stat-tables", type=int, default=32)
    ap.add_argument("--templates", type=int, nargs="*", default=[0, 1, 3])
    a = ap.parse_args()
    nu.load()
    H = hip()
    n, Q, P, C = a.tables, a.spectra, a.toys, 32
    phi = np.array([(i, j, a.step - i - j) for i in range(a.step + 1) for j in range(a.step + 1 - i)], dtype=np.float64) / a.step
    G = len(phi)
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=min(n, a.chunk))
    N, M = plan.N, plan.T + 1
    X = M * C

    def alloc(nbytes):
        p = ctypes.c_void_p()
        assert H.hipMalloc(ctypes.byref(p), nbytes) == 0
        return p

    rng = np.random.default_rng(1)
    B = rng.random(C) + 0.1
    D = 0.5 + 1.5 * rng.random((C, 3, N))
    for c in range(C):
        for f in range(3):
            if c % 3 != f:
                D[c, f] *= 0.05
    plan.set_detector(D, background=B)
    dMass = alloc(n * 3 * X * 8)                    # the folded mass-resolved rows [n][3][M][C]
    dGf = alloc(min(n, a.chunk) * 3 * M * 3 * N * 8)
    for t0 in range(0, n, a.chunk):
        k = min(a.chunk, n - t0)
        plan.response_mass_device(plan.params_array(pts[t0:t0 + k]), None, dGf.value)
        plan.fold_response_device(dGf.value, 3 * k, dMass.value + t0 * 3 * X * 8)
        H.hipDeviceSynchronize()
    H.hipFree(dGf)
    pure = np.array([sources.mass_fractions(e, normal_ordering=True) for e in np.eye(3)])
    assert all(p.get("normal_ordering", True) for p in pts), "the scan's points share one ordering"
    dR3 = alloc(n * 3 * X * 8)                      # [n][3][M][C]: composed onto the pure flavours
    plan.compose_response_device(dMass.value, n, X, pure, dR3.value)
    dR = alloc(n * X * 8)                           # the host route's held matrices: one composition
    plan.compose_response_device(dR3.value, n, X, np.array([1.0, 2.0, 0.0]) / 3.0, dR.value)
    H.hipDeviceSynchronize()
    H.hipFree(dMass)
    nn = n * Q
    dTh, dMu, dNll, dSt = alloc(nn * 6 * 8), alloc(nn * C * 8), alloc(nn * 8), alloc(nn * 4)
    dAcc, dStat, dBest = alloc(nn * G * 4), alloc(nn * 4), alloc(nn * 4)
    dEx, dTy, dQo = alloc(nn * G * 4), alloc(nn * G * 16), alloc(nn * G * 8)
    dTo, dWo = alloc(nn * (1 + G) * 6 * 8), alloc(nn * (1 + G) * 4)
    ns = min(n, a.stat_tables)
    dWa = alloc(ns * Q * G * P * 2 * 4)
    lo, hi, _ = plan.source_axis()
    S = np.array([sources.power_law_integrals(lo, hi, 2.0 + 0.05 * q) for q in range(Q)])
    R30 = np.zeros((3, M, C))
    assert H.hipMemcpy(R30.ctypes.data, dR3, R30.nbytes, 2) == 0
    x = np.linspace(0.0, 3.0, C)
    T3 = np.stack([40.0 * np.exp(-0.5 * x), 15.0 * np.exp(-1.5 * x) + 1.0, 5.0 + 0.0 * x])
    s = [detector.events_host(R30[j], S[Q // 2]) for j in range(3)]
    sig = (s[0] + 2.0 * s[1]) / 3.0
    mean = 300.0 / sig.max() * sig + T3.sum(axis=0) + B
    data = rng.poisson(mean).astype(np.float64)
    L, dp = nu._lib.load(), ctypes.POINTER(ctypes.c_double)
    Sp, datap, phip = S.ctypes.data_as(dp), data.ctypes.data_as(dp), phi.ctypes.data_as(dp)
    F = nu._lib
    seed = 20261021
    for K in a.templates:
        plan.set_templates(T3[:K] if K else None)

        def belt():
            F.check(L.nusi_plan_response_composition_belt(plan._h, dR3, n, Sp, Q, datap, phip, 0, G, P, seed, 0.1, dAcc, dStat,
                                                          dBest, dEx, dTy, dQo, dTo, dWo, None, None, None, None, None))

        def free():
            F.check(L.nusi_plan_response_fit_components(plan._h, dR3, n, 3, Sp, Q, datap, dTh, dNll, dMu, dSt, None))

        def held():
            if K:
                F.check(L.nusi_plan_response_fit(plan._h, dR, n, Sp, Q, datap, dTh, dNll, dMu, dSt, None))
            else:
                F.check(L.nusi_plan_response_profile(plan._h, dR, n, Sp, Q, datap, dTh, dNll, dMu, dSt, None))

        tb, tf, th = [], [], []
        for _ in range(a.reps + 1):                 # alternating; the first of each is left out
            tf.append(once(H, free))
            th.append(once(H, held))
            tb.append(once(H, belt))
        acc, ty, stat = np.zeros(nn * G, dtype=np.int32), np.zeros((nn * G, 4), dtype=np.int32), np.zeros(nn, dtype=np.int32)
        for host, dev in ((acc, dAcc), (ty, dTy), (stat, dStat)):
            assert H.hipMemcpy(host.ctypes.data, dev, host.nbytes, 2) == 0
        # the steps: a second call on a few tables, with the words of every toy
        F.check(L.nusi_plan_response_composition_belt(plan._h, dR3, ns, Sp, Q, datap, phip, 0, G, P, seed, 0.1, None, None, None,
                                                      None, None, None, None, dWo, None, None, dWa, None, None))
        H.hipDeviceSynchronize()
        w = np.zeros((ns * Q * G * P, 2), dtype=np.int32)
        assert H.hipMemcpy(w.ctypes.data, dWa, w.nbytes, 2) == 0
        wo = np.zeros((ns * Q, 1 + G), dtype=np.int32)
        assert H.hipMemcpy(wo.ctypes.data, dWo, wo.nbytes, 2) == 0
        fail = F.FIT_NOT_CONVERGED | F.FIT_SINGULAR
        ran = np.repeat((((wo[:, :1] | wo[:, 1:]) & fail) == 0).reshape(-1), P)       # the toys of valid points
        steps, halv = (w & F.FIT_STEPS_MASK)[ran], ((w >> F.FIT_TRIALS_SHIFT) & F.FIT_TRIALS_MASK)[ran]
        ms, ms_f, ms_h = float(np.median(tb[1:])), float(np.median(tf[1:])), float(np.median(th[1:]))
        route = G * P * (ms_f + ms_h)
        ntoys = max(int(nn * G * P - 0), 1)
        print(json.dumps({"what": "composition_belt", "tables": n, "C": C, "Q": Q, "G": G, "P": P, "K": K, "ms": ms,
                          "ms_min": float(np.min(tb[1:])), "ms_max": float(np.max(tb[1:])),
                          "fit_components_ms": ms_f, "held": "fit" if K else "profile", "held_ms": ms_h,
                          "host_route_ms": route, "ratio_host_route_over_belt": route / ms,
                          "ns_per_record_toy": 1e6 * ms / (nn * G * (P + 1)),
                          "accepted_share": float(acc.mean()), "pairs_no_fit": int(np.count_nonzero(stat & F.REGION_NO_FIT)),
                          "pairs_all": int(np.count_nonzero(stat & F.REGION_ALL)),
                          "pairs_empty": int(np.count_nonzero(stat & F.REGION_EMPTY)),
                          "toys_free_failed_share": float(ty[:, 0].sum() / ntoys),
                          "toys_held_failed_share": float(ty[:, 1].sum() / ntoys),
                          "toys_signal_at_zero_share": float(ty[:, 2].sum() / ntoys),
                          "stat_tables": ns, "free_steps_mean": float(steps[:, 0].mean()) if len(steps) else 0.0,
                          "free_halvings_mean": float(halv[:, 0].mean()) if len(halv) else 0.0,
                          "held_steps_mean": float(steps[:, 1].mean()) if len(steps) else 0.0,
                          "held_halvings_mean": float(halv[:, 1].mean()) if len(halv) else 0.0}), flush=True)
    for d in (dR3, dR, dTh, dMu, dNll, dSt, dAcc, dStat, dBest, dEx, dTy, dQo, dTo, dWo, dWa):
        H.hipFree(d)
    plan.close()


if __name__ == "__main__":
    main()
