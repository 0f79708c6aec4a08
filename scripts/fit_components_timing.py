#!/usr/bin/env python3
"""Timing of the fit with J signal components on the C4 grid (N_E = 300, lE 12 -> 17) with resident tables: one JSON line
per measurement.

    python scripts/fit_components_timing.py [--tables 1024] [--reps 5] [--spectra 1000] [--chunk 128]

  components  nusi_plan_response_fit_components of Q spectra on the n resident stacks R3 [n][J][M][C] (C = 32), every
              output, for J = 2, 3 and K = 0, 1, 3 templates: ms, and from the status words the mean and the largest
              number of Newton steps and of halvings and the tally of flags
  fit         beside each, at equal K and in the same process, ALTERNATING with it: nusi_plan_response_fit (K >= 1) or
              nusi_plan_response_profile (K = 0) on the n matrices composed at equal thirds: the yardstick, and the ratio

The stacks are the mass-resolved response of the C4 scan's points (computed and folded --chunk tables at a time), composed
onto the first J pure flavours with a detector that tells the flavours apart (bin c sees flavour c % 3 in full, the others
at 5 %).  The data are Poisson counts around table 0's middle spectrum at the flavour shares 1 : 1/2 : 1/4 (300 events in
the fullest bin of the first) plus the templates at normalisation 1 plus the fixed background.  Every figure is the wall
clock around the call and a device synchronisation (median; the first repetition of each, with its allocations and
code-object load, is left out).
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
    ap.add_argument("--spectra", type=int, default=1000)
    ap.add_argument("--chunk", type=int, default=128)
    a = ap.parse_args()
    nu.load()
    H = hip()
    n, Q, C = a.tables, a.spectra, 32
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
    dR3 = {J: alloc(n * J * X * 8) for J in (2, 3)}
    for J in (2, 3):                                # [n][J][M][C]: composed onto the first J pure flavours
        plan.compose_response_device(dMass.value, n, X, pure[:J], dR3[J].value)
    dR = alloc(n * X * 8)                           # the yardstick's matrices: the flavours at equal thirds
    plan.compose_response_device(dMass.value, n, X, sources.mass_fractions((1.0, 1.0, 1.0), normal_ordering=True), dR.value)
    H.hipDeviceSynchronize()
    H.hipFree(dMass)
    dTh, dMu, dNll, dSt = alloc(n * Q * 6 * 8), alloc(n * Q * C * 8), alloc(n * Q * 8), alloc(n * Q * 4)
    lo, hi, _ = plan.source_axis()
    S = np.array([sources.power_law_integrals(lo, hi, 2.0 + 0.001 * q) for q in range(Q)])
    R30 = np.zeros((3, M, C))
    assert H.hipMemcpy(R30.ctypes.data, dR3[3], R30.nbytes, 2) == 0
    x = np.linspace(0.0, 3.0, C)
    T3 = np.stack([40.0 * np.exp(-0.5 * x), 15.0 * np.exp(-1.5 * x) + 1.0, 5.0 + 0.0 * x])
    s = [detector.events_host(R30[j], S[Q // 2]) for j in range(3)]
    mean = sum(300.0 * 0.5 ** j / s[0].max() * s[j] for j in range(3)) + T3.sum(axis=0) + B
    data = rng.poisson(mean).astype(np.float64)
    L, dp = nu._lib.load(), ctypes.POINTER(ctypes.c_double)
    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    st = np.zeros(n * Q, dtype=np.int32)
    F = nu._lib
    for K in (0, 1, 3):
        plan.set_templates(T3[:K] if K else None)

        def yard():
            if K:
                F.check(L.nusi_plan_response_fit(plan._h, dR, n, Sp, Q, datap, dTh, dNll, dMu, dSt, None))
            else:
                F.check(L.nusi_plan_response_profile(plan._h, dR, n, Sp, Q, datap, dTh, dNll, dMu, dSt, None))

        for J in (2, 3):
            def comp():
                F.check(L.nusi_plan_response_fit_components(plan._h, dR3[J], n, J, Sp, Q, datap, dTh, dNll, dMu, dSt, None))

            tc, ty = [], []
            for _ in range(a.reps + 1):             # alternating; the first of each is left out
                ty.append(once(H, yard))
                assert H.hipMemcpy(st.ctypes.data, dSt, st.nbytes, 2) == 0
                ysteps = float((st & F.FIT_STEPS_MASK).mean())
                tc.append(once(H, comp))
            assert H.hipMemcpy(st.ctypes.data, dSt, st.nbytes, 2) == 0
            steps, halv = st & F.FIT_STEPS_MASK, (st >> F.FIT_TRIALS_SHIFT) & F.FIT_TRIALS_MASK
            ms, ms_y = float(np.median(tc[1:])), float(np.median(ty[1:]))
            print(json.dumps({"what": "components", "tables": n, "C": C, "Q": Q, "J": J, "K": K, "ms": ms,
                              "ms_min": float(np.min(tc[1:])), "ms_max": float(np.max(tc[1:])),
                              "yardstick": "fit" if K else "profile", "yardstick_ms": ms_y,
                              "yardstick_ms_min": float(np.min(ty[1:])), "yardstick_ms_max": float(np.max(ty[1:])),
                              "ratio": ms / ms_y, "yardstick_steps_mean": ysteps,
                              "steps_mean": float(steps.mean()), "steps_max": int(steps.max()),
                              "halvings_mean": float(halv.mean()), "halvings_max": int(halv.max()),
                              "singular": int(np.count_nonzero(st & F.FIT_SINGULAR)),
                              "not_converged": int(np.count_nonzero(st & F.FIT_NOT_CONVERGED)),
                              "flat": int(np.count_nonzero(st & F.FIT_FLAT)),
                              "boundary": int(np.count_nonzero(st & F.FIT_BOUNDARY)),
                              "a_signal_at_zero": int(np.count_nonzero(st & (((1 << J) - 1) * F.FIT_ZERO)))}), flush=True)
    for d in (dR3[2], dR3[3], dR, dTh, dMu, dNll, dSt):
        H.hipFree(d)
    plan.close()


if __name__ == "__main__":
    main()
