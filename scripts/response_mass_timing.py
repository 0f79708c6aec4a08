#!/usr/bin/env python3
"""Timing of the mass-resolved response on the C4 grid (N_E = 300, lE 12 -> 17): one JSON line per measurement.

    python scripts/response_mass_timing.py [--tables 256] [--reps 7] [--bins 16] [--fifo-kb 0]

  cascade    nusi_plan_response and nusi_plan_response_mass of the same n tables, alternating in one process (both
             outputs, device-resident): the median stage_ms of each, and the cascade stage per workgroup of
             k_cascade_bs_impulse (ceil(T / 16) workgroups per table) beside k_cascade_mass_impulse's (three times as
             many), with the spread (min, max) of the repetitions
  compose    nusi_plan_response_compose of Qc = 1 and 4 compositions per table at X = M 3 N (G3_fla) and at X = M C
             (the folded stack R3, --bins reconstructed-energy bins): ms (wall clock around the call and a device
             synchronisation, median) and GB/s against the bytes read and written

--fifo-kb sets NUSI_OPT_RESPONSE_FIFO_KB for both calls (0 = the default budget of 1 GiB, under which 256 tables of the
mass-resolved call run in two launches; 3145728 holds them in one), and the line reports the launches of each.

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
    ap.add_argument("--tables", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--fifo-kb", type=int, default=0)
    a = ap.parse_args()
    nu.load()
    H = hip()
    n, C = a.tables, a.bins
    pts = scan.c4_points()[:n]
    assert len(pts) == n, "at most 1024 tables (the C4 scan)"
    plan = nu.Plan(*GRID, max_points=n)
    plan.set_option(nu._lib.OPT_RESPONSE_FIFO_KB, a.fifo_kb)
    N, M, T = plan.N, plan.T + 1, plan.T
    ngrp = -(-T // 16)
    X = M * 3 * N
    nbytes = n * X * 8
    bufs = [ctypes.c_void_p() for _ in range(6)]
    dG, dGf, dG3, dG3f, dO, dR = bufs
    for d, sz in zip(bufs, (nbytes, nbytes, 3 * nbytes, 3 * nbytes, 4 * nbytes, 3 * n * M * C * 8)):
        assert H.hipMalloc(ctypes.byref(d), sz) == 0
    arr = plan.params_array(pts)
    ms = {"response": [], "response_mass": []}
    names = {}
    for _ in range(a.reps):
        plan.response_device(arr, dG.value, dGf.value)
        ms["response"].append(plan.stage_ms())
        names["response"] = plan.kernels()[1]
        plan.response_mass_device(arr, dG3.value, dG3f.value)
        ms["response_mass"].append(plan.stage_ms())
        names["response_mass"] = plan.kernels()[1]
    out = {"what": "cascade", "tables": n, "N_E": N, "M": M, "steps": plan.Nz - 1, "reps": a.reps - 1, "fifo_kb": a.fifo_kb}
    budget = (a.fifo_kb << 10) if a.fifo_kb > 0 else 1 << 30
    per = ngrp * 3 * N * 16 * 8                                      # a table's FIFO bytes in the plain call
    for who, wg in (("response", n * ngrp), ("response_mass", 3 * n * ngrp)):
        c = np.array([m[2] for m in ms[who][1:]])
        out[who] = {"kernel": names[who], "stage_ms": [float(np.median([m[k] for m in ms[who][1:]])) for k in range(3)],
                    "workgroups": wg, "launches": -(-n // min(n, max(1, budget // (per * wg // (n * ngrp))))),
                    "cascade_us_per_workgroup": 1e3 * float(np.median(c)) / wg,
                    "cascade_us_per_workgroup_min_max": [1e3 * float(c.min()) / wg, 1e3 * float(c.max()) / wg]}
    out["cascade_ratio_mass_over_plain"] = out["response_mass"]["stage_ms"][2] / out["response"]["stage_ms"][2]
    print(json.dumps(out), flush=True)
    # the folded stack for the compose at X = M C
    D = (0.5 + 1.5 * np.random.default_rng(7).random((C, 3, N))) * 1e3
    plan.set_detector(D)
    plan.fold_response_device(dG3f.value, 3 * n, dR.value)
    kap_rows = [nu.sources.mass_fractions(f) for f in ((1, 2, 0), (0, 1, 0), (1, 0, 0), (1, 1, 1))]
    for what, src, Xc in (("G3_fla", dG3f, X), ("R3", dR, M * C)):
        for Qc in (1, 4):
            kap = np.array(kap_rows[:Qc])
            ts = []
            for _ in range(a.reps + 2):
                H.hipDeviceSynchronize()
                t0 = time.perf_counter()
                plan.compose_response_device(src.value, n, Xc, kap, dO.value)
                H.hipDeviceSynchronize()
                ts.append(1e3 * (time.perf_counter() - t0))
            t = float(np.median(ts[1:]))
            moved = n * Xc * 8 * (3 + Qc)
            print(json.dumps({"what": "compose", "rows": what, "tables": n, "X": Xc, "Qc": Qc, "ms": t,
                              "ms_min_max": [min(ts[1:]), max(ts[1:])], "bytes_moved": moved,
                              "GBps": moved / t * 1e-6}), flush=True)
    for d in bufs:
        H.hipFree(d)
    plan.close()


if __name__ == "__main__":
    main()
