#!/usr/bin/env python3
"""Newton steps inside the calibration call at scripts/inject_timing.py's setting, on a small shape (32 tables of the C4
scan, Q = 200, C = 32, P = 16): one JSON line per K = 0, 1, 3 with the mean and the largest step count and the mean
halvings of the best fit (word 0) and of the conditional fit (word 1) over all (table, spectrum, toy), from the raw words
of an untimed Plan.inject.  A round of either iteration is a step, a halving or the first evaluation.

    python scripts/dev_inject_steps.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import nusiprop_amd as nu
from nusiprop_amd import detector, scan
from scripts.detector_timing import GRID
nu.load()
n, Q, C, P = 32, 200, 32, 16
pts = scan.c4_points()[:n]
plan = nu.Plan(*GRID, max_points=n)
N = plan.N
_, Gf = plan.response(pts)
lo, hi, _ = plan.source_axis()
rng = np.random.default_rng(1)
B = rng.random(C) + 0.1
plan.set_detector(0.5 + 1.5 * rng.random((C, 3, N)), background=B)
R = plan.fold_response(Gf)
S = np.array([nu.sources.power_law_integrals(lo, hi, 2.0 + 0.001 * q) for q in range(Q)])
x = np.linspace(0.0, 3.0, C)
T3 = np.stack([40.0 * np.exp(-0.5 * x), 15.0 * np.exp(-1.5 * x) + 1.0, 5.0 + 0.0 * x])
for K in (0, 1, 3):
    plan.set_templates(T3[:K] if K else None)
    base = T3[:K].sum(axis=0) + B
    toys = detector.pseudo_data(base, P, np.random.default_rng(2))
    _, bhi, _ = plan.ensemble_limit(R, S, toys, 2.706)
    a_test = np.median(np.where(np.isfinite(bhi[..., 2]), bhi[..., 2], 0.0), axis=0)
    out = plan.inject(R, S, 0.0, P, 0x0123456789ABCDEF, theta_inj=np.ones(K) if K else None, a_test=a_test, mode="upper", raw=True)
    w = out[5]
    s0, s1 = w[..., 0] & 0xFF, w[..., 1] & 0xFF
    h0, h1 = (w[..., 0] >> 24) & 0x7F, (w[..., 1] >> 24) & 0x7F
    print(json.dumps({"K": K, "best_steps_mean": float(s0.mean()), "best_steps_max": int(s0.max()), "cond_steps_mean": float(s1.mean()),
                      "cond_steps_max": int(s1.max()), "best_halvings_mean": float(h0.mean()), "cond_halvings_mean": float(h1.mean()),
                      "stat_median": float(np.nanmedian(out[4]))}), flush=True)
plan.close()
