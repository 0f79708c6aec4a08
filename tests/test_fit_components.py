"""The fit with J signal components on the CPU: detector.fit_components_host, the host form of
nusi_plan_response_fit_components (include/nusi.h; DESIGN.md sec. 4, "Signal components: k_components_fit"), and the
composition's statistic.

  * the symbols, their argument counts, the constants, the size check and the refusals without a plan;
  * J = 1 is fit_host to the bit;
  * J = 2, 3 against a scalar loop on Python floats written from the header's text: equal bits;
  * optimality in EXACT arithmetic (fractions.Fraction) at the returned doubles, K_fit = detector.K_fit(C, K, J), with the
    tally of the fits that did not converge printed and capped;
  * the flags; composition; composition_statistic against _limit_lambda and as a statistic (it is not negative, and it
    vanishes at the free fit's own composition, both up to a derived allowance).
"""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_ITER_MAX, FIT_NOT_CONVERGED, FIT_SINGULAR,
                                   FIT_STEPS_MASK, FIT_TRIALS_MASK, FIT_TRIALS_MAX, FIT_TRIALS_SHIFT, FIT_ZERO)
from tests.test_fit import _ldl, _tree

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JK = [(J, K) for J in (2, 3) for K in (0, 1, 2, 3)]


# --- the scalar loop: the header's text on Python floats, J signal components in front ------------------------------------
def components_scalar(sig, T, B, d, m, w, kappa):
    """One fit.  sig: J lists [C]; T: K lists; B, d: lists [C]; m, w: lists [J + K] (J zeros in front)."""
    X = [list(s) for s in sig] + [list(t) for t in T]
    J, n, C = len(sig), len(sig) + len(T), len(d)
    S1 = [_tree(X[j]) for j in range(n)]
    live = [S1[j] > 0.0 and (j >= J or any(d[c] > 0.0 and X[j][c] > 0.0 for c in range(C))) for j in range(n)]
    act = [d[c] > 0.0 and (B[c] > 0.0 or any(live[j] and X[j][c] > 0.0 for j in range(n))) for c in range(C)]
    dmin = min([1.0] + [d[c] for c in range(C) if act[c]])
    D0 = _tree([d[c] if act[c] else 0.0 for c in range(C)])
    nlive = float(sum(live))
    theta = [D0 / (nlive * S1[j]) if live[j] else 0.0 for j in range(n)]

    def evaluate(x):
        den = []
        for c in range(C):
            v = x[0] * X[0][c]
            for j in range(1, n):
                v = v + x[j] * X[j][c]
            den.append(v + B[c])
        bad = any(act[c] and not den[c] > 0.0 for c in range(C))
        wc = [(d[c] / den[c] if act[c] else 0.0) for c in range(C)]
        rc = [(wc[c] / den[c] if act[c] else 0.0) for c in range(C)]
        S2 = [_tree([X[j][c] * wc[c] for c in range(C)]) for j in range(n)]
        H = [[0.0] * n for _ in range(n)]
        for j in range(n):
            for k in range(j, n):
                H[j][k] = H[k][j] = _tree([(X[j][c] * rc[c]) * X[k][c] for c in range(C)]) + (w[j] if j == k else 0.0)
        g = [(S1[j] - S2[j]) + w[j] * (x[j] - m[j]) for j in range(n)]
        return bad, g, H, S2, den

    flags = steps = halvings = 0
    bad, g, H, S2, den = evaluate(theta)
    if bad:
        flags |= FIT_NOT_CONVERGED
    changed = True
    while not bad:
        free = [live[j] and (theta[j] > 0.0 or g[j] < 0.0) for j in range(n)]
        if all(abs(g[j]) <= (kappa * U) * ((S1[j] + S2[j]) + w[j] * (theta[j] + m[j])) for j in range(n) if free[j]):
            break
        if not changed or steps == FIT_ITER_MAX:
            flags |= FIT_NOT_CONVERGED
            break
        F = list(free)
        while True:
            p = _ldl(H, g, F, n)
            leave = [] if p is None else [j for j in range(n) if F[j] and theta[j] == 0.0 and p[j] < 0.0]
            if not leave:
                break
            for j in leave:
                F[j] = False
        acc = 0.0
        if p is not None:
            for j in range(n):
                if F[j]:
                    acc = acc + g[j] * p[j]
        if p is None or not acc < 0.0:
            flags |= FIT_SINGULAR
            break
        ratio = {j: theta[j] / -p[j] for j in range(n) if F[j] and p[j] < 0.0}
        t = min([1.0] + list(ratio.values()))
        clipped = t < 1.0
        quad = not clipped and -acc <= dmin / 16.0
        x = [(0.0 if clipped and ratio.get(j) == t else theta[j] + t * p[j]) for j in range(n)]
        trials = 0
        while True:
            bad_x, g_x, H_x, S2_x, den_x = evaluate(x)
            slope = 0.0
            for j in range(n):
                slope = slope + p[j] * g_x[j]
            if not bad_x and (quad or not slope > 0.0):
                break
            if trials == FIT_TRIALS_MAX:
                x = None
                break
            trials += 1
            halvings += 1
            t = t / 2.0
            x = [theta[j] + t * p[j] for j in range(n)]
        if x is None:
            flags |= FIT_NOT_CONVERGED
            break
        changed = x != theta
        theta, g, H, S2 = x, g_x, H_x, S2_x
        steps += 1
    if not any(live[:J]):
        flags |= FIT_FLAT
    elif all(theta[j] == 0.0 for j in range(J)):
        flags |= FIT_BOUNDARY
    for j in range(n):
        if theta[j] == 0.0:
            flags |= FIT_ZERO << j
    mu = evaluate(theta)[4]
    if any(d[c] > 0.0 and mu[c] == 0.0 for c in range(C)):
        flags |= FIT_INFINITE
    return theta, steps | flags | (min(halvings, FIT_TRIALS_MASK) << FIT_TRIALS_SHIFT), mu


# --- seeded cases ------------------------------------------------------------------------------------------------------
def make_case(C, J, K, seed, bkind="none", close=None, zero=None, pkind="none", asimov=False):
    """(sig (J, C), T (K, C), B, data, prior, truth): falling exponentials with bin-to-bin jitter, every component's
    scale drawn over 12 decades; close: signal row j > 0 is row 0 times (1 + close * a pattern of +-1) instead of a row
    of its own; bkind: the fixed background, none, as large as the signal (1x) or 1000 times it; zero: a component whose
    true normalisation is 0; data Poisson (or Asimov) around the truth, at least J + K bins with data."""
    n = J + K
    rng = np.random.default_rng([seed, C, J, K])
    x = np.linspace(0.0, 3.0, C) if C > 1 else np.zeros(1)
    g0 = rng.uniform(0.2, 1.0)
    base = np.exp(-g0 * x) * (0.7 + 0.6 * rng.random(C))
    rows = []
    for j in range(n):
        if j == 0:
            shape = base
        elif j < J and close is not None:
            shape = base * (1.0 + close * np.where((np.arange(C) * (j + 1) // 2) % 2 == 0, 1.0, -1.0) * (0.5 + 0.5 * rng.random(C)))
        else:
            shape = np.exp(-(g0 + rng.uniform(0.4, 0.9) * j) * x) * (0.7 + 0.6 * rng.random(C))
        rows.append(shape * 10.0 ** rng.uniform(-6, 6))
    X = np.stack(rows)
    counts = 10.0 ** rng.uniform(1.5, 3.5, n)                    # events of each component in its fullest bin
    truth = counts / X.max(axis=1)
    if zero is not None:
        truth[zero] = 0.0
    sig = truth[:J] @ X[:J]
    B = {"none": np.zeros(C), "1x": sig.copy() + 0.5, "1000x": 1e3 * sig + 1.0}[bkind]
    mean = truth @ X + B
    if asimov:
        data = np.array([float(sum(Fraction(float(truth[j])) * Fraction(float(X[j, c])) for j in range(n))
                               + Fraction(float(B[c]))) for c in range(C)])
    else:
        data = rng.poisson(mean).astype(np.float64)
        data[np.argsort(mean)[-n:]] += 1.0                       # (at least J + K bins with data)
    prior = None
    if pkind != "none" and K:
        width, where = pkind.split()
        rel = {"loose": 3.0, "tight": 1e-3}[width]
        floor = 1.0 / X[J:].max(axis=1)
        centre = truth[J:] * ({"near": 1.0, "far": 5.0}[where]) + (0.0 if where == "near" else floor)
        prior = (centre, rel * np.maximum(centre, floor))
    return X[:J], X[J:], B, data, prior, truth


def run(sig, T, B, data, prior):
    J, C = sig.shape
    R3 = np.zeros((J, 2, C))
    R3[:, 1] = sig                                               # M = 2, S = (0, 1): s_j = 0.0 + sig_j * 1.0
    th, nll, mu, st = detector.fit_components_host(R3, np.array([0.0, 1.0]), data, T if len(T) else None, prior=prior,
                                                   background=B, log=math.log)
    return th, float(nll), mu, int(st)


def _prior(J, K, prior):
    m, w = detector._prior(K, prior)
    return np.concatenate([np.zeros(J - 1), m]), np.concatenate([np.zeros(J - 1), w])


VARIANTS = ([dict(bkind=b) for b in ("none", "1x", "1000x")]
            + [dict(close=0.02), dict(close=0.02, bkind="1x"), dict(close=0.02, bkind="1000x")]
            + [dict(zero=0), dict(zero=1, bkind="1x"), dict(zero=1, close=0.02)]
            + [dict(pkind="loose near"), dict(pkind="tight far", bkind="1x"), dict(asimov=True), dict(asimov=True, zero=1),
               dict(asimov=True, bkind="1000x", pkind="tight near")])


# --- the ABI ------------------------------------------------------------------------------------------------------------
NEW = {"nusi_fit_components_shape": 6, "nusi_plan_response_fit_components": 12, "nusi_plan_response_fit_components_host": 11}


def test_abi():
    """The three symbols are declared with the argument counts of the header, bound and exported; the header's constants
    are the package's; without a plan the calls refuse."""
    from nusiprop_amd import _lib
    text = open(os.path.join(ROOT, "include", "nusi.h")).read()
    L = _lib.load()
    for name, nargs in NEW.items():
        decl = re.search(r"^int %s\s*\(([^;]*)\);" % name, text, flags=re.M | re.S)
        assert decl and name in _lib.EXPORTS, name
        args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",")
        assert len(args) == nargs == len(getattr(L, name).argtypes), (name, len(args))
    enum = {k: int(v, 0) for k, v in re.findall(r"^    (NUSI_FIT_[A-Z_]+) = (\w+),?$", text, flags=re.M)}
    assert enum["NUSI_FIT_SIGNALS_MAX"] == detector.FIT_SIGNALS_MAX == _lib.FIT_SIGNALS_MAX == 3
    assert enum["NUSI_FIT_TEMPLATES_MAX"] == detector.FIT_TEMPLATES_MAX == 3
    # NUSI_FIT_ZERO << j for j < 3 + 3: bits 16 .. 21, below the halvings
    assert (enum["NUSI_FIT_ZERO"] << 5) < (1 << enum["NUSI_FIT_TRIALS_SHIFT"]) and enum["NUSI_FIT_ZERO"] == FIT_ZERO
    dp = ctypes.POINTER(ctypes.c_double)
    one = np.ones(8)
    p = one.ctypes.data_as(dp)
    refused = (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_response_fit_components(None, None, 1, 2, p, 1, p, None, None, None, None, None) in refused
    assert L.nusi_plan_response_fit_components_host(None, p, 1, 2, p, 1, p, p, None, None, None) in refused
    # the defaults of the constants' new argument leave every existing value alone
    for C in (1, 5, 64):
        for K in (0, 1, 3):
            assert detector.fit_kappa(C, K) == detector.fit_kappa(C, K, 1) == 2 * (detector._ceil_log2(C) + K) + 18
            assert detector.K_fit(C, K) == detector.K_fit(C, K, 1) == 3 * detector._ceil_log2(C) + 4 * K + 27
            assert detector.fit_kappa(C, K, 3) == detector.fit_kappa(C, K + 2)
            assert detector.K_fit(C, K, 3) == 3 * detector._ceil_log2(C) + 4 * (2 + K) + 27


def test_the_size_check():
    """nusi_fit_components_shape, the check the call applies: J = 2 .. 3, K = 0 .. 3, C = 1 .. 64, and ntab Q and every
    output's element count -- theta [J + K] or mu [C] a record -- below 2^31."""
    from nusiprop_amd import _lib
    L = _lib.load()
    rec = ctypes.c_longlong(-1)
    assert L.nusi_fit_components_shape(64, 3, 3, 7, 11, ctypes.byref(rec)) == _lib.NUSI_OK and rec.value == 77
    assert L.nusi_fit_components_shape(1, 2, 0, 1, 1, None) == _lib.NUSI_OK
    for C, J, K, ntab, Q in ((5, 1, 1, 1, 1), (5, 4, 0, 1, 1), (5, 2, 4, 1, 1), (5, 2, -1, 1, 1), (65, 2, 0, 1, 1),
                             (0, 2, 0, 1, 1), (5, 2, 0, 0, 1), (5, 2, 0, 1, 0), (5, 2, 0, -3, 4), (5, 2, 0, 1, (1 << 19) + 1)):
        assert L.nusi_fit_components_shape(C, J, K, ntab, Q, None) == _lib.NUSI_EPARAM, (C, J, K, ntab, Q)
    for Q in (1000, 4096, 1 << 19):
        # ceil(2^31 / Q) tables are refused whatever the widths ...
        assert L.nusi_fit_components_shape(1, 2, 0, -(-(1 << 31) // Q), Q, None) == _lib.NUSI_EPARAM
        # ... and the limit itself sits at the widest output: W = max(C, J + K) elements a record
        for C, J, K in ((1, 2, 0), (3, 3, 3), (64, 2, 1)):
            W = max(C, J + K)
            edge = -(-(1 << 31) // (Q * W))
            assert L.nusi_fit_components_shape(C, J, K, edge, Q, None) == _lib.NUSI_EPARAM, (C, J, K, Q)
            assert L.nusi_fit_components_shape(C, J, K, edge - 1, Q, ctypes.byref(rec)) == _lib.NUSI_OK, (C, J, K, Q)
            assert rec.value == (edge - 1) * Q


# --- J = 1: fit_host ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", [(C, K) for C in (1, 2, 3, 5, 17, 64) for K in (1, 2, 3)])
def test_one_component_is_fit_host(C, K):
    from tests import test_fit
    seen = 0
    for v, variant in enumerate(test_fit.VARIANTS):
        s, T, B, data, prior, _ = test_fit.make_case(C, K, seed=10 + v, **variant)
        R = np.zeros((2, C))
        R[1] = s
        S = np.array([0.0, 1.0])
        want = detector.fit_host(R, S, data, T, prior=prior, background=B, log=math.log)
        got = detector.fit_components_host(R[None], S, data, T, prior=prior, background=B, log=math.log)
        for a, b in zip(want, got):
            assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), variant
        seen |= int(want[3])
    assert seen & FIT_STEPS_MASK


# --- J = 2, 3 against the scalar loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,J,K", [(C, J, K) for C in (2, 3, 5, 17, 64) for J, K in JK if C >= J + K])
def test_host_equals_the_scalar_loop(C, J, K):
    seen = 0
    for v, variant in enumerate(VARIANTS):
        sig, T, B, data, prior, _ = make_case(C, J, K, seed=10 + v, **variant)
        th, nll, mu, st = run(sig, T, B, data, prior)
        m, w = _prior(J, K, prior)
        th2, st2, mu2 = components_scalar([list(map(float, s)) for s in sig], [list(map(float, t)) for t in T],
                                          list(map(float, B)), list(map(float, data)), list(map(float, m)),
                                          list(map(float, w)), detector.fit_kappa(C, K, J))
        assert st == st2, (variant, hex(st), hex(st2))
        assert th.tolist() == th2 and mu.tolist() == mu2, variant
        want = float(detector.poisson_host(mu, data, log=math.log))
        for j in range(J, J + K):                                # the templates' penalties, ascending
            if w[j] > 0:
                dl = th2[j] - float(m[j])
                want = want + ((0.5 * float(w[j])) * dl) * dl
        assert nll == want, variant
        seen |= st
    assert seen & FIT_STEPS_MASK and (C < 5 or ((seen >> FIT_TRIALS_SHIFT) and seen & (0x3F * FIT_ZERO))), hex(seen)


# --- optimality in exact arithmetic -------------------------------------------------------------------------------------------
def _exact_gradient(X, B, data, m, w, th):
    """(g, scale) of f at th in exact arithmetic on the doubles given (X: all J + K rows)."""
    XF = [[Fraction(float(v)) for v in row] for row in X]
    n, C = len(XF), len(data)
    th = [Fraction(float(v)) for v in th]
    den = [sum(th[k] * XF[k][c] for k in range(n)) + Fraction(float(B[c])) for c in range(C)]
    g, scale = [], []
    for j in range(n):
        S1 = sum(XF[j])
        S2 = Fraction(0)
        for c in range(C):
            if data[c] > 0 and XF[j][c] > 0:
                S2 += XF[j][c] * Fraction(float(data[c])) / den[c]
        wj, mj = Fraction(float(w[j])), Fraction(float(m[j]))
        g.append(S1 - S2 + wj * (th[j] - mj))
        scale.append(S1 + S2 + wj * (th[j] + mj))
    return g, scale


OPT_VARIANTS = [v for v in VARIANTS if not v.get("asimov")]     # 11 variants x 4 seeds: 44 fits a class
OPT_SEEDS = (1, 2, 3, 4)


@pytest.mark.parametrize("C,J,K", [(C, J, K) for C in (3, 5, 6, 17, 64) for J, K in JK if C >= J + K])
def test_optimality_in_exact_arithmetic(C, J, K):
    """Every converged fit: |g_j| <= K_fit u scale_j for the components away from zero, g_j >= -that for those at zero,
    in exact arithmetic, K_fit = detector.K_fit(C, K, J).  A fit flagged SINGULAR or NOT_CONVERGED is left out and
    counted: at most 5 % of a class (44 fits: two)."""
    Kf = detector.K_fit(C, K, J)
    worst, steps, halv, failed, total = 0.0, [], [], [], 0
    for v, variant in enumerate(OPT_VARIANTS):
        for seed in OPT_SEEDS:
            sig, T, B, data, prior, truth = make_case(C, J, K, seed=100 * seed + v, **variant)
            assert np.count_nonzero(data) >= J + K
            th, nll, mu, st = run(sig, T, B, data, prior)
            total += 1
            assert not st & (FIT_INFINITE | FIT_FLAT), (variant, seed, hex(st))
            if st & (FIT_NOT_CONVERGED | FIT_SINGULAR):
                failed.append((variant, seed, hex(st)))
                continue
            m, w = _prior(J, K, prior)
            g, scale = _exact_gradient(np.vstack([sig, T]), B, data, m, w, th)
            for j in range(J + K):
                ratio = g[j] / (Fraction(U) * scale[j])
                if th[j] > 0:
                    assert abs(ratio) <= Kf, (variant, seed, j, float(ratio), Kf)
                    worst = max(worst, abs(float(ratio)))
                else:
                    assert ratio >= -Kf and st & (FIT_ZERO << j), (variant, seed, j, float(ratio))
            steps.append(st & FIT_STEPS_MASK)
            halv.append((st >> FIT_TRIALS_SHIFT) & FIT_TRIALS_MASK)
    print("C=%d J=%d K=%d: %d fits, %d SINGULAR or NOT_CONVERGED %s; worst |g| / (u scale) %.2f of K_fit %d (kappa %d); "
          "steps mean %.2f max %d, halvings mean %.2f max %d" % (C, J, K, total, len(failed), failed, worst, Kf,
                                                                  detector.fit_kappa(C, K, J), np.mean(steps), max(steps),
                                                                  np.mean(halv), max(halv)))
    assert total >= 40 and len(failed) <= 0.05 * total, failed


# --- flags --------------------------------------------------------------------------------------------------------------------
def test_singular():
    sig, T, B, data, _, _ = make_case(17, 2, 1, seed=1)
    sig[1] = sig[0]                                              # two identical rows
    th, nll, mu, st = run(sig, T, B, data, None)
    assert st & FIT_SINGULAR and not st & FIT_NOT_CONVERGED
    for C in (1, 2):                                             # fewer bins with data than components
        for bkind in ("1x", "1000x") + (("none",) if C == 2 else ()):
            sig, T, B, data, _, _ = make_case(C, 3, 0, seed=2, bkind=bkind)
            th, nll, mu, st = run(sig, T, B, data, None)
            assert st & FIT_SINGULAR, (C, bkind, hex(st))
    # (C = 1 without a background is the one class where the data's shortage cannot show: the equal-share start has
    # den = data up to a rounding, which IS a minimiser -- they form a plane -- and the fit stops there before any solve)
    sig, T, B, data, _, _ = make_case(1, 3, 0, seed=2)
    th, nll, mu, st = run(sig, T, B, data, None)
    assert st == 0 and abs(mu[0] - data[0]) <= 4 * U * data[0] and np.allclose(th * sig[:, 0], data[0] / 3.0, rtol=1e-15)


def test_flat_still_fits_the_templates():
    sig, T, B, data, _, truth = make_case(17, 3, 2, seed=4, asimov=True)
    data = np.array([float(v) for v in truth[3:] @ T])           # the templates' own counts
    th, nll, mu, st = run(np.zeros((3, 17)), T, B, data, None)
    assert st & FIT_FLAT and not st & FIT_BOUNDARY and st & FIT_STEPS_MASK and not st & (FIT_SINGULAR | FIT_NOT_CONVERGED)
    assert np.all(th[:3] == 0.0) and (st & (0x3F * FIT_ZERO)) == 7 * FIT_ZERO and np.all(th[3:] > 0)
    assert np.allclose(th[3:], truth[3:], rtol=1e-6)
    # ... and with signal rows only where there are no data
    sig2 = np.zeros((3, 17))
    sig2[:, 3] = (5.0, 1.0, 2.0)
    d2 = data.copy()
    d2[3] = 0.0
    th2, _, _, st2 = run(sig2, T, B, d2, None)
    assert st2 & FIT_FLAT and np.all(th2[:3] == 0.0) and np.all(th2[3:] > 0) and not st2 & (FIT_SINGULAR | FIT_NOT_CONVERGED)


def test_one_dead_component_beside_fitted_ones():
    """A signal row of zeros is not live: it stays at 0 with its ZERO bit, and the others are fitted as if it were not
    there -- the same theta as the fit without it, whose kappa is one step smaller (so: within both stops' reach)."""
    sig, T, B, data, _, truth = make_case(17, 3, 1, seed=5, bkind="1x")
    for dead in range(3):
        s3 = sig.copy()
        s3[dead] = 0.0
        th, nll, mu, st = run(s3, T, B, data, None)
        assert th[dead] == 0.0 and st & (FIT_ZERO << dead) and not st & (FIT_FLAT | FIT_BOUNDARY | FIT_SINGULAR | FIT_NOT_CONVERGED)
        keep = [j for j in range(4) if j != dead]
        th2, _, mu2, st2 = run(np.delete(sig, dead, axis=0), T, B, data, None)
        assert not st2 & (FIT_SINGULAR | FIT_NOT_CONVERGED) and np.any(th2[:2] > 0)
        # (the others may end at zero on their own account: then in both fits alike)
        assert [bool(st & (FIT_ZERO << j)) for j in keep] == [bool(st2 & (FIT_ZERO << j)) for j in range(3)]
        assert np.allclose(th[keep], th2, rtol=1e-9) and np.allclose(mu, mu2, rtol=1e-12)


def test_boundary():
    """Data of the templates and the background alone, Asimov, below what any signal adds: every signal component ends
    at zero with BOUNDARY; and with only one of them absent, no BOUNDARY."""
    sig, T, B, data, _, truth = make_case(17, 2, 2, seed=6, bkind="1x", asimov=True)
    data = np.array([float(v) for v in 0.5 * (truth[2:] @ T + B)])
    th, nll, mu, st = run(sig, T, 0.5 * B + 0.5 * (truth[2:] @ T), data, None)      # B alone explains the data
    assert st & FIT_BOUNDARY and not st & FIT_FLAT and th[0] == 0.0 and th[1] == 0.0
    assert (st & (3 * FIT_ZERO)) == 3 * FIT_ZERO
    sig, T, B, data, _, truth = make_case(17, 2, 1, seed=7, zero=1, asimov=True)
    th, nll, mu, st = run(sig, T, B, data, None)
    assert th[0] > 0 and not st & (FIT_BOUNDARY | FIT_FLAT | FIT_SINGULAR | FIT_NOT_CONVERGED)


def test_infinite_leaves_theta_alone():
    sig, T, B, data, _, _ = make_case(17, 2, 1, seed=8)
    sig[:, 16], T[:, 16], B[16], data[16] = 0.0, 0.0, 0.0, 0.0
    th, nll, mu, st = run(sig, T, B, data, None)
    d2 = data.copy()
    d2[16] = 3.0                                                # a count where nothing can ever be expected
    th2, nll2, mu2, st2 = run(sig, T, B, d2, None)
    assert not st & FIT_INFINITE and math.isfinite(nll)
    assert st2 == st | FIT_INFINITE and nll2 == math.inf and np.array_equal(th2, th) and np.array_equal(mu2, mu)


def test_shapes_and_refusals():
    rng = np.random.default_rng(0)
    M, C, J, K = 6, 7, 3, 2
    R3, S = rng.random((2, J, M, C)), rng.random((4, M))
    T, data = rng.random((K, C)), rng.poisson(20.0, C).astype(float)
    th, nll, mu, st = detector.fit_components_host(R3, S, data, T)
    assert th.shape == (2, 4, J + K) and nll.shape == (2, 4) and mu.shape == (2, 4, C) and st.shape == (2, 4) and st.dtype == np.int32
    one = detector.fit_components_host(R3[1], S[2], data, T)
    assert one[0].shape == (J + K,) and one[2].shape == (C,) and one[1].shape == () and one[3].shape == ()
    assert np.array_equal(one[0], th[1, 2]) and one[1] == nll[1, 2] and one[3] == st[1, 2]
    assert detector.fit_components_host(R3, S, data)[0].shape == (2, 4, J)             # no templates: allowed here
    # the signal rows are events_host's accumulators: mu at the fitted theta from them
    s = [detector.events_host(R3[:, j], S) for j in range(J)]
    den = th[..., 0, None] * s[0]
    for j in range(1, J):
        den = den + th[..., j, None] * s[j]
    for j in range(K):
        den = den + th[..., J + j, None] * T[j]
    assert np.array_equal(mu, den + 0.0)
    for bad in (dict(R3=rng.random((2, 4, M, C))), dict(R3=rng.random((M, C))), dict(R3=-R3), dict(R3=np.where(R3 > 0.9, np.nan, R3)),
                dict(S=rng.random((4, M + 1))), dict(data=data[:-1]), dict(data=-data), dict(T=rng.random((4, C))),
                dict(T=rng.random((K, C + 1)))):
        kw = dict(R3=R3, S=S, data=data, T=T)
        kw.update(bad)
        with pytest.raises(ValueError):
            detector.fit_components_host(kw["R3"], kw["S"], kw["data"], kw["T"])


# --- composition ---------------------------------------------------------------------------------------------------------
def test_composition():
    th = np.array([[1.0, 2.0, 5.0, 9.0], [0.0, 0.0, 0.0, 3.0], [0.25, 0.0, 0.75, 0.0]])
    total, frac = detector.composition(th, 3)
    assert total.tolist() == [8.0, 0.0, 1.0]
    assert frac[0].tolist() == [0.125, 0.25, 0.625] and np.all(np.isnan(frac[1])) and frac[2].tolist() == [0.25, 0.0, 0.75]
    total, frac = detector.composition(th[0], 2)
    assert total == 3.0 and frac.tolist() == [1.0 / 3.0, 2.0 / 3.0]
    assert detector.composition(np.ones((2, 5, 4)), 3)[1].shape == (2, 5, 3)
    with pytest.raises(ValueError):
        detector.composition(th, 5)


# --- the composition's statistic ---------------------------------------------------------------------------------------------
def _scan_host(R3, S, data, phi, T, prior, B):
    """The host form of Plan.composition_scan: compose (response.compose_host's expression), the fits at the held
    compositions, the free fit."""
    ntab, _, M, C = R3.shape
    Qc = phi.shape[0]
    R = np.stack([(phi[c, 0] * R3[:, 0] + phi[c, 1] * R3[:, 1]) + phi[c, 2] * R3[:, 2] for c in range(Qc)], axis=1)
    Rf = R.reshape(ntab * Qc, M, C)
    if T is None:
        ah, nll, mu, st = detector.profile_host(Rf, S, data, background=B, log=math.log)
        th = ah[..., None]
    else:
        th, nll, mu, st = detector.fit_host(Rf, S, data, T, prior=prior, background=B, log=math.log)
    Q = S.shape[0]
    fixed = (th.reshape(ntab, Qc, Q, -1), nll.reshape(ntab, Qc, Q), mu.reshape(ntab, Qc, Q, C), st.reshape(ntab, Qc, Q))
    free = detector.fit_components_host(R3, S, data, T, prior=prior, background=B, log=math.log)
    return fixed, free


def triangle(n):
    """The (n + 1)(n + 2) / 2 points of the flavour triangle with fractions in steps of 1 / n."""
    return np.array([(i / n, j / n, (n - i - j) / n) for i in range(n + 1) for j in range(n + 1 - i)])


def allowance(mu, th, mu_hat, th_hat, phi, X, data, prior, mag, M):
    """The allowance of the statistic's two properties, in the statistic's own units, derived and not fitted:

      lambda >= -allowance at any composition, and |lambda| <= allowance at the free fit's own composition.

    (1) The statistic's own rounding, as DESIGN.md derives K_limit: a term carries the roundings of the difference (1),
        the quotient (1), the log (within an ulp: 2), the product (1) and the subtraction (1), tree() adds L =
        ceil(log2 C), the penalties K additions: E = L + K + 6 units of u mag.
    (2) f is convex, so f(x) - f(theta_hat) >= g(theta_hat) . (x - theta_hat), x the held fit's point in the components'
        space (a phi_j, then its templates); the free fit stopped with |g_j| <= K_fit u scale_j on the free components and
        g_j >= -that on those at zero, where x_j - theta_hat_j >= 0: lambda >= -K_fit u sum_j scale_j |x_j - theta_hat_j|,
        K_fit = detector.K_fit(C, K, J), scale_j = (S1_j + S2_j) + w_j (theta_hat_j + m_j).  At the free fit's own
        composition x lies on the ray through theta_hat, along which the held fit minimises: by the same argument from
        its side (its stop is no wider: K_fit(C, K) <= K_fit(C, K, J); the profile ends within the rounding of its
        gradient) the same term bounds lambda from above.
    (3) The held fit's mu is formed from the composed rows, the free fit's from the components: at equal parameters
        they differ per bin by the roundings of the composition (3), of two front sums over n < M (2 M), of the fractions
        (J), of the two den (J + K + 3): eta = (2 M + 2 J + K + 6) u relative, every term non-negative.  A bin's term has
        the derivative (1 - data_c / mu_c): |mu_hat_c - data_c| eta (1 + eta) at most, plus the second order inside mag."""
    C, n, K = len(data), X.shape[0], th.shape[-1] - 1
    J = n - K
    L = detector._ceil_log2(C)
    m, w = _prior(J, K, prior)
    x = np.concatenate([th[0] * phi, th[1:]])
    S1 = X.sum(axis=1)
    S2 = np.array([np.sum(np.where((data > 0) & (mu_hat > 0), X[j] * data / np.where(mu_hat > 0, mu_hat, 1.0), 0.0)) for j in range(n)])
    scale = (S1 + S2) + w * (th_hat + m)
    eta = (2 * M + 2 * J + K + 6) * U
    return ((L + K + 6) * U * mag + detector.K_fit(C, K, J) * U * float(np.sum(scale * np.abs(x - th_hat))) * (1.0 + 1e-6)
            + eta * (1.0 + eta) * float(np.sum(np.abs(mu_hat - data))) + eta * mag)


@pytest.mark.parametrize("K", (0, 2))
def test_composition_statistic(K):
    """composition_statistic equals _limit_lambda record by record, bit for bit; lambda >= -allowance on a triangle grid
    and |lambda| <= allowance at the free fit's own signal theta_hat taken as the weights (``allowance``: the statistic's
    operation count, the free fit's stop through convexity, the composed rows' roundings)."""
    rng = np.random.default_rng(5 + K)
    ntab, M, C, Q = 2, 6, 17, 3
    x = np.linspace(0.0, 3.0, C)
    R3 = np.stack([[np.outer(0.5 + rng.random(M), np.exp(-(0.3 + 0.5 * j) * x) * (0.7 + 0.6 * rng.random(C))) for j in range(3)]
                   for _ in range(ntab)])
    S = rng.uniform(0.5, 2.0, (Q, M))
    T = np.stack([np.exp(-2.5 * x) * 8.0, np.ones(C)])[:K] if K else None
    prior = (np.array([1.0, 2.0]), np.array([0.3, np.inf])) if K else None
    B = np.full(C, 0.25)
    truth = np.array([40.0, 10.0, 25.0])
    mean = (truth[:, None] * detector.events_host(R3[0].reshape(3, M, C), S[0])).sum(axis=0) + B
    mean = mean + (np.array([1.0, 2.0]) @ T if K else 0.0)
    data = rng.poisson(mean).astype(np.float64)
    phi = triangle(3)                                            # 10 points
    fixed, free = _scan_host(R3, S, data, phi, T, prior, B)
    assert not np.any((fixed[3] | free[3][:, None]) & (FIT_SINGULAR | FIT_NOT_CONVERGED | FIT_INFINITE))
    lam, mag = detector.composition_statistic(fixed[2], fixed[0], free[2][:, None], free[0][:, None], data, prior=prior,
                                              log=math.log)
    assert lam.shape == mag.shape == (ntab, len(phi), Q)
    m, w = detector._prior(K, prior)
    sig = [detector.events_host(R3[:, j], S) for j in range(3)]
    for t in range(ntab):
        for c in range(len(phi)):
            for q in range(Q):
                muh, thh = free[2][t, q], free[0][t, q]
                want = detector._limit_lambda(fixed[0][t, c, q, 0], fixed[0][t, c, q, 1:], fixed[2][t, c, q], muh, thh[3:],
                                              (data > 0) & (muh > 0), data, m[1:], w[1:], math.log)
                assert (lam[t, c, q], mag[t, c, q]) == want, (t, c, q)
                X = np.vstack([np.stack([s[t, q] for s in sig])] + ([T] if K else []))
                ok = allowance(fixed[2][t, c, q], fixed[0][t, c, q], muh, thh, phi[c], X, data, prior, mag[t, c, q], M)
                assert lam[t, c, q] >= -ok, (t, c, q, lam[t, c, q], ok)
    assert np.any(lam > 1e-3)                                   # (the grid's corners are far from the data's composition)
    # the free fit's own signal theta_hat as the weights: the held fit's scale ends near 1 and lambda within the allowance of 0
    for t in range(ntab):
        own = free[0][t, :, :3]                                  # (Q, 3): one composition per spectrum
        fx, fr = _scan_host(R3[t:t + 1], S, data, own, T, prior, B)
        lam2, mag2 = detector.composition_statistic(fx[2], fx[0], fr[2][:, None], fr[0][:, None], data, prior=prior, log=math.log)
        for q in range(Q):
            X = np.vstack([np.stack([s[t, q] for s in sig])] + ([T] if K else []))
            ok = allowance(fx[2][0, q, q], fx[0][0, q, q], fr[2][0, q], fr[0][0, q], own[q], X, data, prior, mag2[0, q, q], M)
            assert abs(fx[0][0, q, q, 0] - 1.0) < 1e-6 and abs(lam2[0, q, q]) <= ok, (t, q, lam2[0, q, q], ok)
            print("K=%d t=%d q=%d: lambda at the own composition %.3e, allowance %.3e" % (K, t, q, lam2[0, q, q], ok))
