"""The fit with floating background templates on the CPU: detector.fit_host, the host form of nusi_plan_response_fit
(include/nusi.h; DESIGN.md sec. 4, "The fit with floating templates").

  * fit_host against a scalar loop on Python floats written from the header's text: equal bits;
  * the algebra by hand where it can be done (C = 1, C = 2, a template pinned by a tight prior);
  * optimality in EXACT arithmetic (fractions.Fraction) at the returned doubles: every free component has
    |g_j| <= K_fit u scale_j, every component at zero g_j >= -K_fit u scale_j, K_fit = detector.K_fit(C, K);
  * checks that do not share the algorithm: the statistic is not smaller nearby or at the start, Asimov data give the
    generating theta back;
  * the flags, the shapes, the refusals, the ABI.

The plan-level refusals (set_templates, fit) need a plan and so a GPU: tests/test_fit_gpu.py.
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

U = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --- the scalar loop: the header's text on Python floats ---------------------------------------------------------------
def _tree(x):
    P = 1
    while P < len(x):
        P *= 2
    v = list(x) + [0.0] * (P - len(x))
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def _ldl(H, g, F, n):
    """p = -H^-1 g on F; None if a pivot is not > 0."""
    a = [[(H[i][j] if F[i] and F[j] else float(i == j)) for j in range(n)] for i in range(n)]
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    for i in range(n):
        c = []
        for j in range(i):
            x = a[i][j]
            for k in range(j):
                x -= c[k] * L[j][k]
            c.append(x)
            L[i][j] = x / D[j]
        x = a[i][i]
        for k in range(i):
            x -= c[k] * L[i][k]
        if not x > 0.0:
            return None
        D[i] = x
    y = []
    for i in range(n):
        x = -g[i] if F[i] else 0.0
        for k in range(i):
            x -= L[i][k] * y[k]
        y.append(x)
    p = [0.0] * n
    for i in reversed(range(n)):
        x = y[i] / D[i]
        for k in range(i + 1, n):
            x -= L[k][i] * p[k]
        p[i] = x
    return p


def fit_scalar(s, T, B, d, m, w, kappa):
    """One fit.  s, B, d: lists [C]; T: K lists; m, w: lists [1 + K] (zeros in front).  Returns (theta, status)."""
    X = [list(s)] + [list(t) for t in T]
    n, C = len(X), len(s)
    S1 = [_tree(X[j]) for j in range(n)]
    live = [S1[j] > 0.0 for j in range(n)]
    live[0] = live[0] and any(d[c] > 0.0 and s[c] > 0.0 for c in range(C))
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
        return bad, g, H, S2

    flags = steps = halvings = 0
    bad, g, H, S2 = evaluate(theta)
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
            bad_x, g_x, H_x, S2_x = evaluate(x)
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
    if not live[0]:
        flags |= FIT_FLAT
    elif theta[0] == 0.0:
        flags |= FIT_BOUNDARY
    for j in range(n):
        if theta[j] == 0.0:
            flags |= FIT_ZERO << j
    return theta, steps | flags | (min(halvings, FIT_TRIALS_MASK) << FIT_TRIALS_SHIFT)


# --- seeded cases ------------------------------------------------------------------------------------------------------
BKINDS = ("none", "tiny", "big")
PRIORS = ("none", "loose near", "tight near", "loose far", "tight far")


def make_case(C, K, seed, bkind="none", collinear=False, zero=None, pkind="none", asimov=False):
    """(s, T, B, data, prior, truth): one spectrum's signal s [C] (its matrix is R = [0, s], S = [0, 1]), templates
    exp(-gamma x) with scales over decades, data Poisson or Asimov around truth, at least 1 + K bins with data."""
    rng = np.random.default_rng([seed, C, K])
    x = np.linspace(0.0, 3.0, C) if C > 1 else np.zeros(1)
    g0 = rng.uniform(0.2, 1.0)
    s = np.exp(-g0 * x) * (0.7 + 0.6 * rng.random(C)) * 10.0 ** rng.uniform(-6, 6)
    gam = [g0 + 0.1 * (j + 1) for j in range(K)] if collinear else [g0 + rng.uniform(0.4, 0.9) * (j + 1) for j in range(K)]
    T = np.stack([np.exp(-gam[j] * x) * (1.0 if collinear else 0.7 + 0.6 * rng.random(C)) * 10.0 ** rng.uniform(-3, 3)
                  for j in range(K)])
    counts = 10.0 ** rng.uniform(1.5, 3.5, 1 + K)                # events of each component in its fullest bin
    truth = counts / np.array([s.max()] + [T[j].max() for j in range(K)])
    if zero is not None:
        truth[zero] = 0.0
    sig = truth[0] * s
    B = {"none": np.zeros(C), "tiny": np.full(C, 1e-300), "big": 1e3 * sig + 1.0}[bkind]
    mean = truth @ np.vstack([s[None], T]) + B
    if asimov:
        data = np.array([float(sum(Fraction(float(truth[j])) * Fraction(float(X)) for j, X in enumerate([s[c]] + list(T[:, c])))
                               + Fraction(float(B[c]))) for c in range(C)])
    else:
        data = rng.poisson(mean).astype(np.float64)
        data[np.argsort(mean)[-(1 + K):]] += 1.0                 # (at least 1 + K bins with data)
    prior = None
    if pkind != "none":
        width, where = pkind.split()
        rel = {"loose": 3.0, "tight": 1e-3}[width]
        centre = truth[1:] * ({"near": 1.0, "far": 5.0}[where]) + (0.0 if where == "near" else 1.0 / T.max(axis=1))
        prior = (centre, rel * np.maximum(centre, 1.0 / T.max(axis=1)))
    return s, T, B, data, prior, truth


def run(s, T, B, data, prior):
    R = np.zeros((2, len(s)))
    R[1] = s
    th, nll, mu, st = detector.fit_host(R, np.array([0.0, 1.0]), data, T, prior=prior, background=B, log=math.log)
    return th, float(nll), mu, int(st)


CASES = [(C, K) for C in (1, 2, 3, 5, 17, 64) for K in (1, 2, 3)]
# the optimality classes hold only the cases whose data can determine every component: at least 1 + K bins
DETERMINED = [(C, K) for C, K in CASES if C >= 1 + K]
VARIANTS = ([dict(bkind=b) for b in BKINDS] + [dict(collinear=True), dict(collinear=True, bkind="tiny")]
            + [dict(zero=1), dict(zero=0, bkind="big"), dict(zero=1, pkind="loose near")]
            + [dict(pkind=p) for p in PRIORS[1:]] + [dict(asimov=True), dict(asimov=True, bkind="tiny", pkind="tight far")])
SEEDS = (1, 2)


# --- fit_host against the scalar loop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", CASES)
def test_fit_host_equals_the_scalar_loop(C, K):
    seen = 0
    for v, variant in enumerate(VARIANTS):
        s, T, B, data, prior, _ = make_case(C, K, seed=10 + v, **variant)
        th, nll, mu, st = run(s, T, B, data, prior)
        m, w = detector._prior(K, prior)
        th2, st2 = fit_scalar(list(map(float, s)), [list(map(float, t)) for t in T], list(map(float, B)),
                              list(map(float, data)), list(map(float, m)), list(map(float, w)), detector.fit_kappa(C, K))
        assert st == st2, (variant, hex(st), hex(st2))
        assert th.tolist() == th2, variant
        den = [float(B[c]) for c in range(C)]
        for c in range(C):
            v_ = th2[0] * float(s[c])
            for j in range(K):
                v_ = v_ + th2[1 + j] * float(T[j, c])
            den[c] = v_ + float(B[c])
        assert mu.tolist() == den, variant
        seen |= st
    # the comparison has something to compare: steps everywhere, and halvings and pinned components where the data
    # can determine the components at all
    assert seen & FIT_STEPS_MASK and (C < 5 or ((seen >> FIT_TRIALS_SHIFT) and seen & (0xF * FIT_ZERO))), hex(seen)


def test_the_statistic_and_its_penalties():
    """nll = the events call's serial statistic of mu, then the penalties in ascending j, each operation rounded."""
    s, T, B, data, prior, _ = make_case(5, 3, seed=3, pkind="loose far")
    th, nll, mu, st = run(s, T, B, data, prior)
    m, w = detector._prior(3, prior)
    want = float(detector.poisson_host(mu, data, log=math.log))
    for j in range(1, 4):
        dl = float(th[j]) - float(m[j])
        want = want + ((0.5 * float(w[j])) * dl) * dl
    assert nll == want and np.all(w[1:] > 0)


# --- the algebra by hand --------------------------------------------------------------------------------------------------
def _exact_gradient(s, T, B, data, m, w, th):
    """(g, scale) of f at th in exact arithmetic on the doubles given; the bins with data and nothing expected (the
    INFINITE ones) stay out, as in the header."""
    X = [[Fraction(float(v)) for v in s]] + [[Fraction(float(v)) for v in t] for t in T]
    n, C = len(X), len(s)
    th = [Fraction(float(v)) for v in th]
    g, scale = [], []
    for j in range(n):
        S1 = sum(X[j])
        S2 = Fraction(0)
        for c in range(C):
            if data[c] > 0 and X[j][c] > 0:
                den = sum(th[k] * X[k][c] for k in range(n)) + Fraction(float(B[c]))
                S2 += X[j][c] * Fraction(float(data[c])) / den
        wj, mj = Fraction(float(w[j])), Fraction(float(m[j]))
        g.append(S1 - S2 + wj * (th[j] - mj))
        scale.append(S1 + S2 + wj * (th[j] + mj))
    return g, scale


def _theta_bound(s, T, B, data, m, w, th, C, K, extra=0.0):
    """The residual bound carried through the Hessian: two points whose gradients differ by at most r_j = (K_fit u +
    extra) scale_j on the components away from zero differ by at most 2 |H^-1| r there (2: the Hessian between them
    against the one at th, for differences this small)."""
    X = np.vstack([np.asarray(s)[None], T])
    den = th @ X + B
    keep = np.array(th) > 0
    act = data > 0
    H = (X[:, act] * (data[act] / den[act] ** 2)) @ X[:, act].T + np.diag(w)
    _, scale = _exact_gradient(s, T, B, data, m, w, th)
    r = (detector.K_fit(C, K) * U + extra) * np.array([float(v) for v in scale])
    out = np.zeros(1 + K)
    out[keep] = 2.0 * np.abs(np.linalg.inv(H[np.ix_(keep, keep)])) @ r[keep]
    return out


@pytest.mark.parametrize("C", (1, 2))
def test_a_pinned_template_by_hand(C):
    """data = a s + m T + B exactly, with the prior's mean at m: the gradient vanishes at (a, m) whatever the width, and
    with one bin per component short (C = 1) only the prior tells the two apart.  Then, at C = 1, data BELOW m T: the
    signal ends at zero and theta_1 solves w t^2 + (T - w m) t - d = 0."""
    s, T = np.array([2.0, 0.5][:C]), np.array([[3.0, 8.0][:C]])
    B = np.array([1.0, 0.25][:C])
    a, mean = 18.5, 4.0
    data = a * s + mean * T[0] + B                                # exact in doubles: 50, 41.5
    for sigma in (1e-3, 1e-6):
        prior = (np.array([mean]), np.array([sigma]))
        th, nll, mu, st = run(s, T, B, data, prior)
        m, w = detector._prior(1, prior)
        assert not st & ~(FIT_STEPS_MASK | (FIT_TRIALS_MASK << FIT_TRIALS_SHIFT)), hex(st)
        bound = _theta_bound(s, T, B, data, m, w, th, C, 1)
        assert np.all(np.abs(th - [a, mean]) <= bound), (th, bound)
        assert np.all(np.abs(mu - data) <= np.abs(np.vstack([s[None], T])).T @ bound + 4 * U * data)
    if C == 1:
        d, w_ = 7.0, 1.0 / (1e-2 * 1e-2)
        prior = (np.array([mean]), np.array([1e-2]))
        th, nll, mu, st = run(s, T, np.zeros(1), np.array([d]), prior)
        tq = (-(3.0 - w_ * mean) + math.sqrt((3.0 - w_ * mean) ** 2 + 4.0 * w_ * d)) / (2.0 * w_)
        m, w = detector._prior(1, prior)
        assert st & FIT_BOUNDARY and st & FIT_ZERO and th[0] == 0.0 and not st & (FIT_SINGULAR | FIT_NOT_CONVERGED)
        # (tq itself: a square root, a difference of nearly equal numbers, a division -- 8 u w m / w relative to m)
        assert abs(th[1] - tq) <= _theta_bound(s, T, np.zeros(1), np.array([d]), m, w, th, 1, 1)[1] + 8 * U * mean


# --- optimality in exact arithmetic -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", DETERMINED)
def test_optimality_in_exact_arithmetic(C, K):
    Kf = detector.K_fit(C, K)
    worst, steps, halv = 0.0, [], []
    for v, variant in enumerate(VARIANTS):
        for seed in SEEDS:
            s, T, B, data, prior, truth = make_case(C, K, seed=100 * seed + v, **variant)
            assert np.count_nonzero(data) >= 1 + K
            th, nll, mu, st = run(s, T, B, data, prior)
            assert not st & (FIT_NOT_CONVERGED | FIT_SINGULAR | FIT_INFINITE | FIT_FLAT), (variant, seed, hex(st))
            m, w = detector._prior(K, prior)
            g, scale = _exact_gradient(s, T, B, data, m, w, th)
            for j in range(1 + K):
                ratio = g[j] / (Fraction(U) * scale[j])
                if th[j] > 0:
                    assert abs(ratio) <= Kf, (variant, seed, j, float(ratio), Kf)
                    worst = max(worst, abs(float(ratio)))
                else:
                    assert ratio >= -Kf and st & (FIT_ZERO << j), (variant, seed, j, float(ratio))
            steps.append(st & FIT_STEPS_MASK)
            halv.append((st >> FIT_TRIALS_SHIFT) & FIT_TRIALS_MASK)
    print("C=%d K=%d: worst |g| / (u scale) %.2f of K_fit %d (kappa %d); steps mean %.2f max %d, halvings mean %.2f max %d" % (
        C, K, worst, Kf, detector.fit_kappa(C, K), np.mean(steps), max(steps), np.mean(halv), max(halv)))


@pytest.mark.parametrize("C,K", DETERMINED)
def test_a_component_that_is_not_there_ends_pinned(C, K):
    """Asimov data of a truth with theta_j = 0 under a fixed background: the component ends at exactly zero with its
    bit set (its gradient at the truth is 0 and the others explain the data)."""
    for j in range(1 + K):
        s, T, B, data, prior, truth = make_case(C, K, seed=7 + j, bkind="none", zero=j, asimov=True)
        th, nll, mu, st = run(s, T, B, data, prior)
        assert not st & (FIT_NOT_CONVERGED | FIT_SINGULAR), hex(st)
        m, w = detector._prior(K, prior)
        bound = _theta_bound(s, T, B, data, m, w, np.where(truth > 0, truth, 0.0), C, K, extra=U)
        # at zero, or within the bound of it (the exact gradient there is 0: either side of the boundary is optimal)
        g, scale = _exact_gradient(s, T, B, data, m, w, th)
        assert th[j] == 0.0 or abs(g[j]) <= detector.K_fit(C, K) * Fraction(U) * scale[j], (j, th)
        if th[j] == 0.0:
            assert st & (FIT_ZERO << j) and (j > 0 or st & FIT_BOUNDARY)
            assert np.all(np.abs(th - truth) <= bound), (j, th, truth, bound)


# --- checks that do not share the algorithm ---------------------------------------------------------------------------------
def _f(s, T, B, data, m, w, th):
    """(f, the sum of its terms' magnitudes) at th, by math.fsum."""
    mu = th[0] * s + th[1:] @ T + B
    terms = [float(v) for v in mu] + [-float(dc) * math.log(float(v)) for v, dc in zip(mu, data) if dc > 0]
    terms += [0.5 * float(w[j]) * (float(th[j]) - float(m[j])) ** 2 for j in range(1, len(th))]
    return math.fsum(terms), math.fsum(abs(v) for v in terms)


@pytest.mark.parametrize("C,K", DETERMINED)
def test_the_statistic_is_not_smaller_nearby(C, K):
    """f(theta_hat) is not above f with each component moved by +-1e-3 relative (a component at zero: by 1e-3 of its
    equal-share start, upwards) and not above f at the start -- up to the rounding of f itself, 4 (C + K + 3) u times
    the sum of its terms' magnitudes: a log within an ulp, a product and a difference per term, fsum exact."""
    for v, variant in enumerate(VARIANTS):
        s, T, B, data, prior, truth = make_case(C, K, seed=300 + v, **variant)
        th, nll, mu, st = run(s, T, B, data, prior)
        m, w = detector._prior(K, prior)
        f0, mag = _f(s, T, B, data, m, w, th)
        slack = 4 * (C + K + 3) * U * mag
        start = data.sum() / ((1 + K) * np.array([s.sum()] + [t.sum() for t in T]))
        others = [start]
        for j in range(1 + K):
            for sign in (1.0, -1.0):
                o = th.copy()
                o[j] = max(0.0, th[j] * (1.0 + sign * 1e-3)) if th[j] > 0 else (1e-3 * start[j] if sign > 0 else 0.0)
                others.append(o)
        for o in others:
            f1, mag1 = _f(s, T, B, data, m, w, o)
            assert f0 <= f1 + slack + 4 * (C + K + 3) * U * mag1, (variant, o, f0, f1)
        # the reported nll is that statistic: the serial sum against fsum
        assert abs(nll - f0) <= slack, (nll, f0)


@pytest.mark.parametrize("C,K", DETERMINED)
def test_asimov_data_give_the_truth_back(C, K):
    """data = the exact mu(truth) rounded once: the truth's own gradient is at most u S1_j, the fit's at most
    K_fit u scale_j, and the two points differ by at most those residuals carried through the Hessian."""
    for v, variant in enumerate((dict(), dict(bkind="tiny"), dict(bkind="big"), dict(pkind="loose near"), dict(pkind="tight near"))):
        s, T, B, data, prior, truth = make_case(C, K, seed=500 + v, asimov=True, **variant)
        th, nll, mu, st = run(s, T, B, data, prior)
        assert not st & (FIT_NOT_CONVERGED | FIT_SINGULAR), hex(st)
        m, w = detector._prior(K, prior)
        bound = _theta_bound(s, T, B, data, m, w, truth, C, K, extra=U)
        assert np.all(np.abs(th - truth) <= bound), (variant, th, truth, bound)


# --- flags --------------------------------------------------------------------------------------------------------------------
def test_singular():
    s, T, B, data, _, _ = make_case(5, 2, seed=1)
    T[1] = T[0]                                                 # two identical templates
    th, nll, mu, st = run(s, T, B, data, None)
    assert st & FIT_SINGULAR and not st & FIT_NOT_CONVERGED
    s, T, B, data, _, _ = make_case(5, 3, seed=2)
    data[:] = 0.0
    data[1], data[3] = 4.0, 9.0                                 # two bins with data, four components
    th, nll, mu, st = run(s, T, B, data, None)
    assert st & FIT_SINGULAR
    th, nll, mu, st = run(s, T, B, data, (np.ones(3), np.ones(3)))        # priors on three of the four: determined
    assert not st & (FIT_SINGULAR | FIT_NOT_CONVERGED)


def test_flat_with_a_zero_signal_still_fits_the_templates():
    s, T, B, data, _, truth = make_case(17, 2, seed=4, zero=0, asimov=True)
    th, nll, mu, st = run(np.zeros(17), T, B, data, None)
    assert st & FIT_FLAT and not st & FIT_BOUNDARY and st & FIT_ZERO and th[0] == 0.0
    assert not st & (FIT_SINGULAR | FIT_NOT_CONVERGED) and st & FIT_STEPS_MASK
    m, w = detector._prior(2, None)
    assert np.all(np.abs(th[1:] - truth[1:]) <= _theta_bound(s, T, B, data, m, w, truth, 17, 2, extra=U)[1:])
    # ... and with a signal only where there are no data
    s2 = np.zeros(17)
    s2[3] = 5.0
    d2 = data.copy()
    d2[3] = 0.0
    th2, _, _, st2 = run(s2, T, B, d2, None)
    assert st2 & FIT_FLAT and th2[0] == 0.0 and np.any(th2[1:] > 0) and st2 & FIT_STEPS_MASK
    assert not st2 & (FIT_SINGULAR | FIT_NOT_CONVERGED)


def test_infinite_leaves_theta_alone():
    s, T, B, data, _, _ = make_case(17, 2, seed=5)
    s[16], T[:, 16], B[16], data[16] = 0.0, 0.0, 0.0, 0.0
    th, nll, mu, st = run(s, T, B, data, None)
    d2 = data.copy()
    d2[16] = 3.0                                                # a count where nothing can ever be expected
    th2, nll2, mu2, st2 = run(s, T, B, d2, None)
    assert not st & FIT_INFINITE and math.isfinite(nll)
    assert st2 == st | FIT_INFINITE and nll2 == math.inf and np.array_equal(th2, th) and np.array_equal(mu2, mu)


def test_no_data_at_all():
    s, T, B, data, _, _ = make_case(5, 3, seed=6, bkind="big")
    th, nll, mu, st = run(s, T, B, np.zeros(5), None)
    assert np.all(th == 0.0) and st == FIT_FLAT | 0xF * FIT_ZERO and np.array_equal(mu, B)
    # with a prior the template follows it: theta = max(0, m - S1 / w), one Newton step on a quadratic
    prior = (np.array([2.0, 2.0, 2.0]), np.array([np.inf, 1e-3 / T[1].sum() ** 0.5, 1e3]))
    th, nll, mu, st = run(s, T, B, np.zeros(5), prior)
    m, w = detector._prior(3, prior)
    assert th[0] == 0.0 and th[1] == 0.0 and th[3] == 0.0
    assert abs(th[2] - (2.0 - T[1].sum() / w[2])) <= 8 * U * 2.0 and (st & FIT_STEPS_MASK) >= 1


# --- shapes, refusals, the ABI ------------------------------------------------------------------------------------------------
def test_shapes_and_refusals_of_fit_host():
    rng = np.random.default_rng(0)
    M, C, K = 6, 5, 2
    R, S = rng.random((3, M, C)), rng.random((4, M))
    T, data = rng.random((K, C)), rng.poisson(20.0, C).astype(float)
    th, nll, mu, st = detector.fit_host(R, S, data, T)
    assert th.shape == (3, 4, 1 + K) and nll.shape == (3, 4) and mu.shape == (3, 4, C)
    assert st.shape == (3, 4) and st.dtype == np.int32
    one = detector.fit_host(R[1], S[2], data, T)
    assert one[0].shape == (1 + K,) and one[2].shape == (C,) and one[1].shape == () and one[3].shape == ()
    assert np.array_equal(one[0], th[1, 2]) and one[1] == nll[1, 2] and one[3] == st[1, 2]
    assert detector.fit_host(R, S, data, T[0])[0].shape == (3, 4, 2)          # one template as a vector
    prior = (np.ones(K), np.array([0.5, np.inf]))
    assert np.array_equal(detector.fit_host(R, S, data, T, prior=(None, None))[0], th)
    assert not np.array_equal(detector.fit_host(R, S, data, T, prior=prior)[0], th)
    for bad in (dict(templates=rng.random((4, C))), dict(templates=rng.random((K, C + 1))), dict(templates=-T),
                dict(templates=np.vstack([T[:1], np.zeros((1, C))])), dict(templates=np.where(T > 0.5, np.nan, T)),
                dict(data=data[:-1]), dict(data=-data), dict(data=np.where(data > 18, np.inf, data)),
                dict(prior=(np.ones(K), np.array([0.0, 1.0]))), dict(prior=(np.ones(K), np.array([np.nan, 1.0]))),
                dict(prior=(np.array([-1.0, 1.0]), np.ones(K))), dict(prior=(np.array([np.inf, 1.0]), np.ones(K)))):
        kw = dict(templates=T, data=data, prior=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            detector.fit_host(R, S, kw["data"], kw["templates"], prior=kw["prior"])
    with pytest.raises(ValueError):
        detector.fit_host(R[:, :-1], S, data, T)


def test_abi():
    """The header's constants are the package's; the new calls are declared, bound and exported; without a plan they
    refuse."""
    from nusiprop_amd import _lib
    text = open(os.path.join(ROOT, "include", "nusi.h")).read()
    macro = {k: int(v, 0) for k, v in re.findall(r"^#define (NUSI_FIT_[A-Z_]+) (\S+)$", text, flags=re.M)}
    macro.update({k: int(v, 0) for k, v in re.findall(r"^    (NUSI_FIT_[A-Z_]+) = (\w+),?$", text, flags=re.M)})
    for name in ("TEMPLATES_MAX", "TRIALS_MAX", "SINGULAR", "ZERO", "TRIALS_SHIFT", "TRIALS_MASK", "ITER_MAX", "FLAT",
                 "BOUNDARY", "NOT_CONVERGED", "INFINITE", "STEPS_MASK"):
        assert macro["NUSI_FIT_" + name] == getattr(detector, "FIT_" + name) == getattr(_lib, "FIT_" + name), name
    assert macro["NUSI_FIT_SINGULAR"] == 0x1000 and macro["NUSI_FIT_ZERO"] == 1 << 16 and macro["NUSI_FIT_TEMPLATES_MAX"] == 3
    flags = [macro["NUSI_FIT_" + k] for k in ("FLAT", "BOUNDARY", "NOT_CONVERGED", "INFINITE", "SINGULAR")]
    fields = flags + [macro["NUSI_FIT_STEPS_MASK"], 0xF * macro["NUSI_FIT_ZERO"],
                      macro["NUSI_FIT_TRIALS_MASK"] << macro["NUSI_FIT_TRIALS_SHIFT"]]
    assert sum(fields) == np.bitwise_or.reduce(fields) < 2 ** 31           # disjoint, and the word stays positive
    new = ("nusi_plan_set_templates", "nusi_plan_templates", "nusi_plan_response_fit", "nusi_plan_response_fit_host")
    L = _lib.load()
    for name in new:
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name).argtypes is not None
    assert L.nusi_plan_templates(None) == 0
    dp = ctypes.POINTER(ctypes.c_double)
    one = np.ones(4)
    p = one.ctypes.data_as(dp)
    assert L.nusi_plan_set_templates(None, 1, p, None, None) in (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_response_fit(None, None, 1, p, 1, p, None, None, None, None, None) in (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_response_fit_host(None, p, 1, p, 1, p, p, None, None, None) in (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert detector.K_fit(64, 3) == detector.fit_kappa(64, 3) + 6 + 6 + 9 and detector.fit_kappa(1, 1) == 20
