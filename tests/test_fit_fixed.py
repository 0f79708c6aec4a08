"""The conditional fit on the CPU: detector.fit_fixed_host, the host form of nusi_plan_response_fit_fixed (include/nusi.h;
DESIGN.md sec. 4, "The conditional fit and limits on the signal scale") -- the fit's templates with the signal's scale
held.

The yardsticks are the EXISTING host forms, which know nothing of the new text:

  * K = 1 without a prior is a one-parameter problem: profile_host with the template as its "signal" (a two-row matrix
    R' = [0, T_1], S' = [0, 1]) on the background a s + B;
  * K = 2, 3 with no prior on T_1: fit_host with T_1 as its signal, T_2 .. as its templates, on that background;
  * optimality in EXACT arithmetic (fractions.Fraction, test_fit's gradient) at the returned doubles;
  * the global fit: the conditional minimum is nowhere below fit_host's, and equals it at a = theta_hat_0.

Bounds.  Two minimisers that each leave a residual gradient of at most r_j differ by at most 2 |H^-1| (r + r') on the
components away from zero (test_fit._theta_bound's argument: the Hessian between them against the one at the point, for
differences this small).  r is the stop's allowance of each form in exact arithmetic -- K_fit(C, K) u scale_j for the
conditional fit and for fit_host (with its own K), (2 ceil(log2 C) + 18) u (S1 + S2) for profile_host (the header's) --
plus 2 u scale_j for the yardstick's background, which is fl(fl(a s) + B) where the conditional fit's den holds a s and
B exactly: two relative roundings of den move S2_j by at most 2 u S2_j <= 2 u scale_j.  For K = 1 the Hessian is the
curvature S3 = sum d T^2 / mu^2.
"""
import math

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_NOT_CONVERGED, FIT_SINGULAR,
                                   FIT_STEPS_MASK, FIT_ZERO)
from tests.test_fit import DETERMINED, VARIANTS, _exact_gradient, make_case

U = 2.0 ** -53
SCALES = (0.0, 0.5, 1.0, 3.0)                       # of theta_hat_0: the background-only fit, both sides, the best fit


def _R(s):
    R = np.zeros((2, len(s)))
    R[1] = s
    return R


S01 = np.array([0.0, 1.0])


def run_fixed(s, T, B, data, prior, a):
    th, nll, mu, st = detector.fit_fixed_host(_R(s), S01, a, data, T, prior=prior, background=B, log=math.log)
    return th, float(nll), mu, int(st)


def run_fit(s, T, B, data, prior):
    th, nll, mu, st = detector.fit_host(_R(s), S01, data, T, prior=prior, background=B, log=math.log)
    return th, float(nll), mu, int(st)


def _no_prior_on_first(prior):
    if prior is None:
        return None
    mean, sigma = np.array(prior[0], dtype=np.float64), np.array(prior[1], dtype=np.float64)
    sigma[0] = np.inf
    return mean, sigma


def _nll_bound(mu, data, theta, m, w):
    """test_fit_gpu._check's bound on a computed nll: 2 (C + 3 + 3 K) u (sum_c (mu_c + |d_c log mu_c|) + penalties)."""
    C, K = len(data), len(theta) - 1
    mag = float(np.sum(mu + np.where(data > 0, np.abs(data * np.log(np.where(mu > 0, mu, 1.0))), 0.0)))
    mag += float(np.sum(0.5 * w * (theta - m) ** 2))
    return 2 * (C + 3 + 3 * K) * U * mag


def _cases(K_of=(1, 2, 3), first_free=False):
    """(C, K, variant index, s, T, B, data, prior, theta_hat_0) over test_fit's determined classes; first_free: T_1 without
    a prior."""
    for C, K in DETERMINED:
        if K not in K_of:
            continue
        for v, variant in enumerate(VARIANTS):
            s, T, B, data, prior, _ = make_case(C, K, seed=300 + v, **variant)
            if first_free:
                prior = _no_prior_on_first(prior)
            th, _, _, st = run_fit(s, T, B, data, prior)
            assert not st & (FIT_NOT_CONVERGED | FIT_SINGULAR), (C, K, variant)
            yield C, K, v, s, T, B, data, prior, float(th[0])


def _held_scales(a_hat, s):
    """The held scales of a case: SCALES times the best fit's, and where that is zero a scale of 100 signal events."""
    ref = a_hat if a_hat > 0 else 100.0 / float(s.max())
    return [f * ref for f in SCALES]


def _diff_bound(a, s, T, B, data, m, w, theta, const):
    """2 |H^-1| r on the templates away from zero, r_j = const u scale_j: the module's docstring."""
    K = len(T)
    den = a * s + theta[1:] @ T + B
    act = data > 0
    H = (T[:, act] * (data[act] / den[act] ** 2)) @ T[:, act].T + np.diag(w[1:])
    _, scale = _exact_gradient(s, T, B, data, m, w, theta)
    r = const * U * np.array([float(v) for v in scale[1:]])
    keep = theta[1:] > 0
    out = np.zeros(K)
    if keep.any():
        out[keep] = 2.0 * np.abs(np.linalg.inv(H[np.ix_(keep, keep)])) @ r[keep]
    return out


# --- K = 1 against the profile ------------------------------------------------------------------------------------------
def test_one_template_against_the_profile():
    seen = worst = 0
    for C, K, v, s, T, B, data, prior, a_hat in _cases(K_of=(1,)):
        if prior is not None:
            continue                                # (the profile has no prior)
        L = detector._ceil_log2(C)
        for a in _held_scales(a_hat, s):
            th, nll, mu, st = run_fixed(s, T, B, data, None, a)
            assert not st & (FIT_NOT_CONVERGED | FIT_SINGULAR | FIT_FLAT | FIT_BOUNDARY | FIT_ZERO), (C, v, a, hex(st))
            bgp = a * s + B                          # fl(fl(a s) + B)
            ap, _, _, sp = detector.profile_host(_R(T[0]), S01, data, background=bgp, log=math.log)
            ap, sp = float(ap), int(sp)
            assert not sp & FIT_NOT_CONVERGED, (C, v, a)
            if ap == 0.0 or th[1] == 0.0:           # at the bound: both, or the other within the bound of zero
                assert bool(sp & (FIT_BOUNDARY | FIT_FLAT)) == bool(st & (FIT_ZERO << 1)) or max(ap, th[1]) <= _diff_bound(
                    a, s, T, B, data, np.zeros(2), np.zeros(2), np.array([a, max(ap, th[1])]),
                    detector.K_fit(C, 1) + 2 * L + 18 + 2)[0], (C, v, a, ap, th[1])
                continue
            bound = _diff_bound(a, s, T, B, data, np.zeros(2), np.zeros(2), th, detector.K_fit(C, 1) + 2 * L + 18 + 2)[0]
            assert abs(th[1] - ap) <= bound, (C, v, a, th[1], ap, bound)
            worst = max(worst, abs(th[1] - ap) / bound)
            seen += 1
    print("conditional K = 1 against profile_host: %d comparisons, worst ratio to the bound %.3f" % (seen, worst))
    assert seen >= 40


# --- K = 2, 3 against the fit with T_1 as its signal ----------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 3))
def test_more_templates_against_the_fit(K):
    seen = worst = 0
    for C, _, v, s, T, B, data, prior, a_hat in _cases(K_of=(K,), first_free=True):
        m, w = detector._prior(K, prior)
        sub = None if prior is None else (np.asarray(prior[0])[1:], np.asarray(prior[1])[1:])
        for a in _held_scales(a_hat, s):
            th, nll, mu, st = run_fixed(s, T, B, data, prior, a)
            tf, nf, mf, sf = detector.fit_host(_R(T[0]), S01, data, T[1:], prior=sub, background=a * s + B, log=math.log)
            assert not st & (FIT_NOT_CONVERGED | FIT_SINGULAR) and not int(sf) & (FIT_NOT_CONVERGED | FIT_SINGULAR), (C, v, a)
            const = detector.K_fit(C, K) + detector.K_fit(C, K - 1) + 2
            both = np.array([a] + [max(x, y) for x, y in zip(th[1:], tf)])
            bound = _diff_bound(a, s, T, B, data, m, w, both, const)
            assert np.all(np.abs(th[1:] - tf) <= bound), (C, v, a, th[1:], tf, bound)
            nz = bound > 0
            if nz.any():
                worst = max(worst, float(np.max(np.abs(th[1:] - tf)[nz] / bound[nz])))
            seen += 1
    print("conditional K = %d against fit_host: %d comparisons, worst ratio to the bound %.3f" % (K, seen, worst))
    assert seen >= 100


# --- KKT in exact arithmetic, the word, mu's bits ------------------------------------------------------------------------
@pytest.mark.parametrize("C,K", DETERMINED)
def test_kkt_in_exact_arithmetic(C, K):
    Kf = detector.K_fit(C, K)
    worst, seen = 0.0, 0
    for v, variant in enumerate(VARIANTS):
        s, T, B, data, prior, _ = make_case(C, K, seed=300 + v, **variant)
        a_hat = float(run_fit(s, T, B, data, prior)[0][0])
        m, w = detector._prior(K, prior)
        for a in _held_scales(a_hat, s):
            th, nll, mu, st = run_fixed(s, T, B, data, prior, a)
            assert not st & (FIT_NOT_CONVERGED | FIT_SINGULAR | FIT_INFINITE), (variant, a, hex(st))
            assert not st & (FIT_FLAT | FIT_BOUNDARY | FIT_ZERO) and th[0] == a, (variant, a, hex(st))
            assert np.all(th >= 0)
            for j in range(1, 1 + K):
                assert bool(st & (FIT_ZERO << j)) == (th[j] == 0.0)
            den = a * s                             # the fit's den at (a, theta): the same bits
            for j in range(K):
                den = den + th[1 + j] * T[j]
            assert np.array_equal(mu, den + B)
            g, scale = _exact_gradient(s, T, B, data, m, w, th)
            for j in range(1, 1 + K):
                ratio = float(g[j] / scale[j]) / U
                if th[j] > 0:
                    assert abs(ratio) <= Kf, (variant, a, j, ratio)
                    worst = max(worst, abs(ratio))
                else:
                    assert ratio >= -Kf, (variant, a, j, ratio)
            seen |= st
    print("C=%d K=%d: largest exact residual %.1f u scale against K_fit = %d" % (C, K, worst, Kf))
    assert seen & FIT_STEPS_MASK


# --- against the global fit ------------------------------------------------------------------------------------------------
def test_the_conditional_minimum_is_not_below_the_global_one():
    seen = 0
    for C, K, v, s, T, B, data, prior, a_hat in _cases():
        if a_hat == 0.0:
            continue
        m, w = detector._prior(K, prior)
        tg, ng, mg, sg = run_fit(s, T, B, data, prior)
        bg = _nll_bound(mg, data, tg, m, w)
        for f in (0.0, 0.5, 1.0, 2.0):
            th, nll, mu, st = run_fixed(s, T, B, data, prior, f * a_hat)
            if st & FIT_INFINITE:
                assert nll == math.inf
                continue
            bc = _nll_bound(mu, data, th, m, w)
            assert nll >= ng - (bc + bg), (C, K, v, f, nll - ng, bc + bg)
            if f == 1.0:
                assert abs(nll - ng) <= bc + bg, (C, K, v, nll - ng, bc + bg)
            seen += 1
    assert seen >= 400


# --- shapes, flags, refusals ------------------------------------------------------------------------------------------------
def test_shapes_and_squeezing():
    rng = np.random.default_rng(5)
    C, K, M, ntab, Q = 5, 2, 4, 3, 6
    R, S = rng.random((ntab, M, C)) + 0.1, rng.random((Q, M))
    T, B = rng.random((K, C)) + 0.1, rng.random(C)
    data = rng.poisson(20.0, C).astype(np.float64)
    a = np.linspace(0.0, 5.0, Q)
    th, nll, mu, st = detector.fit_fixed_host(R, S, a, data, T, background=B)
    assert th.shape == (ntab, Q, 1 + K) and nll.shape == (ntab, Q) and mu.shape == (ntab, Q, C) and st.shape == (ntab, Q)
    assert st.dtype == np.int32 and np.array_equal(th[..., 0], np.broadcast_to(a, (ntab, Q)))
    one = detector.fit_fixed_host(R[1], S[2], a[2], data, T, background=B)
    assert one[0].shape == (1 + K,) and one[1].shape == () and one[2].shape == (C,) and one[3].shape == ()
    for x, y in zip(one, (th, nll, mu, st)):
        assert np.array_equal(x, y[1, 2])
    row = detector.fit_fixed_host(R, S[2], 2.0, data, T, background=B)          # a number serves every spectrum
    assert row[0].shape == (ntab, 1 + K) and np.all(row[0][:, 0] == 2.0)
    # a = 0 is the background-only fit: the signal does not enter
    z = detector.fit_fixed_host(R, S, 0.0, data, T, background=B)
    z2 = detector.fit_fixed_host(R, 7.0 * S, 0.0, data, T, background=B)
    assert np.array_equal(z[0], z2[0]) and np.array_equal(z[2], z2[2]) and np.array_equal(z[3], z2[3])


def test_flags_at_the_edges():
    C, K = 4, 2
    s = np.array([3.0, 2.0, 1.0, 0.5])
    T = np.array([[1.0, 1.0, 1.0, 0.0], [2.0, 1.0, 0.5, 0.0]])                  # the last bin: the signal's alone
    B = np.zeros(C)
    data = np.array([40.0, 25.0, 12.0, 3.0])
    th, nll, mu, st = run_fixed(s, T, B, data, None, 2.0)                       # held signal supports the bin
    assert not st & (FIT_INFINITE | FIT_NOT_CONVERGED | FIT_SINGULAR) and math.isfinite(nll) and mu[3] == 1.0
    th0, nll0, mu0, st0 = run_fixed(s, T, B, data, None, 0.0)                   # ... at a = 0 nothing does: +inf
    assert st0 & FIT_INFINITE and nll0 == math.inf and mu0[3] == 0.0 and not st0 & (FIT_NOT_CONVERGED | FIT_SINGULAR)
    assert np.all(th0[1:] >= 0) and th0[1:].sum() > 0                           # the templates are fitted all the same
    # data of zeros, no priors: every template ends at zero without a step
    thz, nllz, muz, stz = run_fixed(s, T, B, np.zeros(C), None, 2.0)
    assert stz == (FIT_ZERO << 1 | FIT_ZERO << 2) and np.all(thz[1:] == 0.0) and np.array_equal(muz, 2.0 * s)
    # a spectrum of zeros: any held scale gives the background-only fit
    e = run_fixed(np.zeros(C), T[:, :], B + 0.5, data, None, 5.0)
    e0 = run_fixed(s, T, B + 0.5, data, None, 0.0)
    assert np.array_equal(e[0][1:], e0[0][1:]) and e[3] == e0[3] and np.array_equal(e[2], e0[2])
    # a signal far above the data: the templates are pushed to zero, with their bits
    big = run_fixed(s, T, B, data, None, 1e3)
    assert big[3] & (FIT_ZERO << 1) and big[3] & (FIT_ZERO << 2) and not big[3] & (FIT_NOT_CONVERGED | FIT_SINGULAR)
    # identical templates without priors are not determined
    sing = run_fixed(s, np.array([T[0], T[0]]), B, data, None, 1.0)
    assert sing[3] & FIT_SINGULAR


def test_refusals_of_the_host_form():
    C, K = 3, 1
    R, S, data, T = np.ones((2, C)), np.array([0.0, 1.0]), np.ones(C), np.ones((K, C))
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            detector.fit_fixed_host(R, S, bad, data, T)
        db = data.copy()
        db[1] = bad
        with pytest.raises(ValueError):
            detector.fit_fixed_host(R, S, 1.0, db, T)
    with pytest.raises(ValueError):
        detector.fit_fixed_host(R, S, 1.0, data, np.zeros((K, C)))
    with pytest.raises(ValueError):
        detector.fit_fixed_host(R, S, 1.0, data, np.ones((4, C)))
    with pytest.raises(ValueError):
        detector.fit_fixed_host(R, S, np.ones(2), data, T)                      # one spectrum, two scales
