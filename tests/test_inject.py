"""The host form of the calibration call (CPU, numpy only): detector.inject_host -- per table the toys of draw_host around
the injected expectation, per toy the existing host forms (fit_host / profile_host, fit_fixed_host, limit_host's lambda),
then order_stat, the tally and the exceedance count -- against an explicit loop of those forms, and the new symbols of
the built library.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from nusiprop_amd.detector import FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_NOT_CONVERGED, FIT_SINGULAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, C, NTAB, Q, P = 6, 5, 2, 4, 5
SEED = 0x5EED0123456789AB
FAIL = FIT_NOT_CONVERGED | FIT_SINGULAR


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _case(seed=1):
    rng = np.random.default_rng(seed)
    R = rng.random((NTAB, M, C)) * 10.0 ** rng.uniform(-1, 1, (NTAB, 1, 1))
    S = rng.random((Q, M)) * 10.0 ** rng.uniform(-1, 1, (Q, 1))
    S[3] = 0.0                                                      # a spectrum of zeros
    B = 0.5 + rng.random(C)
    T = np.stack([(1.0 + j) * np.exp(-(0.5 + 0.4 * j) * np.linspace(0.0, 3.0, C)) for j in range(3)]) * 5.0
    return R, S, B, T


def _loop(R, S, a_inj, a_test, th_inj, mode, T, prior, B):
    """The definition, written out: the toys of Plan.draw's host form, then the existing host forms per toy."""
    K = 0 if T is None else len(T)
    m, w = detector._prior(K, prior)
    s = detector.events_host(R, S)
    th_all, st_all = np.zeros((NTAB, Q, P)), np.zeros((NTAB, Q, P))
    words, data = np.zeros((NTAB, Q, P, 2), dtype=np.int32), np.zeros((NTAB, Q, P, C))
    for t in range(NTAB):
        mu = a_inj[:, None] * s[t]
        for j in range(K):
            mu = mu + th_inj[j] * T[j]
        mu = mu + B
        data[t] = detector.draw_host(mu, P, SEED, stream=t)
        for q in range(Q):
            for p in range(P):
                d = data[t, q, p]
                if K:
                    thh, _, muh, sth = detector.fit_host(R[t], S[q], d, T, prior=prior, background=B)
                    thc, _, muc, stc = detector.fit_fixed_host(R[t], S[q], a_test[q], d, T, prior=prior, background=B)
                    assert thc[0] == a_test[q]
                else:
                    ah, _, muh, sth = detector.profile_host(R[t], S[q], d, background=B)
                    thh, thc, stc = np.array([ah]), np.array([a_test[q]]), 0
                    muc = detector.events_host(R[t], S[q], scale=a_test[q], background=B)
                with np.errstate(all="ignore"):
                    lam, _ = detector._limit_lambda(a_test[q], thc[1:], muc, muh, thh[1:], (d > 0) & (muh > 0), d, m[1:], w[1:],
                                                    np.log)
                stat = 2.0 * lam if lam > 0 else 0.0
                if (mode == "upper" and thh[0] > a_test[q]) or (mode == "discovery" and thh[0] < a_test[q]):
                    stat = 0.0
                th0 = thh[0]
                if sth & FAIL:
                    th0 = stat = np.nan
                if stc & FAIL:
                    stat = np.nan
                th_all[t, q, p], st_all[t, q, p], words[t, q, p] = th0, stat, (sth, stc)
    return th_all, st_all, words, data


@pytest.mark.parametrize("given", (False, True))
@pytest.mark.parametrize("mode", ("two-sided", "upper", "discovery"))
@pytest.mark.parametrize("K", (0, 1, 3))
def test_host_form_equals_the_loop(K, mode, given):
    R, S, B, T = _case()
    Tk = T[:K] if K else None
    prior = (np.full(K, 1.0), np.full(K, 0.5)) if K else None
    a_inj = np.array([0.0, 2.0, 0.7, 1.0])                          # a_inj = 0: background-only toys
    a_test = np.array([0.5, 0.0, 0.7, 3.0]) if given else None      # a_test = 0 under an injected signal
    th_inj = np.array([1.0, 0.8, 1.3])[:K]
    ranks = [0, 2, 4, 2]
    q_obs = np.array([[0.0, 1.0, 2.706, 0.5], [np.nan, np.inf, 0.3, 0.0]])
    out = detector.inject_host(R, S, a_inj, P, SEED, theta_inj=th_inj, a_test=a_test, mode=mode, ranks=ranks, q_obs=q_obs,
                               templates=Tk, prior=prior, background=B, raw=True)
    bth, bst, tally, exceed, th_all, st_all, words, data = out
    assert bth.shape == bst.shape == (NTAB, Q, 4) and tally.shape == (NTAB, Q, 4) and exceed.shape == (NTAB, Q)
    assert tally.dtype == exceed.dtype == words.dtype == np.int32 and data.shape == (NTAB, Q, P, C)
    wth, wst, wwords, wdata = _loop(R, S, a_inj, a_inj if a_test is None else a_test, th_inj, mode, Tk, prior, B)
    assert np.array_equal(data, wdata) and np.array_equal(words, wwords)
    assert np.array_equal(_bits(th_all), _bits(wth)) and np.array_equal(_bits(st_all), _bits(wst))
    # the bands against order_stat, the tally and exceed against the raw values
    assert np.array_equal(_bits(bth), _bits(detector.order_stat(th_all, ranks)))
    assert np.array_equal(_bits(bst), _bits(detector.order_stat(st_all, ranks)))
    nofit, nocond = (words[..., 0] & FAIL) != 0, (words[..., 1] & FAIL) != 0
    assert np.array_equal(tally[..., 0], nofit.sum(-1)) and np.array_equal(tally[..., 1], (nocond & ~nofit).sum(-1))
    assert np.array_equal(tally[..., 2], ((words[..., 0] & (FIT_BOUNDARY | FIT_FLAT)) != 0).sum(-1))
    assert np.array_equal(tally[..., 3], ((words[..., 0] & FIT_INFINITE) != 0).sum(-1))
    assert np.array_equal(np.isnan(st_all), nofit | nocond) and np.array_equal(np.isnan(th_all), nofit)
    assert np.array_equal(np.isnan(st_all).sum(-1), tally[..., 0] + tally[..., 1])      # the p-value's denominator
    with np.errstate(invalid="ignore"):
        assert np.array_equal(exceed, (st_all >= q_obs[..., None]).sum(-1))
    assert not exceed[1, 0] and np.all(exceed[0, 0] + np.isnan(st_all[0, 0]).sum() == P)   # NaN never counts; stat >= 0 always
    # what the rules give: non-negative, never -0.0; the spectrum of zeros is FLAT with theta_hat_0 = 0
    fin = ~np.isnan(st_all)
    assert np.all(st_all[fin] >= 0) and not np.signbit(st_all[fin]).any() and not np.signbit(th_all[~np.isnan(th_all)]).any()
    assert np.all(words[:, 3, :, 0] & FIT_FLAT) and np.all(tally[:, 3, 2] == P) and not np.nansum(th_all[:, 3])
    if K == 0:
        assert not words[..., 1].any()
    if a_test is None:
        # the spectrum of zeros tested at its own hypothesis: the fits coincide, lambda is 0 up to rounding
        assert np.all(st_all[:, 3][~np.isnan(st_all[:, 3])] < 1e-9)
    if mode == "upper":
        assert np.all(st_all[fin & (th_all > np.broadcast_to((a_inj if a_test is None else a_test)[None, :, None], th_all.shape))] == 0)
    # without raw and q_obs: the first three; ranks = None: band_ranks(P)
    three = detector.inject_host(R, S, a_inj, P, SEED, theta_inj=th_inj, a_test=a_test, mode=mode, templates=Tk, prior=prior,
                                 background=B)
    assert len(three) == 3 and three[0].shape == (NTAB, Q, 5)
    assert np.array_equal(_bits(three[1]), _bits(detector.order_stat(st_all, detector.band_ranks(P))))
    assert np.array_equal(three[2], tally)


def test_injected_signal_moves_the_statistic():
    """Discovery power in one line: at a_test = 0 the statistic of toys with an injected signal lies above that of
    background-only toys, and the best fit follows the injection."""
    R, S, B, T = _case(seed=3)
    a = np.array([0.0, 0.0, 6.0, 6.0])
    S[3] = S[2]
    S[1] = S[2]
    _, bst, _, th_all, st_all, _, _ = detector.inject_host(R, S, a, 9, SEED, a_test=0.0, mode="discovery", ranks=[4],
                                                            background=B, raw=True)
    assert np.all(bst[:, 2, 0] > bst[:, 1, 0]) and np.all(np.median(th_all[:, 2], axis=-1) > np.median(th_all[:, 1], axis=-1))
    # rows 2 and 3 are the same hypothesis but other toys (the row enters the draw's identity)
    assert not np.array_equal(st_all[:, 2], st_all[:, 3])


def test_a_singular_class_is_nan_and_counted():
    """Two identical templates without priors: the best fit's system is singular where a solve is needed."""
    R, S, B, T = _case(seed=5)
    T2 = np.stack([T[0], T[0]])
    bth, bst, tally, th_all, st_all, words, data = detector.inject_host(R, S, 1.0, P, SEED, theta_inj=[1.0, 1.0], ranks=[0, P - 1],
                                                                        templates=T2, background=B, raw=True)
    nofit = (words[..., 0] & FAIL) != 0
    assert nofit.any() and np.array_equal(np.isnan(th_all), nofit) and np.array_equal(tally[..., 0], nofit.sum(-1))
    assert np.all(np.isnan(st_all[nofit]))
    assert np.array_equal(np.isnan(bth[..., 1]), nofit.any(-1))     # NaN sorts last: the top rank is NaN where any toy failed
    assert np.array_equal(np.isnan(bth[..., 0]), nofit.all(-1))


def test_theta_inj_defaults_to_the_prior_means_and_one_toy():
    R, S, B, T = _case(seed=2)
    prior = (np.array([1.5, 0.7]), np.array([0.3, np.inf]))         # the second template has no prior: its mean counts as 0
    a = detector.inject_host(R[0], S[1], 1.0, 1, 7, templates=T[:2], prior=prior, background=B, raw=True)
    b = detector.inject_host(R[0], S[1], 1.0, 1, 7, theta_inj=[1.5, 0.0], templates=T[:2], prior=prior, background=B, raw=True)
    assert a[0].shape == (1, 1, 5) and a[3].shape == (1, 1, 1) and a[6].shape == (1, 1, 1, C)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.all(a[0] == a[3][..., 0, None]) or np.all(np.isnan(a[0]))          # P = 1: every rank is the one toy


def test_host_form_refusals():
    R, S, B, T = _case(seed=4)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            detector.inject_host(R, S, bad, P, 1, background=B)
        with pytest.raises(ValueError):
            detector.inject_host(R, S, 1.0, P, 1, a_test=bad, background=B)
        with pytest.raises(ValueError):
            detector.inject_host(R, S, 1.0, P, 1, theta_inj=[bad], templates=T[:1], background=B)
    with pytest.raises(ValueError):
        detector.inject_host(R, S, 1.0, 0, 1, background=B)
    with pytest.raises(ValueError):
        detector.inject_host(R, S[:, :-1], 1.0, P, 1, background=B)
    with pytest.raises(ValueError):
        detector.inject_host(R, S, 1.0, P, 1, mode="sideways", background=B)
    for bad in ([P], [-1]):
        with pytest.raises(ValueError):
            detector.inject_host(R, S, 1.0, P, 1, ranks=bad, background=B)
    with pytest.raises(ValueError):
        detector.inject_host(R, S, 1.0, P, 2 ** 64, background=B)


def test_abi():
    """The header's constants are the package's; the new calls are declared, bound and exported; without a plan they
    refuse."""
    text = open(os.path.join(ROOT, "include", "nusi.h")).read()
    macro = {k: int(v, 0) for k, v in re.findall(r"^#define (NUSI_[A-Z_]+) (\d+)$", text, flags=re.M)}
    assert (macro["NUSI_INJECT_TWO_SIDED"], macro["NUSI_INJECT_UPPER"], macro["NUSI_INJECT_DISCOVERY"]) == (
        _lib.INJECT_TWO_SIDED, _lib.INJECT_UPPER, _lib.INJECT_DISCOVERY) == (
        detector.INJECT_TWO_SIDED, detector.INJECT_UPPER, detector.INJECT_DISCOVERY) == (0, 1, 2)
    assert macro["NUSI_DRAW_DATASETS_MAX"] == _lib.DRAW_DATASETS_MAX
    L = _lib.load()
    for name in ("nusi_plan_response_inject", "nusi_plan_response_inject_host", "nusi_plan_draw_counts",
                 "nusi_plan_draw_counts_host"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name).argtypes is not None
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    one, r = np.ones(4), np.zeros(1, dtype=np.int32)
    p, rp = one.ctypes.data_as(dp), r.ctypes.data_as(ip)
    refused = (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_response_inject(None, None, 1, p, 1, p, None, None, 1, 1, 0, rp, 1, None, None, None, None, None,
                                       None, None, None, None, None) in refused
    assert L.nusi_plan_response_inject_host(None, p, 1, p, 1, p, None, None, 1, 1, 0, rp, 1, None, p, p, None, None, None,
                                            None, None, None) in refused
