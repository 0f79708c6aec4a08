"""The toys' ensembles of inject_host and belt_host on the CPU (NUSI_OPT_TOY_NUISANCE: "fixed", "global", "prior").

A prior (m_j, sigma_j) on template j stands for an auxiliary measurement.  "fixed" keeps m_j in every toy; "global" redraws
it per toy around the value the toys are thrown from; "prior" (inject only) throws the nuisance itself from its prior.

The statistical point (test_global_observables_restore_the_nuisance_spread): C = 8, M = 5, one template under a prior
with w = 9 I_d, where I_d is the counts' information on theta_1 from the expected Fisher matrix (the Schur complement
over the signal), P = 400 toys.  In the linear-Gaussian picture Var(theta_hat_1) is I_d / (I_d + w)^2 with the mean
fixed and 1 / (I_d + w) with the mean drawn: a ratio of (I_d + w) / I_d = 10.  The assertion is that the measured ratio
lies within [0.6, 1.6] of that: the relative s.d. of a sample variance at P = 400 is sqrt(2 / 399) = 0.07, and the
Gaussian approximation itself is some per cent off (bounds theta >= 0, Poisson counts).
"""
import math

import numpy as np
import pytest

from nusiprop_amd import detector

SEED = 0x9E3779B97F4A7C15


def _model(C=5, M=4, K=2, Q=3, ntab=2, seed=1):
    rng = np.random.default_rng(seed)
    R = rng.uniform(0.5, 2.0, (ntab, M, C))
    S = rng.uniform(0.2, 1.0, (Q, M))
    S[-1] = 0.0                                                     # a spectrum of zeros
    T = rng.uniform(2.0, 8.0, (K, C)) if K else None
    B = rng.uniform(0.5, 1.5, C)
    return R, S, T, B


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)


def test_fixed_is_the_call_without_the_keyword():
    R, S, T, B = _model()
    prior = ([1.0, 1.2], [0.3, np.inf])
    kw = dict(theta_inj=[1.1, 0.9], templates=T, prior=prior, background=B, q_obs=1.0)
    for raw in (False, True):
        base = detector.inject_host(R, S, 2.0, 3, SEED, raw=raw, **kw)
        assert len(base) == (8 if raw else 4)
        _same(base, detector.inject_host(R, S, 2.0, 3, SEED, raw=raw, nuisance="fixed", **kw))
        _same(base, detector.inject_host(R, S, 2.0, 3, SEED, raw=raw, nuisance=detector.TOYS_FIXED, **kw))
    d = np.array([30.0, 25.0, 41.0, 28.0, 33.0])
    bkw = dict(templates=T, prior=prior, background=B)
    for raw in (False, True):
        base = detector.belt_host(R[0], S[:2], d, [0.0, 1.0, 3.0], 3, SEED, raw=raw, **bkw)
        assert len(base) == (13 if raw else 9)
        _same(base, detector.belt_host(R[0], S[:2], d, [0.0, 1.0, 3.0], 3, SEED, raw=raw, nuisance="fixed", **bkw))


def test_the_names_and_refusals():
    R, S, T, B = _model()
    kw = dict(templates=T, prior=([1.0, 1.2], [0.3, 0.4]), background=B)
    for bad in ("Global", "none", 3, -1, None, True):
        with pytest.raises(ValueError):
            detector.inject_host(R, S, 2.0, 2, SEED, nuisance=bad, **kw)
    d = np.full(5, 30.0)
    for bad in ("prior", detector.TOYS_PRIOR, "none", 3):
        with pytest.raises(ValueError):
            detector.belt_host(R[0], S[:1], d, [1.0], 2, SEED, nuisance=bad, **kw)
    a = detector.inject_host(R[0], S[:1], 2.0, 2, SEED, nuisance="global", raw=True, **kw)
    _same(a, detector.inject_host(R[0], S[:1], 2.0, 2, SEED, nuisance=detector.TOYS_GLOBAL, raw=True, **kw))
    a = detector.inject_host(R[0], S[:1], 2.0, 2, SEED, nuisance="prior", raw=True, **kw)
    _same(a, detector.inject_host(R[0], S[:1], 2.0, 2, SEED, nuisance=detector.TOYS_PRIOR, raw=True, **kw))


def test_nothing_constrained_gives_fixed():
    """With every sigma = inf, with no prior, and with K = 0 the three ensembles are one."""
    R, S, T, B = _model()
    d = np.array([30.0, 25.0, 41.0, 28.0, 33.0])
    for templates, prior in ((T, ([1.0, 1.2], [np.inf, np.inf])), (T, None), (None, None)):
        kw = dict(templates=templates, prior=prior, background=B)
        K = 0 if templates is None else len(templates)
        ti = [1.1, 0.9][:K] if K else None
        base = detector.inject_host(R, S, 2.0, 3, SEED, theta_inj=ti, raw=True, **kw)
        for ens in ("global", "prior"):
            got = detector.inject_host(R, S, 2.0, 3, SEED, theta_inj=ti, raw=True, nuisance=ens, **kw)
            _same(base, got[:-1])
            assert got[-1].shape == (2, 3, 3, K)
            if K:                                                   # the centre itself: theta_inj
                assert np.array_equal(got[-1], np.broadcast_to(np.array(ti), got[-1].shape))
        base = detector.belt_host(R, S, d, [0.0, 1.0, 3.0], 3, SEED, raw=True, **kw)
        got = detector.belt_host(R, S, d, [0.0, 1.0, 3.0], 3, SEED, raw=True, nuisance="global", **kw)
        _same(base, got[:-1])
        assert got[-1].shape == (2, 3, 3, 3, K)


def test_global_is_a_hand_loop_of_the_fits():
    """GLOBAL: the counts are FIXED's; nuis_all is draw_normal_host around theta_inj; a toy's record is fit_host /
    fit_fixed_host with prior = (nuis_all[t, q, p], sigma)."""
    R, S, T, B = _model()
    prior, ti, P = ([1.0, 1.2], [0.3, np.inf]), np.array([1.1, 0.9]), 4
    kw = dict(theta_inj=ti, a_test=1.5, templates=T, prior=prior, background=B, raw=True)
    fix = detector.inject_host(R, S, 2.0, P, SEED, **kw)
    glo = detector.inject_host(R, S, 2.0, P, SEED, nuisance="global", **kw)
    assert len(glo) == len(fix) + 1
    th_all, st_all, words, data, nuis = glo[3:]
    assert np.array_equal(data, fix[6])                             # every integer
    assert not np.array_equal(th_all, fix[3])                       # ... and other fits
    ntab, Q = R.shape[0], len(S)
    for t in range(ntab):
        want = detector.draw_normal_host(np.broadcast_to(ti, (Q, 2)), prior[1], P, SEED, stream=t)
        assert np.array_equal(nuis[t], want)
    assert np.all(nuis[..., 1] == ti[1]) and np.all(nuis[..., 0] >= 0) and len(np.unique(nuis[..., 0])) == ntab * Q * P
    m, w = detector._prior(2, prior)
    for t in range(ntab):
        for q in range(Q):
            for p in range(P):
                pr = (nuis[t, q, p], prior[1])
                thh, _, muh, sth = detector.fit_host(R[t], S[q], data[t, q, p], T, prior=pr, background=B)
                thc, _, muc, stc = detector.fit_fixed_host(R[t], S[q], 1.5, data[t, q, p], T, prior=pr, background=B)
                assert tuple(words[t, q, p]) == (sth, stc)
                assert th_all[t, q, p] == thh[0]
                mp = detector._prior(2, pr)[0]
                d = data[t, q, p]
                with np.errstate(all="ignore"):
                    lam, _ = detector._limit_lambda(1.5, thc[1:], muc, muh, thh[1:], (d > 0) & (muh > 0), d, mp[1:], w[1:], np.log)
                assert st_all[t, q, p] == (2.0 * lam if lam > 0 else 0.0)
    # the bands and the tally follow the raw arrays
    assert np.array_equal(glo[0], detector.order_stat(th_all, detector.band_ranks(P)), equal_nan=True)
    assert np.array_equal(glo[2], detector.inject_tally(words))


def test_prior_draws_the_counts_from_the_thrown_nuisances():
    R, S, T, B = _model()
    prior, ti, P = ([1.0, 1.2], [0.3, np.inf]), np.array([1.1, 0.9]), 4
    kw = dict(theta_inj=ti, templates=T, prior=prior, background=B, raw=True)
    fix = detector.inject_host(R, S, 2.0, P, SEED, **kw)
    pri = detector.inject_host(R, S, 2.0, P, SEED, nuisance="prior", **kw)
    th_all, st_all, words, data, nuis = pri[3:]
    ntab, Q, C = R.shape[0], len(S), R.shape[2]
    s = np.reshape(detector.events_host(R, S), (ntab, Q, C))
    for t in range(ntab):
        # the constrained template is thrown around its prior mean, the other one is theta_inj's
        want = detector.draw_normal_host(np.broadcast_to(np.array([1.0, ti[1]]), (Q, 2)), prior[1], P, SEED, stream=t)
        assert np.array_equal(nuis[t], want)
        for p in range(P):
            mu = 2.0 * s[t]
            for j in range(2):
                mu = mu + nuis[t, :, p, j][:, None] * T[j][None, :]
            mu = mu + B[None, :]
            assert np.array_equal(data[t, :, p], detector.draw_host(mu, P, SEED, stream=t)[:, p])
    assert not np.array_equal(data, fix[6])
    # the fits use the plan's means
    for t, q, p in ((0, 0, 0), (1, 2, 3), (1, 1, 2)):
        thh, _, _, sth = detector.fit_host(R[t], S[q], data[t, q, p], T, prior=prior, background=B)
        _, _, _, stc = detector.fit_fixed_host(R[t], S[q], 2.0, data[t, q, p], T, prior=prior, background=B)
        assert th_all[t, q, p] == thh[0] and tuple(words[t, q, p]) == (sth, stc)


def test_belt_global_is_a_hand_loop_of_the_fits():
    R, S, T, B = _model()
    prior, P, frac = ([1.0, 1.2], [0.3, np.inf]), 3, np.array([0.0, 1.0, 3.0])
    d = np.array([30.0, 25.0, 41.0, 28.0, 33.0])
    kw = dict(templates=T, prior=prior, background=B, raw=True)
    fix = detector.belt_host(R, S, d, frac, P, SEED, ref=[[1.0, 2.0, np.nan]] * 2, **kw)
    glo = detector.belt_host(R, S, d, frac, P, SEED, ref=[[1.0, 2.0, np.nan]] * 2, nuisance="global", **kw)
    assert len(glo) == len(fix) + 1
    for k in (6, 7, 8, 12):                                          # the observed side and the counts drawn: FIXED's
        assert np.array_equal(glo[k], fix[k], equal_nan=True), k
    q_obs, theta_obs = glo[6], glo[7]
    th_all, st_all, words, data, nuis = glo[9:]
    ntab, Q, G = R.shape[0], len(S), len(frac)
    valid = ~np.isnan(q_obs)
    assert valid[:, :2].all() and not valid[:, 2].any() and not nuis[:, 2].any()
    for t in range(ntab):
        centre = np.where(valid[t][..., None], theta_obs[t, :, 1:, 1:], 0.0).reshape(Q * G, 2)
        want = detector.draw_normal_host(centre, prior[1], P, SEED, stream=t).reshape(Q, G, P, 2)
        assert np.array_equal(nuis[t][valid[t]], want[valid[t]])
        for q, g in zip(*np.nonzero(valid[t])):
            a = frac[g] * (1.0, 2.0)[q]
            assert np.all(nuis[t, q, g, :, 1] == theta_obs[t, q, 1 + g, 2])
            for p in range(P):
                pr = (nuis[t, q, g, p], prior[1])
                thh, _, _, sth = detector.fit_host(R[t], S[q], data[t, q, g, p], T, prior=pr, background=B)
                _, _, _, stc = detector.fit_fixed_host(R[t], S[q], a, data[t, q, g, p], T, prior=pr, background=B)
                assert th_all[t, q, g, p] == thh[0] and tuple(words[t, q, g, p]) == (sth, stc)
    assert not np.array_equal(st_all, fix[10], equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(glo[4], (st_all >= q_obs[..., None]).sum(-1).astype(np.int32))


def test_global_observables_restore_the_nuisance_spread():
    C, M, P = 8, 5, 400
    rng = np.random.default_rng(11)
    R = rng.uniform(0.5, 2.0, (M, C))
    S = rng.uniform(0.2, 1.0, M)
    T = rng.uniform(20.0, 60.0, (1, C))
    a_inj, th_inj = 20.0, 1.0
    s = np.reshape(detector.events_host(R, S), C)
    mu = a_inj * s + th_inj * T[0]
    # the expected Fisher matrix of (a, theta_1) from the counts, and the counts' information on theta_1 with a profiled
    F = np.array([[np.sum(s * s / mu), np.sum(s * T[0] / mu)], [np.sum(s * T[0] / mu), np.sum(T[0] * T[0] / mu)]])
    I_d = F[1, 1] - F[0, 1] ** 2 / F[0, 0]
    w = 9.0 * I_d
    sigma = 1.0 / math.sqrt(w)
    prior = ([th_inj], [sigma])

    def var(ens):
        data = detector.inject_host(R, S, a_inj, P, SEED, theta_inj=[th_inj], templates=T, prior=prior, raw=True, nuisance=ens)
        toys = data[6][0, 0]
        nuis = data[7][0, 0, :, 0] if ens != "fixed" else np.full(P, th_inj)
        th1 = np.array([detector.fit_host(R, S, toys[p], T, prior=([nuis[p]], [sigma]))[0].reshape(-1)[1] for p in range(P)])
        return th1.var(ddof=1)

    v_fix, v_glo = var("fixed"), var("global")
    want = (I_d + w) / I_d
    print("Var(theta_hat_1): fixed %.3e (linear-Gaussian %.3e), global %.3e (%.3e); ratio %.3f of the predicted %.1f: %.3f" % (
        v_fix, I_d / (I_d + w) ** 2, v_glo, 1.0 / (I_d + w), v_glo / v_fix, want, v_glo / v_fix / want))
    assert 0.6 <= (v_glo / v_fix) / want <= 1.6
