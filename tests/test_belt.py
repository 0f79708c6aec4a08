"""The host form of the calibrated interval (CPU, numpy only): detector.belt_host -- per (table, spectrum, grid point) the
data's fits by the existing host forms, the toys of draw_host around the data's conditional fit, inject_host's loop body
per toy, the exceedance count and detector.belt_accept -- against an explicit loop of those forms, the acceptance rule on
hand-made counts, the statistic against an exact enumeration, the flags and the refusals.
"""
import math

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (BELT_BAD_POINT, BELT_EMPTY, BELT_GAPS, BELT_HI_EDGE, BELT_LO_EDGE, BELT_NO_FIT,
                                   BELT_NO_GRID, FIT_NOT_CONVERGED, FIT_SINGULAR)

M, NTAB, Q, G, P = 6, 2, 3, 3, 5
SEED = 0x5EED0123456789AB
FAIL = FIT_NOT_CONVERGED | FIT_SINGULAR


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _case(C, seed=1):
    rng = np.random.default_rng(seed)
    R = rng.random((NTAB, M, C)) * 10.0 ** rng.uniform(-1, 1, (NTAB, 1, 1))
    S = rng.random((Q, M)) * 10.0 ** rng.uniform(-1, 1, (Q, 1))
    S[2] = 0.0                                                      # a spectrum of zeros
    B = 0.5 + rng.random(C)
    T = np.stack([(1.0 + j) * np.exp(-(0.5 + 0.4 * j) * np.linspace(0.0, 3.0, C)) for j in range(3)]) * 5.0
    data = rng.poisson(3.0 + 4.0 * rng.random(C)).astype(np.float64)
    return R, S, B, T, data


def _observed(Rt, Sq, a, d, T, prior, B, mode):
    """The data's records at the scale a, from the existing host forms: (theta_hat, its word, the conditional fit's
    theta with a in front, its word, q_obs)."""
    K = 0 if T is None else len(T)
    m, w = detector._prior(K, prior)
    if K:
        thh, _, muh, sth = detector.fit_host(Rt, Sq, d, T, prior=prior, background=B)
        thc, _, muc, stc = detector.fit_fixed_host(Rt, Sq, a, d, T, prior=prior, background=B)
        assert thc[0] == a
    else:
        ah, _, muh, sth = detector.profile_host(Rt, Sq, d, background=B)
        thh, thc, stc = np.array([float(ah)]), np.array([a]), 0
        muc = detector.events_host(Rt, Sq, scale=a, background=B)
    with np.errstate(all="ignore"):
        lam, _ = detector._limit_lambda(a, thc[1:], muc, muh, thh[1:], (d > 0) & (muh > 0), d, m[1:], w[1:], np.log)
    q = 2.0 * lam if lam > 0 else 0.0
    if mode == "upper" and thh[0] > a:
        q = 0.0
    if (int(sth) | int(stc)) & FAIL:
        q = np.nan
    return thh, int(sth), thc, int(stc), q


@pytest.mark.parametrize("C", (1, 5))
@pytest.mark.parametrize("mode", ("two-sided", "upper"))
@pytest.mark.parametrize("K", (0, 1, 3))
def test_host_form_equals_the_loop(K, mode, C):
    R, S, B, T, data = _case(C)
    Tk = T[:K] if K else None
    prior = (np.full(K, 1.0), np.full(K, 0.5)) if K else None
    frac = np.array([0.0, 0.6, 1.7])
    ref = np.array([[1.0, 2.5, 1.0], [0.3, 4.0, 2.0]])
    out = detector.belt_host(R, S, data, frac, P, SEED, ref=ref, mode=mode, alpha=0.3, templates=Tk, prior=prior,
                             background=B, raw=True)
    lo, hi, idx, status, exceed, tally, q_obs, theta_obs, words_obs, th_all, st_all, words, toys = out
    assert lo.shape == hi.shape == status.shape == (NTAB, Q) and idx.shape == (NTAB, Q, 2)
    assert exceed.shape == q_obs.shape == (NTAB, Q, G) and tally.shape == (NTAB, Q, G, 4)
    assert theta_obs.shape == (NTAB, Q, 1 + G, 1 + K) and words_obs.shape == (NTAB, Q, 1 + G)
    assert th_all.shape == st_all.shape == (NTAB, Q, G, P) and words.shape == (NTAB, Q, G, P, 2)
    assert toys.shape == (NTAB, Q, G, P, C)
    assert idx.dtype == status.dtype == exceed.dtype == tally.dtype == words_obs.dtype == words.dtype == np.int32
    a = frac[None, None, :] * ref[:, :, None]
    Srep = np.repeat(S, G, axis=0)                                  # row q G + g
    for t in range(NTAB):
        for q in range(Q):
            for g in range(G):
                thh, sth, thc, stc, qo = _observed(R[t], S[q], a[t, q, g], data, Tk, prior, B, mode)
                assert np.array_equal(_bits(theta_obs[t, q, 0]), _bits(thh)) and words_obs[t, q, 0] == sth
                assert np.array_equal(_bits(theta_obs[t, q, 1 + g]), _bits(thc)) and words_obs[t, q, 1 + g] == stc
                assert not (sth | stc) & FAIL                       # (this case: every observed fit holds)
                assert _bits(q_obs[t, q, g]) == _bits(qo)
                # the record's toys: inject on the repeated list with the record's a and conditional theta
                w = detector.inject_host(R[:t + 1], Srep, a[t].reshape(-1), P, SEED,
                                         theta_inj=thc[1:], mode=mode, ranks=[0], q_obs=qo, templates=Tk, prior=prior,
                                         background=B, raw=True)
                _, _, wtally, wexceed, wth, wst, wwords, wdata = w
                r = q * G + g
                assert np.array_equal(toys[t, q, g], wdata[t, r]) and np.array_equal(words[t, q, g], wwords[t, r])
                assert np.array_equal(_bits(th_all[t, q, g]), _bits(wth[t, r]))
                assert np.array_equal(_bits(st_all[t, q, g]), _bits(wst[t, r]))
                assert np.array_equal(tally[t, q, g], wtally[t, r]) and exceed[t, q, g] == wexceed[t, r]
    # the interval is belt_accept of the counts; without raw: the first nine
    want = detector.belt_accept(exceed, tally, a, 0.3, np.ones((NTAB, Q, G), dtype=bool), P)
    for x, y in zip((lo, hi, idx, status), want):
        assert np.array_equal(x, y, equal_nan=True)
    nine = detector.belt_host(R, S, data, frac, P, SEED, ref=ref, mode=mode, alpha=0.3, templates=Tk, prior=prior, background=B)
    assert len(nine) == 9
    for x, y in zip(nine, out):
        assert np.array_equal(x, y, equal_nan=True)
    # frac[0] = 0 is the background-only point; the statistic is never negative, never -0.0
    assert np.all(q_obs >= 0) and not np.signbit(q_obs).any()


def test_accept_on_hand_made_counts():
    P_, alpha = 20, 0.25                                            # alpha nv = 5 exactly at nv = 20
    a = np.arange(1.0, 6.0)                                         # G = 5
    z = np.zeros((5, 4), dtype=np.int32)
    ok = np.ones(5, dtype=bool)

    def run(ex, ty=z, valid=ok, flags=0):
        lo, hi, idx, st = detector.belt_accept(np.array(ex, dtype=np.int32), ty, a, alpha, valid, P_, flags)
        return float(lo), float(hi), tuple(int(i) for i in idx), int(st)

    # empty; the strict inequality: exceed == alpha nv does not accept, one more does
    lo, hi, idx, st = run([0, 5, 5, 1, 0])
    assert np.isnan(lo) and np.isnan(hi) and idx == (-1, -1) and st == BELT_EMPTY
    assert run([0, 5, 6, 5, 0]) == (3.0, 3.0, (2, 2), 0)
    # both edges; a gap
    assert run([6, 6, 6, 6, 6]) == (1.0, 5.0, (0, 4), BELT_LO_EDGE | BELT_HI_EDGE)
    assert run([6, 0, 0, 0, 0]) == (1.0, 1.0, (0, 0), BELT_LO_EDGE)
    assert run([0, 0, 0, 0, 6]) == (5.0, 5.0, (4, 4), BELT_HI_EDGE)
    assert run([0, 6, 2, 6, 0]) == (2.0, 4.0, (1, 3), BELT_GAPS)
    # an invalid point in the middle is not accepted whatever its count; the caller's flag is kept
    v = ok.copy()
    v[2] = False
    assert run([0, 6, 20, 6, 0], valid=v, flags=BELT_BAD_POINT) == (2.0, 4.0, (1, 3), BELT_GAPS | BELT_BAD_POINT)
    # nv = 0: no toy has a statistic -- BAD_POINT, not accepted; nv = 4 of 20: the bar is alpha nv = 1
    ty = z.copy()
    ty[1] = (12, 8, 0, 0)
    ty[3] = (10, 6, 3, 1)
    assert run([0, 0, 6, 1, 0], ty=ty) == (3.0, 3.0, (2, 2), BELT_BAD_POINT)
    assert run([0, 0, 6, 2, 0], ty=ty) == (3.0, 4.0, (2, 3), BELT_BAD_POINT)
    # leading axes, and shapes that do not match
    lo, hi, idx, st = detector.belt_accept(np.full((2, 3, 5), 6), np.zeros((2, 3, 5, 4), dtype=np.int32),
                                           np.broadcast_to(a, (2, 3, 5)), alpha, None, P_)
    assert lo.shape == (2, 3) and idx.shape == (2, 3, 2) and idx.dtype == st.dtype == np.int32 and np.all(hi == 5.0)
    with pytest.raises(ValueError):
        detector.belt_accept(np.zeros(5), np.zeros((5, 3)), a, alpha, None, P_)


def _one_bin():
    """C = 1, K = 0, background 3, one signal count per unit scale."""
    R = np.zeros((1, 2, 1))
    R[0, 1, 0] = 1.0
    return R, np.array([0.0, 1.0]), np.array([3.0])


def test_a_toy_equal_to_the_data_has_the_datas_statistic():
    R, S, B = _one_bin()
    *_, q_obs, _, _, th_all, st_all, words, toys = detector.belt_host(R, S, [5.0], [0.5, 2.0, 6.0], 40, SEED, background=B,
                                                                      raw=True)
    same = toys[0, 0, :, :, 0] == 5.0
    assert same.any(axis=-1).all()                                  # every grid point has such a toy
    for g in range(3):
        assert np.all(_bits(st_all[0, 0, g][same[g]]) == _bits(q_obs[0, 0, g]))


def test_the_statistic_against_the_exact_p_value():
    """exceed / P against sum_n [q_n(a) >= q_obs(a)] Pois(n; a + 3), n <= 60, the same statistic in floats; the bound is
    the binomial's: 4 sigma plus one toy."""
    R, S, B = _one_bin()
    frac, P_, n_obs = np.array([0.5, 2.0, 6.0, 9.0]), 400, 5

    def stat(n, a):
        ah = max(n - 3.0, 0.0)
        mu, muh = a + 3.0, ah + 3.0
        lam = (mu - muh) - n * math.log(mu / muh) if n > 0 else mu - muh
        return 2.0 * lam if lam > 0 else 0.0

    out = detector.belt_host(R, S, [float(n_obs)], frac, P_, 20241, background=B)
    exceed, tally, q_obs = out[4][0, 0], out[5][0, 0], out[6][0, 0]
    assert not tally[:, :2].any()
    for g, a in enumerate(frac):
        qo = stat(n_obs, a)
        assert abs(q_obs[g] - qo) <= 1e-12 * max(qo, 1.0)
        lam = a + 3.0
        pois = [math.exp(-lam + n * math.log(lam) - math.lgamma(n + 1.0)) for n in range(61)]
        assert abs(sum(pois) - 1.0) < 1e-12
        p = sum(w for n, w in enumerate(pois) if stat(n, a) >= qo)     # (n = n_obs ties with q_obs and counts)
        got = exceed[g] / P_
        print("a = %g: exact p = %.6f, toys %.6f" % (a, p, got))
        assert abs(got - p) <= 4.0 * math.sqrt(p * (1.0 - p) / P_) + 1.0 / P_, (a, p, got)


def test_flags():
    R, S, B, T, data = _case(5, seed=4)
    frac = np.array([0.0, 0.5, 1.0])
    # a ref of NaN, +inf and -1: NO_GRID, no toys, NaN / 0; the observed best fit is still returned
    ref = np.array([[np.nan, np.inf, 1.0], [-1.0, 1.0, 1.0]])
    out = detector.belt_host(R, S, data, frac, P, SEED, ref=ref, templates=T[:1], background=B, raw=True)
    lo, hi, idx, status, exceed, tally, q_obs, theta_obs, words_obs, th_all, st_all, words, toys = out
    bad = ~(np.isfinite(ref) & (ref >= 0))
    assert np.array_equal((status & BELT_NO_GRID) != 0, bad) and np.all(status[bad] & BELT_EMPTY)
    assert np.all(np.isnan(lo[bad])) and np.all(np.isnan(hi[bad])) and np.all(idx[bad] == -1)
    assert np.all(np.isnan(q_obs[bad])) and not exceed[bad].any() and not tally[bad].any()
    assert np.all(np.isnan(th_all[bad])) and np.all(np.isnan(st_all[bad])) and not words[bad].any() and not toys[bad].any()
    assert np.all(np.isnan(theta_obs[bad][:, 1:])) and not words_obs[bad][:, 1:].any()
    assert not np.isnan(theta_obs[:, :, 0]).any() and not np.isnan(q_obs[~bad]).any()
    # a singular observed best fit (tests/test_inject.py's class: two identical templates without priors): NO_FIT
    T2 = np.stack([T[0], T[0]])
    out = detector.belt_host(R, S, data, frac, P, SEED, templates=T2, background=B, raw=True)
    status, exceed, q_obs, words_obs, st_all = out[3], out[4], out[6], out[8], out[10]
    nofit = (words_obs[:, :, 0] & FAIL) != 0
    assert nofit.any() and np.array_equal((status & BELT_NO_FIT) != 0, nofit)
    assert np.all(np.isnan(q_obs[nofit])) and not exceed[nofit].any() and np.all(np.isnan(st_all[nofit]))
    assert np.all(status[nofit] & BELT_EMPTY) and np.all(np.isnan(out[0][nofit]))
    # data of zeros, upper mode: theta_hat_0 = 0, q_obs = 0 at a = 0 and every toy with a statistic counts: LO_EDGE
    out = detector.belt_host(R, S, np.zeros(5), frac, P, SEED, mode="upper", alpha=0.2, background=B)
    lo, idx, status, exceed, tally, q_obs = out[0], out[2], out[3], out[4], out[5], out[6]
    assert np.all(q_obs[..., 0] == 0) and np.array_equal(exceed[..., 0], P - tally[..., 0, 0] - tally[..., 0, 1])
    assert np.all(idx[..., 0] == 0) and np.all(status & BELT_LO_EDGE) and np.all(lo == 0)
    # upper mode with data: every grid point below theta_hat_0 has q_obs = +0.0, so all its toys count and it is accepted
    out = detector.belt_host(R, S[:2], 10.0 * data + 20.0, [0.0, 0.01, 50.0], P, SEED, mode="upper", alpha=0.2, background=B)
    idx, status, exceed, tally, q_obs, theta_obs = out[2], out[3], out[4], out[5], out[6], out[7]
    below = theta_obs[:, :, 1:, 0] < theta_obs[:, :, :1, 0]
    assert below[..., :2].all() and np.all(_bits(q_obs[below]) == 0)
    assert np.array_equal(exceed[below], (P - tally[..., 0] - tally[..., 1])[below])
    assert np.all(idx[..., 0] == 0) and np.all(status & BELT_LO_EDGE)


def test_host_form_refusals():
    R, S, B, T, data = _case(5, seed=4)
    ok = dict(background=B)
    for bad in ([], [0.0, 0.0], [1.0, 0.5], [-1.0, 1.0], [0.0, np.nan], [0.0, np.inf], np.arange(65.0)):
        with pytest.raises(ValueError):
            detector.belt_host(R, S, data, bad, P, 1, **ok)
    for bad in (0.0, 1.0, -0.1, np.nan):
        with pytest.raises(ValueError):
            detector.belt_host(R, S, data, [0.0, 1.0], P, 1, alpha=bad, **ok)
    for mode in ("discovery", detector.INJECT_DISCOVERY, "sideways"):
        with pytest.raises(ValueError):
            detector.belt_host(R, S, data, [0.0, 1.0], P, 1, mode=mode, **ok)
    with pytest.raises(ValueError):
        detector.belt_host(R, S, data, [0.0, 1.0], 0, 1, **ok)
    with pytest.raises(ValueError):
        detector.belt_host(R, S[:, :-1], data, [0.0, 1.0], P, 1, **ok)
    for bad in (data[:-1], -data - 1.0, data * np.nan):
        with pytest.raises(ValueError):
            detector.belt_host(R, S, bad, [0.0, 1.0], P, 1, **ok)
