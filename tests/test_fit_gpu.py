"""The fit with floating background templates on the GPU: k_detector_fit (nusi_plan_response_fit).

Yardstick: detector.fit_host (numpy), the same operations in the same order, so theta, status and mu are compared with
np.array_equal.  nll passes through the log and is held to the events test's bound with the penalties' operations
counted in: 2 (C + 3 + 3 K) u (sum_c (mu_c + |data_c log mu_c|) + sum_j pen_j) -- per penalty a difference, two
products and an addition on either side -- against fit_host with the oracle's ora_log, with +inf in the same places.

Shapes: a block of the kernel holds 256 >> ceil(log2 C) groups of ONE spectrum, a group 2^ceil(log2 C) lanes inside one
wave.  C = 1 is a group of one lane (64 fits per wave), C = 3, 5 and 17 have padded lanes in the butterfly, C = 64 is one
group per wave with all six stages; Q = 1, 5 and 19 give partial blocks, Q = 600 at C = 1, 2 several blocks.  K = 1 and
3 are the smallest and the largest instance (2 and 4 components); K = 2 runs in the synthetic classes.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_ITER_MAX, FIT_NOT_CONVERGED, FIT_SINGULAR,
                                   FIT_STEPS_MASK, FIT_TRIALS_MASK, FIT_TRIALS_SHIFT, FIT_ZERO)
from tests.test_detector_gpu import (GRIDS, MAXIS, _B, _D, _Dev, _folded, _hip, _ora_log, _plan, _spectra,
                                     nusi)  # noqa: F401  (nusi: the fixture)
from tests.test_profile_gpu import _fetch_int, _synthetic

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
N = GRIDS["G6"][0]
U = 2.0 ** -53


def _templates(C, K, scale=1.0, gamma0=0.5):
    """K falling templates exp(-gamma_j x) over the bins, gamma_j 0.4 apart; nothing in the detector's dead last bin."""
    x = np.linspace(0.0, 3.0, C) if C > 1 else np.zeros(1)
    T = np.stack([scale * (1.0 + j) * np.exp(-(gamma0 + 0.4 * j) * x) for j in range(K)])
    if C > 1:
        T[:, C - 1] = 0.0
    return T


def _check(got, R, S, data, T, prior, B, log, what, quiet=False):
    """theta, status and mu equal fit_host's bits; nll within the bound of the module's docstring.  Returns the host's."""
    theta, nll, mu, st = got
    hth, hn, hm, hs = detector.fit_host(R, S, data, T, prior=prior, background=B, log=log)
    assert theta.shape == hth.shape and st.shape == hs.shape and mu.shape == hm.shape and st.dtype == np.int32
    assert np.array_equal(st, hs), (what, np.argwhere(st != hs)[:4], [hex(v) for v in st[st != hs][:4]],
                                    [hex(v) for v in hs[st != hs][:4]])
    assert np.array_equal(theta, hth), (what, np.argwhere(theta != hth)[:4])
    assert np.array_equal(mu, hm), what
    C, K = len(data), len(T)
    inf = np.isinf(hn)
    assert np.array_equal(np.isinf(nll), inf) and np.all(nll[inf] > 0), what
    assert np.array_equal(inf, (hs & FIT_INFINITE) != 0), what
    m, w = detector._prior(K, prior)
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.sum(mu + np.where(data > 0, np.abs(data * np.log(np.where(mu > 0, mu, 1.0))), 0.0), axis=-1)
    mag = mag + np.sum(0.5 * w * (theta - m) ** 2, axis=-1)
    bound = 2 * (C + 3 + 3 * K) * U * mag
    fin = ~inf
    ratio = float(np.max(np.abs(nll[fin] - hn[fin]) / bound[fin])) if np.any(fin) else 0.0
    steps, halv = hs & FIT_STEPS_MASK, (hs >> FIT_TRIALS_SHIFT) & FIT_TRIALS_MASK
    if not quiet:
        print("%s: nll ratio to the bound %.3f; steps %d .. %d (mean %.2f), halvings mean %.2f max %d, %d flat, %d singular, "
              "%d not converged, %d infinite" % (what, ratio, steps.min(), steps.max(), steps.mean(), halv.mean(), halv.max(),
                                                 np.count_nonzero(hs & FIT_FLAT), np.count_nonzero(hs & FIT_SINGULAR),
                                                 np.count_nonzero(hs & FIT_NOT_CONVERGED), int(inf.sum())))
    assert ratio <= 1.0, (what, ratio)
    assert np.all(steps <= FIT_ITER_MAX), what
    return hth, hn, hm, hs


def _data(R, S, T, B, C, seed):
    """Counts around theta_0 s + sum_j T_j + B for table 0's first spectrum, theta_0 its scale of 200 signal events in
    the fullest bin; some bins empty."""
    s = detector.events_host(R, S)[0, 0]
    data = np.floor((200.0 / s.max() * s + T.sum(axis=0) + B) * (0.5 + np.random.default_rng(seed).random(C)))
    if C > 7:
        data[::5] = 0.0
    if C == 1:
        data[0] += 1.0
    return data


def _prior_of(T, kind):
    K = len(T)
    if kind == "none":
        return None
    if kind == "loose":
        return (np.full(K, 1.2), np.full(K, 0.5))
    return (np.full(K, 1.2), np.array([0.05, np.inf, 0.3][:K]))     # "mixed": a tight one, none, a loose one


# --- a real fold: the G6 tables ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
@pytest.mark.parametrize("Q", (1, 5, 19))
def test_fit_equals_the_host_form(nusi, oracle_mod, Q, C, K):  # noqa: F811
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0)
    data = _data(R, S, T, B, C, seed=C + Q)
    if C > 1:
        data[C - 1] = 0.0                           # the bin nothing ever fills
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    for kind in ("none", "mixed"):
        prior = _prior_of(T, kind)
        plan.set_templates(T, prior=prior)
        assert plan.templates() == K
        got = plan.fit(R, S, data)
        hth, hn, hm, hs = _check(got, R, S, data, T, prior, B, log, "G6 C=%d Q=%d K=%d prior %s" % (C, Q, K, kind))
        if np.count_nonzero(data) >= 1 + K:         # enough bins with data to determine every component
            assert not np.any(hs & (FIT_NOT_CONVERGED | FIT_SINGULAR)) and np.all(np.isfinite(got[1]))
        if C > 1:                                   # a count where nothing is expected: +inf, the flag, the same theta
            d2 = data.copy()
            d2[C - 1] = 2.0
            got2 = plan.fit(R, S, d2)
            _check(got2, R, S, d2, T, prior, B, log, "... a count where nothing is expected", quiet=True)
            assert np.all(np.isinf(got2[1])) and np.array_equal(got2[0], got[0])
            assert np.array_equal(got2[3], got[3] | FIT_INFINITE)
    plan.close()


# --- synthetic matrices: fits that part ways inside one wave ---------------------------------------------------------------
FIT_CLASSES = (("no background", False, "zero", "none", 1), ("background 1e-300", False, "tiny", "loose", 2),
               ("signal over decades", True, "zero", "none", 3), ("a template that is not there", False, "alike", "none", 3),
               ("tight priors far from the truth", False, "alike", "far", 2), ("data below the templates", False, "alike", "below", 3),
               ("signals of different shapes", False, "zero", "shapes", 2), ("shapes over decades", True, "tiny", "shapes", 3))


def _fit_case(C, what, decades, bkind, pkind, K, ntab=3, Q=40):
    """(R, S, data, T, prior, B) of one call.  The data follow one (table, spectrum) plus the templates; the other
    spectra, decades apart, fit what they can."""
    R, S = _synthetic(C, ntab, Q, seed=len(what), decades=decades)
    rng = np.random.default_rng(C + len(what))
    if pkind == "shapes":                                       # every row of R a bump somewhere else, spectra of 1 .. 3 rows
        c0, wd = rng.uniform(0, C, (ntab, M, 1)), rng.uniform(0.5, C / 3 + 1, (ntab, M, 1))
        R = R * np.exp(-((np.arange(C)[None, None, :] - c0) / wd) ** 2)
        pick = rng.random((Q, M)) < 2.0 / M
        pick[np.arange(Q), rng.integers(1, M, Q)] = True
        S = S * pick
    S[3::16] = 0.0                                              # spectra of zeros among the groups of a wave
    ev = detector.events_host(R, S)[1]
    ref = ev[np.argsort(ev.sum(axis=-1))[Q // 2]]               # table 1's median spectrum
    a0 = 1e3 / ref.max()
    T = _templates(C, K, scale=50.0)
    if C > 1:
        T[:, C - 1] = T[:, 0] * 1e-3                            # (no dead bin here)
    B = {"zero": np.zeros(C), "tiny": 1e-300 * (0.5 + rng.random(C)), "alike": 30.0 * (0.5 + rng.random(C))}[bkind]
    truth = np.ones(K)
    if what == "a template that is not there":
        truth[K - 1] = 0.0
    if pkind == "below":
        truth[:] = 0.05
    mean = a0 * ref + truth @ T + B
    data = mean * (0.5 + rng.random(C)) if what == "no background" else rng.poisson(mean).astype(np.float64)
    if C > 4:
        data[1] = 0.0
    prior = {"none": None, "below": None, "shapes": None, "loose": (np.full(K, 1.0), np.full(K, 0.5)),
             "far": (np.full(K, 30.0), np.array([1e-2, 3.0, 1e-3][:K]))}[pkind]
    if prior is None and C <= K:                                # fewer bins than components: only priors determine them
        prior = (np.full(K, 1.0), np.full(K, 0.5))
    return R, S, data, T, prior, B


def _parted(hs, per_wave):
    """Do fits that share a wave (per_wave consecutive spectra of a table) differ in steps, halvings and zero bits?"""
    steps, halv, zero = hs & FIT_STEPS_MASK, (hs >> FIT_TRIALS_SHIFT) & FIT_TRIALS_MASK, (hs >> 16) & 0xF
    out = [False, False, False]
    for t in range(hs.shape[0]):
        for q0 in range(0, hs.shape[1], per_wave):
            for i, x in enumerate((steps, halv, zero)):
                out[i] |= len(set(x[t, q0:q0 + per_wave].tolist())) > 1
    return out


@pytest.mark.parametrize("C", (1, 3, 5, 17, 64))
def test_fits_that_part_ways_inside_a_wave(nusi, oracle_mod, C):  # noqa: F811
    """Groups of one wave stop after different numbers of steps, take different numbers of halvings and end with
    different free sets: the run masks, the divergent solve and the full-exec butterflies are what can go wrong.  At
    C = 64 a wave holds one group; there the waves of a block part ways instead."""
    log = _ora_log(oracle_mod)
    plan = _plan(nusi, "G6")
    D = _D(C, N)
    lg = int(np.ceil(np.log2(C))) if C > 1 else 0
    per_wave = max(64 >> lg, 4)                     # (C = 64: the four waves of a block)
    parted, flags = np.zeros(3, dtype=bool), 0
    for what, decades, bkind, pkind, K in FIT_CLASSES:
        R, S, data, T, prior, B = _fit_case(C, what, decades, bkind, pkind, K)
        plan.set_detector(D, background=B)
        plan.set_templates(T, prior=prior)
        got = plan.fit(R, S, data)
        hth, hn, hm, hs = _check(got, R, S, data, T, prior, B, log, "C=%d K=%d %s" % (C, K, what))
        parted |= np.array(_parted(hs, per_wave))
        flags |= int(np.bitwise_or.reduce(hs.ravel()))
    plan.close()
    assert parted.all(), parted                     # steps, halvings, free sets
    assert flags & (0xF * FIT_ZERO) and (C == 1 or flags & FIT_BOUNDARY), hex(flags)


@pytest.mark.parametrize("C", (1, 2))
def test_many_spectra_on_few_bins(nusi, oracle_mod, C):  # noqa: F811
    """Q = 600 is several blocks (256 fits a block at C = 1, 128 at C = 2) with a partial last one.  One bin cannot
    determine two components, so the template has a prior.  The device form writes into buffers of NaNs (status: of
    -1): no entry may be left unwritten."""
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    Q, K = 600, 1
    S = _spectra(M, Q)
    T = np.array([[4.0, 7.0][:C]])
    prior = (np.array([1.0]), np.array([0.2]))
    data = np.array([9.0, 0.0][:C])
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=prior)
    got = plan.fit(R, S, data)
    hth, hn, hm, hs = _check(got, R, S, data, T, prior, B, log, "G6 C=%d Q=%d" % (C, Q))
    assert not np.any(hs & (FIT_NOT_CONVERGED | FIT_SINGULAR))
    H = _hip()
    with _Dev(H) as dev:
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        dT, dN = dev.alloc(got[0].nbytes, np.full((3, Q, 1 + K), np.nan)), dev.alloc(got[1].nbytes, np.full((3, Q), np.nan))
        dM = dev.alloc(got[2].nbytes, np.full((3, Q, C), np.nan))
        dS = dev.alloc(got[3].nbytes, np.full((3, Q), -1, dtype=np.int32))
        assert plan.fit_device(dR, 3, S, data, dT, dN, dM, dS) == Q
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dT, (3, Q, 1 + K)), got[0]) and np.array_equal(dev.fetch(dN, (3, Q)), got[1])
        assert np.array_equal(dev.fetch(dM, (3, Q, C)), got[2]) and np.array_equal(_fetch_int(H, dS, (3, Q)), got[3])
    plan.close()


def test_spectra_and_data_of_zeros(nusi, oracle_mod):  # noqa: F811
    log = _ora_log(oracle_mod)
    C, Q, K = 5, 7, 2
    R, D, B = _folded(nusi, C)
    S = np.array(_spectra(M, Q))
    S[2] = 0.0                                      # spectra of zeros among the groups of a wave
    S[4] = 0.0
    T = _templates(C, K, scale=20.0)
    data = _data(R, S, T, B, C, seed=1)
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T)
    got = plan.fit(R, S, data)
    _check(got, R, S, data, T, None, B, log, "G6 C=5, two spectra of zeros")
    for q in (2, 4):                                # flat: no signal, and the templates are fitted all the same
        assert np.all(got[3][:, q] & FIT_FLAT) and np.all(got[0][:, q, 0] == 0.0) and np.all(got[0][:, q, 1:].sum(axis=-1) > 0)
        assert np.array_equal(got[0][0, q], got[0][1, q])
    assert not np.any(np.delete(got[3], (2, 4), axis=1) & FIT_FLAT)
    zero = np.zeros(C)
    got0 = plan.fit(R, S, zero)                     # data of zeros and no priors: theta = 0, nll = sum of the background
    _check(got0, R, S, zero, T, None, B, log, "G6 C=5, data of zeros")
    assert np.all(got0[0] == 0.0) and np.all(got0[3] == (FIT_FLAT | 7 * FIT_ZERO))
    assert np.array_equal(got0[1], np.full((3, Q), detector.poisson_host(B, zero)))
    plan.close()


# --- equivalence and consistency ----------------------------------------------------------------------------------------
def test_tables_alone_and_the_device_forms(nusi):  # noqa: F811
    C, Q, K = 17, 19, 3
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0)
    data = _data(R, S, T, B, C, seed=2)
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=_prior_of(T, "mixed"))
    theta, nll, mu, st = plan.fit(R, S, data)
    assert len({theta[t].tobytes() for t in range(3)}) == 3
    for t in range(3):                              # a 3-table call against each table alone, and a spectrum alone
        one = plan.fit(R[t:t + 1], S, data)
        for x, y in zip(one, (theta, nll, mu, st)):
            assert np.array_equal(x[0], y[t]), t
    one = plan.fit(R, S[6:7], data)
    for x, y in zip(one, (theta, nll, mu, st)):
        assert np.array_equal(x[:, 0], y[:, 6])
    H = _hip()
    with _Dev(H) as dev:                            # into NaN-filled buffers, each optional output NULL in turn
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        for skip in (None, "nll", "mu", "status"):
            dT, dN = dev.alloc(theta.nbytes, np.full(theta.shape, np.nan)), dev.alloc(nll.nbytes, np.full(nll.shape, np.nan))
            dM = dev.alloc(mu.nbytes, np.full(mu.shape, np.nan))
            dS = dev.alloc(st.nbytes, np.full(st.shape, -1, dtype=np.int32))
            assert plan.fit_device(dR, 3, S, data, dT, None if skip == "nll" else dN, None if skip == "mu" else dM,
                                   None if skip == "status" else dS) == Q
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(dev.fetch(dT, theta.shape), theta), skip
            n2, m2, s2 = dev.fetch(dN, nll.shape), dev.fetch(dM, mu.shape), _fetch_int(H, dS, st.shape)
            assert np.all(np.isnan(n2)) if skip == "nll" else np.array_equal(n2, nll), skip
            assert np.all(np.isnan(m2)) if skip == "mu" else np.array_equal(m2, mu), skip
            assert np.all(s2 == -1) if skip == "status" else np.array_equal(s2, st), skip
    # the profile is untouched by the templates: it still fits a s + B alone
    a, _, _, _ = plan.profile(R, S, data)
    assert np.array_equal(a, detector.profile_host(R, S, data, background=B)[0])
    plan.close()


# --- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(nusi):  # noqa: F811
    from nusiprop_amd import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    C, K = 5, 2
    R, D, B = _folded(nusi, C)
    S = _spectra(M, 2)
    data = np.ones(C)
    T = _templates(C, K)
    plan = _plan(nusi, "G6")

    def refused(code, f, *a, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*a, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    refused(_lib.NUSI_ESTATE, plan.set_templates, T)                                        # no detector
    refused(_lib.NUSI_ESTATE, plan.fit, np.ones((1, M, C)), S, data)
    plan.set_detector(D, background=B)
    assert plan.templates() == 0
    refused(_lib.NUSI_ESTATE, plan.fit, R, S, data)                                         # no templates
    assert L.nusi_plan_response_fit(plan._h, None, 1, Sp, 2, datap, None, None, None, None, None) == _lib.NUSI_ESTATE
    for bad in (-1.0, np.nan, np.inf):
        Tb = T.copy()
        Tb[1, 2] = bad
        refused(_lib.NUSI_EPARAM, plan.set_templates, Tb)
        if bad != np.inf:
            refused(_lib.NUSI_EPARAM, plan.set_templates, T, prior=(None, [1.0, bad]))
        refused(_lib.NUSI_EPARAM, plan.set_templates, T, prior=([1.0, bad], [1.0, 1.0]))
    refused(_lib.NUSI_EPARAM, plan.set_templates, T, prior=(None, [1.0, 0.0]))
    Tz = T.copy()
    Tz[0] = 0.0
    refused(_lib.NUSI_EPARAM, plan.set_templates, Tz)                                       # a template of zeros
    refused(_lib.NUSI_EPARAM, plan.set_templates, np.ones((4, C)))                          # K = 4
    with pytest.raises(ValueError):
        plan.set_templates(np.ones((2, C + 1)))
    assert plan.templates() == 0                                                            # the refusals set nothing
    plan.set_templates(T, prior=([1.0, 1.0], [np.inf, 0.5]))                                # (+inf: no prior, accepted)
    assert plan.templates() == K
    want = plan.fit(R, S, data)
    refused(_lib.NUSI_EPARAM, plan.fit, R, S, None)                                         # NULL data
    for bad in (-1.0, np.nan, np.inf):
        db, Sb = data.copy(), np.array(S)
        db[C - 1] = bad
        Sb[1, M - 1] = bad
        refused(_lib.NUSI_EPARAM, plan.fit, R, S, db)
        refused(_lib.NUSI_EPARAM, plan.fit, R, Sb, data)
    with pytest.raises(ValueError):
        plan.fit(R[:, :-1], S, data)
    with pytest.raises(ValueError):
        plan.fit(R, S, data[:-1])
    H = _hip()
    with _Dev(H) as dev:
        dR, dT = dev.alloc(R.nbytes, np.ascontiguousarray(R)), dev.alloc(3 * 2 * (1 + K) * 8)
        ft = L.nusi_plan_response_fit
        assert ft(plan._h, dR, 3, Sp, 2, datap, None, None, None, None, None) == _lib.NUSI_EPARAM      # no theta
        assert ft(plan._h, dR, 3, Sp, 2, None, dT, None, None, None, None) == _lib.NUSI_EPARAM         # no data
        assert ft(plan._h, None, 3, Sp, 2, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM
        assert ft(plan._h, dR, 0, Sp, 2, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM
        assert ft(plan._h, dR, 3, Sp, 0, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM
    got = plan.fit(R, S, data)                      # the refusals changed nothing
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    plan.set_templates(None)                        # cleared by hand ...
    assert plan.templates() == 0
    plan.set_templates(T)
    plan.set_detector(D, background=B)              # ... and by a new detector
    assert plan.templates() == 0
    refused(_lib.NUSI_ESTATE, plan.fit, R, S, data)
    plan.close()
