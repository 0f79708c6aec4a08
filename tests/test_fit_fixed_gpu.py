"""The conditional fit on the GPU: k_conditional_fit (nusi_plan_response_fit_fixed), the fit's templates with the
signal's scale held.

Yardstick: detector.fit_fixed_host (numpy), the same operations in the same order, so theta, status and mu are compared
with np.array_equal; nll is held to test_fit_gpu._check's bound, 2 (C + 3 + 3 K) u (sum_c (mu_c + |data_c log mu_c|) +
sum_j pen_j), against the host form with the oracle's ora_log, with +inf in the same places.  (The host form itself is
held against profile_host, fit_host and exact arithmetic in tests/test_fit_fixed.py.)

Shapes: the kernel has k_detector_fit's block shape -- 256 >> ceil(log2 C) groups of ONE spectrum, a group
2^ceil(log2 C) lanes inside one wave: C = 1 is a group of one lane, C = 3, 5 and 17 pad the butterfly, C = 64 is one group
per wave; Q = 1, 5, 19 give partial blocks, Q = 600 at C = 1, 2 several.  K = 1 and 3 are the smallest and the largest
instance; K = 2 runs in the synthetic classes.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_ITER_MAX, FIT_NOT_CONVERGED, FIT_SINGULAR,
                                   FIT_STEPS_MASK, FIT_TRIALS_MASK, FIT_TRIALS_SHIFT, FIT_ZERO)
from tests.test_detector_gpu import (GRIDS, MAXIS, _D, _Dev, _folded, _hip, _ora_log, _plan, _spectra,
                                     nusi)  # noqa: F401  (nusi: the fixture)
from tests.test_fit_gpu import FIT_CLASSES, _data, _fit_case, _parted, _prior_of, _templates
from tests.test_profile_gpu import _fetch_int

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
N = GRIDS["G6"][0]
U = 2.0 ** -53


def _check(got, R, S, a, data, T, prior, B, log, what, quiet=False):
    """theta, status and mu equal fit_fixed_host's bits; nll within the bound of the module's docstring.  Returns the
    host's."""
    theta, nll, mu, st = got
    hth, hn, hm, hs = detector.fit_fixed_host(R, S, a, data, T, prior=prior, background=B, log=log)
    assert theta.shape == hth.shape and st.shape == hs.shape and mu.shape == hm.shape and st.dtype == np.int32
    assert np.array_equal(st, hs), (what, np.argwhere(st != hs)[:4], [hex(v) for v in st[st != hs][:4]],
                                    [hex(v) for v in hs[st != hs][:4]])
    assert np.array_equal(theta, hth), (what, np.argwhere(theta != hth)[:4])
    assert np.array_equal(mu, hm), what
    assert np.array_equal(theta[..., 0], np.broadcast_to(a, theta.shape[:-1])), what
    assert not np.any(hs & (FIT_FLAT | FIT_BOUNDARY | FIT_ZERO)), what
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
        print("%s: nll ratio to the bound %.3f; steps %d .. %d (mean %.2f), halvings mean %.2f max %d, %d singular, "
              "%d not converged, %d infinite" % (what, ratio, steps.min(), steps.max(), steps.mean(), halv.mean(), halv.max(),
                                                 np.count_nonzero(hs & FIT_SINGULAR), np.count_nonzero(hs & FIT_NOT_CONVERGED),
                                                 int(inf.sum())))
    assert ratio <= 1.0, (what, ratio)
    assert np.all(steps <= FIT_ITER_MAX), what
    return hth, hn, hm, hs


# --- a real fold: the G6 tables ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
@pytest.mark.parametrize("Q", (1, 5, 19))
def test_fit_fixed_equals_the_host_form(nusi, oracle_mod, Q, C, K):  # noqa: F811
    """Scales 0, theta_hat_0 and 3 theta_hat_0 (of table 0's global fit) side by side in one call's scale[q], in every
    rotation, so that every spectrum sees each."""
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
        best = plan.fit(R, S, data)
        a0 = best[0][0, :, 0]
        a0 = np.where(a0 > 0, a0, 200.0 / np.maximum(detector.events_host(R, S)[0].max(axis=-1), 1e-300))
        for rot in range(3):
            a = a0 * np.array([0.0, 1.0, 3.0])[(np.arange(Q) + rot) % 3]
            got = plan.fit_fixed(R, S, a, data)
            hth, hn, hm, hs = _check(got, R, S, a, data, T, prior, B, log,
                                     "G6 C=%d Q=%d K=%d prior %s rot %d" % (C, Q, K, kind, rot), quiet=rot > 0)
            if np.count_nonzero(data) >= K:         # enough bins with data to determine every template
                assert not np.any(hs & FIT_NOT_CONVERGED)
        if C > 1:                                   # a count where nothing is expected: +inf, the flag, the same theta
            d2 = data.copy()
            d2[C - 1] = 2.0
            got2 = plan.fit_fixed(R, S, a, d2)
            _check(got2, R, S, a, d2, T, prior, B, log, "... a count where nothing is expected", quiet=True)
            assert np.all(np.isinf(got2[1])) and np.array_equal(got2[0], got[0])
            assert np.array_equal(got2[3], got[3] | FIT_INFINITE)
        after = plan.fit(R, S, data)                # the fit is untouched by the calls between
        for x, y in zip(after, best):
            assert np.array_equal(x, y)
    plan.close()


# --- synthetic matrices: fits that part ways inside one wave ---------------------------------------------------------------
def _class_scales(R, S):
    """Held scales decades apart between neighbouring spectra: 10^-4 .. 10^2 times the scale of 1e3 signal events in
    table 1's fullest bin, and 0 for every eleventh spectrum."""
    top = detector.events_host(R, S)[1].max(axis=-1)
    Q = len(S)
    a = np.where(top > 0, 1e3 / np.where(top > 0, top, 1.0), 1.0) * 10.0 ** ((np.arange(Q) % 7) - 4.0)
    a[5::11] = 0.0
    return a


@pytest.mark.parametrize("C", (1, 3, 5, 17, 64))
def test_fits_that_part_ways_inside_a_wave(nusi, oracle_mod, C):  # noqa: F811
    """test_fit_gpu's eight classes with per-spectrum scales decades apart: groups of one wave stop after different
    numbers of steps, take different numbers of halvings and end with different zero sets.  At C = 64 a wave holds one
    group; there the waves of a block part ways instead."""
    log = _ora_log(oracle_mod)
    plan = _plan(nusi, "G6")
    D = _D(C, N)
    lg = int(np.ceil(np.log2(C))) if C > 1 else 0
    per_wave = max(64 >> lg, 4)                     # (C = 64: the four waves of a block)
    parted, flags = np.zeros(3, dtype=bool), 0
    for what, decades, bkind, pkind, K in FIT_CLASSES:
        R, S, data, T, prior, B = _fit_case(C, what, decades, bkind, pkind, K)
        a = _class_scales(R, S)
        plan.set_detector(D, background=B)
        plan.set_templates(T, prior=prior)
        got = plan.fit_fixed(R, S, a, data)
        hth, hn, hm, hs = _check(got, R, S, a, data, T, prior, B, log, "C=%d K=%d %s" % (C, K, what))
        parted |= np.array(_parted(hs, per_wave))
        flags |= int(np.bitwise_or.reduce(hs.ravel()))
    plan.close()
    assert parted.all(), parted                     # steps, halvings, zero sets
    assert flags & (0xE * FIT_ZERO), hex(flags)


@pytest.mark.parametrize("C", (1, 2))
def test_many_spectra_on_few_bins(nusi, oracle_mod, C):  # noqa: F811
    """Q = 600 is several blocks (256 fits a block at C = 1, 128 at C = 2) with a partial last one.  The device form
    writes into buffers of NaNs (status: of -1): no entry may be left unwritten."""
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    Q, K = 600, 1
    S = _spectra(M, Q)
    T = np.array([[4.0, 7.0][:C]])
    prior = (np.array([1.0]), np.array([0.2]))
    data = np.array([9.0, 0.0][:C])
    a = (2.0 / np.maximum(detector.events_host(R, S)[0].max(axis=-1), 1e-300)) * (np.arange(Q) % 5)
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=prior)
    got = plan.fit_fixed(R, S, a, data)
    hth, hn, hm, hs = _check(got, R, S, a, data, T, prior, B, log, "G6 C=%d Q=%d" % (C, Q))
    assert not np.any(hs & (FIT_NOT_CONVERGED | FIT_SINGULAR))
    H = _hip()
    with _Dev(H) as dev:
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        dT, dN = dev.alloc(got[0].nbytes, np.full((3, Q, 1 + K), np.nan)), dev.alloc(got[1].nbytes, np.full((3, Q), np.nan))
        dM = dev.alloc(got[2].nbytes, np.full((3, Q, C), np.nan))
        dS = dev.alloc(got[3].nbytes, np.full((3, Q), -1, dtype=np.int32))
        assert plan.fit_fixed_device(dR, 3, S, a, data, dT, dN, dM, dS) == Q
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dT, (3, Q, 1 + K)), got[0]) and np.array_equal(dev.fetch(dN, (3, Q)), got[1])
        assert np.array_equal(dev.fetch(dM, (3, Q, C)), got[2]) and np.array_equal(_fetch_int(H, dS, (3, Q)), got[3])
    plan.close()


# --- equivalence and consistency ----------------------------------------------------------------------------------------
def test_tables_alone_the_device_forms_and_the_fit(nusi):  # noqa: F811
    C, Q, K = 17, 19, 3
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0)
    data = _data(R, S, T, B, C, seed=2)
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=_prior_of(T, "mixed"))
    best = plan.fit(R, S, data)
    a = best[0][1, :, 0] * np.array([0.0, 1.0, 3.0])[np.arange(Q) % 3]
    theta, nll, mu, st = plan.fit_fixed(R, S, a, data)
    assert len({theta[t].tobytes() for t in range(3)}) == 3
    for t in range(3):                              # a 3-table call against each table alone, and a spectrum alone
        one = plan.fit_fixed(R[t:t + 1], S, a, data)
        for x, y in zip(one, (theta, nll, mu, st)):
            assert np.array_equal(x[0], y[t]), t
    one = plan.fit_fixed(R, S[6:7], a[6:7], data)
    for x, y in zip(one, (theta, nll, mu, st)):
        assert np.array_equal(x[:, 0], y[:, 6])
    # the conditional minimum is not below the global one -- either computed nll is within _check's bound of the
    # host form's, and that within the same bound of the exact value: twice each call's bound -- and on table 1, where
    # a = theta_hat_0, it is the global one within those bounds
    m, w = detector._prior(K, _prior_of(T, "mixed"))

    def mag(mu_, th_):
        with np.errstate(divide="ignore", invalid="ignore"):
            x = np.sum(mu_ + np.where(data > 0, np.abs(data * np.log(np.where(mu_ > 0, mu_, 1.0))), 0.0), axis=-1)
        return x + np.sum(0.5 * w * (th_ - m) ** 2, axis=-1)

    tol = 2 * 2 * (C + 3 + 3 * K) * U * (mag(mu, theta) + mag(best[2], best[0]))
    assert np.all(nll >= best[1] - tol)
    same = np.arange(Q) % 3 == 1
    assert np.all(np.abs(nll[1, same] - best[1][1, same]) <= tol[1, same])
    H = _hip()
    with _Dev(H) as dev:                            # into NaN-filled buffers, each optional output NULL in turn
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        for skip in (None, "nll", "mu", "status"):
            dT, dN = dev.alloc(theta.nbytes, np.full(theta.shape, np.nan)), dev.alloc(nll.nbytes, np.full(nll.shape, np.nan))
            dM = dev.alloc(mu.nbytes, np.full(mu.shape, np.nan))
            dS = dev.alloc(st.nbytes, np.full(st.shape, -1, dtype=np.int32))
            assert plan.fit_fixed_device(dR, 3, S, a, data, dT, None if skip == "nll" else dN,
                                         None if skip == "mu" else dM, None if skip == "status" else dS) == Q
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(dev.fetch(dT, theta.shape), theta), skip
            n2, m2, s2 = dev.fetch(dN, nll.shape), dev.fetch(dM, mu.shape), _fetch_int(H, dS, st.shape)
            assert np.all(np.isnan(n2)) if skip == "nll" else np.array_equal(n2, nll), skip
            assert np.all(np.isnan(m2)) if skip == "mu" else np.array_equal(m2, mu), skip
            assert np.all(s2 == -1) if skip == "status" else np.array_equal(s2, st), skip
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
    a = np.array([0.0, 1e-3])
    plan = _plan(nusi, "G6")

    def refused(code, f, *args, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*args, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    Sp, datap, ap = S.ctypes.data_as(dp), data.ctypes.data_as(dp), a.ctypes.data_as(dp)
    refused(_lib.NUSI_ESTATE, plan.fit_fixed, np.ones((1, M, C)), S, a, data)                # no detector
    plan.set_detector(D, background=B)
    refused(_lib.NUSI_ESTATE, plan.fit_fixed, R, S, a, data)                                 # no templates: that is events
    ff = L.nusi_plan_response_fit_fixed
    assert ff(plan._h, None, 1, Sp, 2, ap, datap, None, None, None, None, None) == _lib.NUSI_ESTATE
    plan.set_templates(T, prior=([1.0, 1.0], [np.inf, 0.5]))
    want_fit, want = plan.fit(R, S, data), plan.fit_fixed(R, S, a, data)
    refused(_lib.NUSI_EPARAM, plan.fit_fixed, R, S, a, None)                                 # NULL data
    with pytest.raises(ValueError):
        plan.fit_fixed(R, S, None, data)                                                     # no scale
    for bad in (-1.0, np.nan, np.inf):
        db, Sb, ab = data.copy(), np.array(S), a.copy()
        db[C - 1] = bad
        Sb[1, M - 1] = bad
        ab[1] = bad
        refused(_lib.NUSI_EPARAM, plan.fit_fixed, R, S, a, db)
        refused(_lib.NUSI_EPARAM, plan.fit_fixed, R, Sb, a, data)
        refused(_lib.NUSI_EPARAM, plan.fit_fixed, R, S, ab, data)                            # a scale
    with pytest.raises(ValueError):
        plan.fit_fixed(R[:, :-1], S, a, data)
    with pytest.raises(ValueError):
        plan.fit_fixed(R, S, a, data[:-1])
    with pytest.raises(ValueError):
        plan.fit_fixed(R, S, np.ones(3), data)                                               # three scales, two spectra
    H = _hip()
    with _Dev(H) as dev:
        dR, dT = dev.alloc(R.nbytes, np.ascontiguousarray(R)), dev.alloc(3 * 2 * (1 + K) * 8)
        assert ff(plan._h, dR, 3, Sp, 2, ap, datap, None, None, None, None, None) == _lib.NUSI_EPARAM   # no theta
        assert ff(plan._h, dR, 3, Sp, 2, ap, None, dT, None, None, None, None) == _lib.NUSI_EPARAM      # no data
        assert ff(plan._h, dR, 3, Sp, 2, None, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM   # no scale
        assert ff(plan._h, None, 3, Sp, 2, ap, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM
        assert ff(plan._h, dR, 0, Sp, 2, ap, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM
        assert ff(plan._h, dR, 3, Sp, 0, ap, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM
    for x, y in zip(plan.fit_fixed(R, S, a, data), want):                                    # the refusals changed nothing
        assert np.array_equal(x, y)
    for x, y in zip(plan.fit(R, S, data), want_fit):                                         # ... and fit gives what it did
        assert np.array_equal(x, y)
    plan.set_detector(D, background=B)                                                       # a new detector clears the templates
    refused(_lib.NUSI_ESTATE, plan.fit_fixed, R, S, a, data)
    plan.close()
