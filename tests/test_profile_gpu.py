"""The statistic profiled over the flux normalisation on the GPU: k_detector_profile (nusi_plan_response_profile).

Yardstick: detector.profile_host (numpy), the same operations in the same order, so ahat, status and mu are compared
with np.array_equal; nll passes through the log and is held to the events test's own bound,
2 (C + 3) u sum (mu + |data log mu|), against profile_host with the oracle's ora_log, with +inf in the same places.

Shapes: a block of the kernel holds 256 >> ceil(log2 C) groups of four spectra, a group 2^ceil(log2 C) lanes inside
one wave.  C = 1 is a group of one lane, C = 5 and 17 have padded lanes in the butterfly (8 and 32 lanes), C = 64 is
one group per wave with all six butterfly stages; Q = 1, 5 and 19 give a partial group of four and a partial last
block, Q = 600 at C = 1, 2 a block with more spectra than threads.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_ITER_MAX, FIT_NOT_CONVERGED, FIT_STEPS_MASK
from tests.test_detector_gpu import (GRIDS, MAXIS, _B, _D, _Dev, _check_nll, _folded, _hip, _ora_log, _plan, _spectra,
                                     nusi)  # noqa: F401  (nusi: the fixture)

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
N = GRIDS["G6"][0]


def _fetch_int(H, ptr, shape):
    out = np.zeros(shape, dtype=np.int32)
    assert H.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0
    return out


def _check(got, R, S, data, B, log, what):
    """ahat, status and mu equal profile_host's bits; nll within the events test's bound of it.  Returns the host's."""
    ahat, nll, mu, st = got
    ha, hn, hm, hs = detector.profile_host(R, S, data, background=B, log=log)
    assert ahat.shape == ha.shape and st.shape == hs.shape and mu.shape == hm.shape and st.dtype == np.int32
    assert np.array_equal(st, hs), (what, np.argwhere(st != hs)[:4])
    assert np.array_equal(ahat, ha), (what, np.argwhere(ahat != ha)[:4])
    assert np.array_equal(mu, hm), what
    _check_nll(nll, mu, data, log, what)
    assert np.array_equal(np.isinf(nll), (st & FIT_INFINITE) != 0), what
    steps = st & FIT_STEPS_MASK
    assert not np.any(st & FIT_NOT_CONVERGED) and np.all(steps <= FIT_ITER_MAX), what
    print("%s: steps %d .. %d (mean %.2f), %d flat, %d at the boundary, %d infinite" % (
        what, steps.min(), steps.max(), steps.mean(), np.count_nonzero(st & FIT_FLAT), np.count_nonzero(st & FIT_BOUNDARY),
        np.count_nonzero(st & FIT_INFINITE)))
    return ha, hn, hm, hs


def _data(R, S, B, C, seed):
    """Counts around a s + B for table 0's first spectrum, a its scale of 200 signal events in the fullest bin (the
    other tables and spectra then fit scales of that order); some bins empty."""
    s = detector.events_host(R, S)[0, 0]
    data = np.floor((200.0 / s.max() * s + B) * (0.5 + np.random.default_rng(seed).random(C)))
    if C > 3:
        data[::3] = 0.0
    if C == 1:
        data[0] += 1.0
    return data


# --- a real fold: the G6 tables ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 5, 17, 64))
@pytest.mark.parametrize("Q", (1, 5, 19))
def test_profile_equals_the_host_form(nusi, oracle_mod, Q, C):  # noqa: F811
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    data = _data(R, S, B, C, seed=C + Q)
    if C > 1:
        data[C - 1] = 0.0                           # the bin the detector never fills, and no background there
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    got = plan.profile(R, S, data)
    ha, hn, hm, hs = _check(got, R, S, data, B, log, "G6 C=%d Q=%d" % (C, Q))
    assert np.all(np.isfinite(got[1])) and np.all(ha > 0) and not np.any(hs & ~FIT_STEPS_MASK)
    if C > 1:                                       # a count in that bin: +inf, the flag, and the same ahat
        d2 = data.copy()
        d2[C - 1] = 2.0
        got2 = plan.profile(R, S, d2)
        _check(got2, R, S, d2, B, log, "G6 C=%d Q=%d, a count where nothing is expected" % (C, Q))
        assert np.all(np.isinf(got2[1])) and np.array_equal(got2[0], got[0]) and np.array_equal(got2[3], got[3] | FIT_INFINITE)
    plan.close()


# --- synthetic matrices: the edge classes ------------------------------------------------------------------------------
def _synthetic(C, ntab, Q, seed, decades):
    """Non-negative R (ntab, M, C) and S (Q, M) whose signals differ by many orders of magnitude between tables, spectra
    and (decades) bins, so the chains of one lane and the groups of one wave stop after different numbers of steps."""
    rng = np.random.default_rng([seed, C])
    R = rng.random((ntab, M, C)) * 10.0 ** rng.uniform(-4, 4, (ntab, 1, 1))
    if decades:
        R = R * 10.0 ** rng.uniform(-12, 12, (ntab, 1, C))
    keep = rng.random((ntab, 1)) < 0.7
    keep[1] = True                                              # (table 1 is the one the data follow)
    R[:, :, C // 2] *= keep                                     # a bin without signal in some tables
    S = rng.random((Q, M)) * 10.0 ** rng.uniform(-3, 3, (Q, 1))
    S[:, 1::2] *= (rng.random((Q, 1)) < 0.5)                    # sparse spectra
    return np.ascontiguousarray(R), np.ascontiguousarray(S)


EDGE_CLASSES = (("no background", False, "zero"), ("background 1e-300", False, "tiny"),
                ("background-dominated", False, "big"), ("signal over decades", True, "zero"),
                ("data below the background", False, "above"), ("signal and background alike", False, "alike"))


def _edge_case(C, what, decades, bkind, ntab=4, Q=23):
    """(R, S, data, B) of one call.  The data follow one (table, spectrum); the others fit a scale to it."""
    R, S = _synthetic(C, ntab, Q, seed=len(what), decades=decades)
    ref = detector.events_host(R, S)[1, Q // 2]
    rng = np.random.default_rng(C + len(what))
    a0 = 1e4 / ref.max()
    B = {"zero": np.zeros(C), "tiny": 1e-300 * (0.5 + rng.random(C)), "big": 1e6 * a0 * ref + 1e6,
         "above": np.full(C, 40.0), "alike": 1e3 * (0.5 + rng.random(C))}[bkind]
    if bkind == "above":
        data = rng.poisson(25.0, C).astype(np.float64)
    elif what == "no background":
        data = a0 * ref * (0.5 + rng.random(C))                 # non-integer
    elif bkind == "big":                                        # an excess the background's fluctuations do not hide
        data = rng.poisson(B) + np.floor(30.0 * np.sqrt(B))
    else:
        data = rng.poisson(a0 * ref + B).astype(np.float64)
    if C > 2 and bkind != "big":                                # (an empty bin there would outweigh the excess: a = 0)
        data[1] = 0.0
    return R, S, data, B


@pytest.mark.parametrize("C", (1, 3, 5, 17, 64))
def test_edge_classes(nusi, oracle_mod, C):  # noqa: F811
    log = _ora_log(oracle_mod)
    plan = _plan(nusi, "G6")
    D = _D(C, N)
    steps_seen, lanes_differ, groups_differ = set(), False, False
    for what, decades, bkind in EDGE_CLASSES:
        R, S, data, B = _edge_case(C, what, decades, bkind)
        plan.set_detector(D, background=B)
        got = plan.profile(R, S, data)
        ha, hn, hm, hs = _check(got, R, S, data, B, log, "C=%d %s" % (C, what))
        if bkind == "above":
            assert np.any(hs & FIT_BOUNDARY)
        steps = hs & FIT_STEPS_MASK
        steps_seen |= set(steps.ravel().tolist())
        lanes_differ |= any(len(set(steps[t, q:q + 4].tolist())) > 1 for t in range(len(steps)) for q in range(0, 20, 4))
        groups_differ |= any(steps[t, 0] != steps[t, 4 * k] for t in range(len(steps)) for k in range(1, 5))
    plan.close()
    # the four chains of a lane, and the groups of a wave, do stop after different numbers of steps
    assert lanes_differ and groups_differ and len(steps_seen) >= 3, steps_seen


@pytest.mark.parametrize("C", (1, 2))
def test_many_spectra_on_few_bins(nusi, oracle_mod, C):  # noqa: F811
    """A block owns 1024 spectra at C = 1 and 512 at C = 2, more than it has threads (the statistic's pass strides over
    them); Q = 600 also crosses a block boundary at C = 2.  The device form writes into buffers of NaNs (status: of
    -1): no entry may be left unwritten."""
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    Q = 600
    S = _spectra(M, Q)
    data = np.array([3.0, 0.0][:C])
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    got = plan.profile(R, S, data)
    _check(got, R, S, data, B, log, "G6 C=%d Q=%d" % (C, Q))
    H = _hip()
    with _Dev(H) as dev:
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        dA, dN = dev.alloc(got[0].nbytes, np.full((3, Q), np.nan)), dev.alloc(got[1].nbytes, np.full((3, Q), np.nan))
        dM = dev.alloc(got[2].nbytes, np.full((3, Q, C), np.nan))
        dS = dev.alloc(got[3].nbytes, np.full((3, Q), -1, dtype=np.int32))
        assert plan.profile_device(dR, 3, S, data, dA, dN, dM, dS) == Q
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dA, (3, Q)), got[0]) and np.array_equal(dev.fetch(dN, (3, Q)), got[1])
        assert np.array_equal(dev.fetch(dM, (3, Q, C)), got[2]) and np.array_equal(_fetch_int(H, dS, (3, Q)), got[3])
    plan.close()


def test_spectra_and_data_of_zeros(nusi, oracle_mod):  # noqa: F811
    log = _ora_log(oracle_mod)
    C, Q = 5, 7
    R, D, B = _folded(nusi, C)
    S = np.array(_spectra(M, Q))
    S[2] = 0.0                                      # a spectrum of zeros, inside a group of four
    S[4] = 0.0
    data = _data(R, S, B, C, seed=1)
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    got = plan.profile(R, S, data)
    _check(got, R, S, data, B, log, "G6 C=5, two spectra of zeros")
    for q in (2, 4):
        assert np.all(got[3][:, q] == FIT_FLAT) and np.all(got[0][:, q] == 0.0) and np.array_equal(got[2][:, q], np.tile(B, (3, 1)))
    assert not np.any(np.delete(got[3], (2, 4), axis=1) & FIT_FLAT)
    zero = np.zeros(C)
    got0 = plan.profile(R, S, zero)                 # data of zeros: every fit is flat, nll = sum of the background
    _check(got0, R, S, zero, B, log, "G6 C=5, data of zeros")
    assert np.all(got0[3] == FIT_FLAT) and np.all(got0[0] == 0.0)
    assert np.array_equal(got0[1], np.full((3, Q), detector.poisson_host(B, zero)))
    plan.close()


# --- equivalence and consistency ----------------------------------------------------------------------------------------
def test_tables_alone_device_forms_and_the_events_call(nusi):  # noqa: F811
    C, Q = 17, 19
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    data = _data(R, S, B, C, seed=2)
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    ahat, nll, mu, st = plan.profile(R, S, data)
    assert np.all(ahat > 0) and len({ahat[t].tobytes() for t in range(3)}) == 3
    # a 3-table call against each table alone, and a spectrum alone
    for t in range(3):
        one = plan.profile(R[t:t + 1], S, data)
        for x, y in zip(one, (ahat, nll, mu, st)):
            assert np.array_equal(x[0], y[t]), t
    one = plan.profile(R, S[6:7], data)
    for x, y in zip(one, (ahat, nll, mu, st)):
        assert np.array_equal(x[:, 0], y[:, 6])
    # the events call at the fitted scale gives the profile's mu and nll, bit for bit
    for t in range(3):
        m, n = plan.events(R[t:t + 1], S, scale=ahat[t], data=data)
        assert np.array_equal(m[0], mu[t]) and np.array_equal(n[0], nll[t]), t
    # ... and the profile is the smaller statistic at any other scale
    _, n_other = plan.events(R, S, scale=1.01 * ahat[0], data=data)
    assert np.all(nll[0] < n_other[0])
    # the device form into NaN-filled buffers, with each optional output NULL in turn
    H = _hip()
    with _Dev(H) as dev:
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        for skip in (None, "nll", "mu", "status"):
            dA, dN = dev.alloc(ahat.nbytes, np.full(ahat.shape, np.nan)), dev.alloc(nll.nbytes, np.full(nll.shape, np.nan))
            dM = dev.alloc(mu.nbytes, np.full(mu.shape, np.nan))
            dS = dev.alloc(st.nbytes, np.full(st.shape, -1, dtype=np.int32))
            assert plan.profile_device(dR, 3, S, data, dA, None if skip == "nll" else dN, None if skip == "mu" else dM,
                                       None if skip == "status" else dS) == Q
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(dev.fetch(dA, ahat.shape), ahat), skip
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
    C = 5
    R, D, B = _folded(nusi, C)
    S = _spectra(M, 2)
    data = np.ones(C)
    plan = _plan(nusi, "G6")

    def refused(code, f, *a, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*a, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    refused(_lib.NUSI_ESTATE, plan.profile, np.ones((1, M, C)), S, data)                    # no detector
    assert L.nusi_plan_response_profile(plan._h, None, 1, Sp, 2, datap, None, None, None, None, None) == _lib.NUSI_ESTATE
    plan.set_detector(D, background=B)
    want = plan.profile(R, S, data)
    refused(_lib.NUSI_EPARAM, plan.profile, R, S, None)                                     # NULL data
    for bad in (-1.0, np.nan, np.inf):
        db, Sb = data.copy(), np.array(S)
        db[C - 1] = bad
        Sb[1, M - 1] = bad
        refused(_lib.NUSI_EPARAM, plan.profile, R, S, db)
        refused(_lib.NUSI_EPARAM, plan.profile, R, Sb, data)
    with pytest.raises(ValueError):
        plan.profile(R[:, :-1], S, data)
    with pytest.raises(ValueError):
        plan.profile(R, S, data[:-1])
    H = _hip()
    with _Dev(H) as dev:
        dR, dA = dev.alloc(R.nbytes, np.ascontiguousarray(R)), dev.alloc(3 * 2 * 8)
        pr = L.nusi_plan_response_profile
        assert pr(plan._h, dR, 3, Sp, 2, datap, None, None, None, None, None) == _lib.NUSI_EPARAM      # no ahat
        assert pr(plan._h, dR, 3, Sp, 2, None, dA, None, None, None, None) == _lib.NUSI_EPARAM         # no data
        assert pr(plan._h, None, 3, Sp, 2, datap, dA, None, None, None, None) == _lib.NUSI_EPARAM
        assert pr(plan._h, dR, 0, Sp, 2, datap, dA, None, None, None, None) == _lib.NUSI_EPARAM
        assert pr(plan._h, dR, 3, Sp, 0, datap, dA, None, None, None, None) == _lib.NUSI_EPARAM
    got = plan.profile(R, S, data)                  # the refusals changed nothing
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    plan.close()
