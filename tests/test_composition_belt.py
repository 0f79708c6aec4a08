"""The toy-calibrated region of the flavour composition on the CPU: detector.composition_belt_host, the host form of
nusi_plan_response_composition_belt (include/nusi.h; DESIGN.md sec. 4, "The composition region"), with
detector.composition_accept and detector.composition_tally.

  * the symbols, their argument counts, the constants, the size check and the refusals without a plan;
  * the host form on synthetic rows (test_fit_components.py's flavour-telling rows), C in {5, 17}, K in {0, 1}, Q = 2,
    G = 4, P = 6: the observed side against fit_components_host, fit_host / profile_host on compose_host's rows and
    composition_statistic, the toys against draw_host, a toy's record against the same host forms, the counts from the
    raw arrays and the mask from the counts -- all bit for bit;
  * NaN and 0 at invalid points (identical rows with a background: SINGULAR, NO_FIT) and the FLAT path, which is valid;
  * composition_accept on hand-made counts, strict at exceed == alpha nv.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_NOT_CONVERGED, FIT_SINGULAR, FIT_ZERO,
                                   REGION_ALL, REGION_BAD_POINT, REGION_EMPTY, REGION_NO_FIT)
from nusiprop_amd.response import compose_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAIL = FIT_NOT_CONVERGED | FIT_SINGULAR
SEED = 20261021
NEW = {"nusi_composition_belt_shape": 7, "nusi_plan_response_composition_belt": 25,
       "nusi_plan_response_composition_belt_host": 24}


# --- the ABI ------------------------------------------------------------------------------------------------------------
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
    macro = {k: int(v, 0) for k, v in re.findall(r"^#define (NUSI_REGION_[A-Z_]+) (\w+)$", text, flags=re.M)}
    assert macro == {"NUSI_REGION_GRID_MAX": 1024, "NUSI_REGION_NO_FIT": 1, "NUSI_REGION_BAD_POINT": 2,
                     "NUSI_REGION_EMPTY": 4, "NUSI_REGION_ALL": 8}
    assert detector.REGION_GRID_MAX == _lib.REGION_GRID_MAX == macro["NUSI_REGION_GRID_MAX"]
    assert (REGION_NO_FIT, REGION_BAD_POINT, REGION_EMPTY, REGION_ALL) == (1, 2, 4, 8)
    assert (_lib.REGION_NO_FIT, _lib.REGION_BAD_POINT, _lib.REGION_EMPTY, _lib.REGION_ALL) == (1, 2, 4, 8)
    dp = ctypes.POINTER(ctypes.c_double)
    one = np.ones(8)
    p = one.ctypes.data_as(dp)
    refused = (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    nul = [None] * 12
    assert L.nusi_plan_response_composition_belt(None, None, 1, p, 1, p, p, 0, 1, 1, 1, 0.1, *nul, None) in refused
    assert L.nusi_plan_response_composition_belt_host(None, p, 1, p, 1, p, p, 0, 1, 1, 1, 0.1, *nul) in refused


def test_the_size_check():
    """nusi_composition_belt_shape, the check the call applies: every limit, one past it, and the last allowed value."""
    from nusiprop_amd import _lib
    L = _lib.load()
    shape = L.nusi_composition_belt_shape
    units = ctypes.c_longlong(-1)
    OK, BAD = _lib.NUSI_OK, _lib.NUSI_EPARAM
    # units = ntab ceil(Q G / QB), QB = 256 >> ceil(log2 C)
    assert shape(64, 3, 7, 11, 21, 5, ctypes.byref(units)) == OK and units.value == 7 * -(-11 * 21 // 4)
    assert shape(5, 0, 2, 3, 4, 6, ctypes.byref(units)) == OK and units.value == 2 * 1
    assert shape(1, 0, 1, 1, 1, 1, None) == OK
    assert shape(64, 3, 1, 1 << 19, 1, 1, None) == OK and shape(64, 3, 1, (1 << 19) + 1, 1, 1, None) == BAD
    assert shape(5, 0, 1, 1, 1024, 1, None) == OK and shape(5, 0, 1, 1, 1025, 1, None) == BAD
    assert shape(5, 0, 1, 1, 1, _lib.DRAW_DATASETS_MAX, None) == OK
    assert shape(5, 0, 1, 1, 1, _lib.DRAW_DATASETS_MAX + 1, None) == BAD
    for C, K, ntab, Q, G, P in ((5, 4, 1, 1, 1, 1), (5, -1, 1, 1, 1, 1), (65, 0, 1, 1, 1, 1), (0, 0, 1, 1, 1, 1),
                                (5, 0, 0, 1, 1, 1), (5, 0, -2, 1, 1, 1), (5, 0, 1, 0, 1, 1), (5, 0, 1, 1, 0, 1),
                                (5, 0, 1, 1, -1, 1), (5, 0, 1, 1, 1, 0), (5, 0, 1, 1, 1, -1)):
        assert shape(C, K, ntab, Q, G, P, None) == BAD, (C, K, ntab, Q, G, P)
    for Q, G in ((1000, 1), (16, 66), (4096, 21), (1 << 19, 1024)):
        # ceil(2^31 / (Q G)) tables are refused whatever the widths ...
        assert shape(1, 0, -(-(1 << 31) // (Q * G)), Q, G, 1, None) == BAD
        # ... and the limit itself sits at the widest observed output, theta_obs: (1 + G) (3 + K) elements a pair
        for C, K in ((1, 0), (17, 1), (64, 3)):
            W = (1 + G) * (3 + K)
            edge = -(-(1 << 31) // (Q * W))
            assert shape(C, K, edge, Q, G, 1, None) == BAD, (C, K, Q, G)
            if edge > 1:
                assert shape(C, K, edge - 1, Q, G, 1, ctypes.byref(units)) == OK, (C, K, Q, G)
                QB = 256 >> detector._ceil_log2(C)
                assert units.value == (edge - 1) * -(-Q * G // QB)


# --- synthetic rows ----------------------------------------------------------------------------------------------------
def rows(C, K, seed, ntab=2, M=6, Q=2):
    """Three flavour-telling rows a table (test_fit_components.py's), spectra, K templates with a mixed prior, a
    background and data around a truth inside the triangle."""
    rng = np.random.default_rng([seed, C, K])
    x = np.linspace(0.0, 3.0, C)
    R3 = np.stack([[np.outer(0.5 + rng.random(M), np.exp(-(0.3 + 0.5 * j) * x) * (0.7 + 0.6 * rng.random(C))) for j in range(3)]
                   for _ in range(ntab)])
    S = rng.uniform(0.5, 2.0, (Q, M))
    T = np.stack([np.exp(-2.5 * x) * 8.0, np.ones(C)])[:K] if K else None
    prior = (np.array([1.0, 2.0])[:K], np.array([0.3, np.inf])[:K]) if K else None
    B = np.full(C, 0.25)
    truth = np.array([40.0, 10.0, 25.0])
    mean = (truth[:, None] * detector.events_host(R3[0].reshape(3, M, C), S[0])).sum(axis=0) + B
    mean = mean + (np.array([1.0, 2.0])[:K] @ T if K else 0.0)
    data = rng.poisson(mean).astype(np.float64)
    return R3, S, T, prior, B, data


PHI = np.array([[1.0, 2.0, 0.0], [1.0, 0.0, 0.0], [0.4, 0.1, 0.25], [1.0, 1.0, 1.0]]) / np.array([[3.0], [1.0], [1.0], [3.0]])
_CACHE = {}


def belt(C, K):
    """The host form's raw output of a class, computed once."""
    if (C, K) not in _CACHE:
        R3, S, T, prior, B, data = rows(C, K, 7)
        out = detector.composition_belt_host(R3, S, data, PHI, 6, SEED, alpha=0.25, templates=T, prior=prior, background=B,
                                             exp=math.exp, log=math.log, raw=True)
        _CACHE[(C, K)] = ((R3, S, T, prior, B, data), out)
    return _CACHE[(C, K)]


CLASSES = [(C, K) for C in (5, 17) for K in (0, 1)]


def _held(Rc, S, d, T, prior, B):
    if T is None:
        ah, _, mu, st = detector.profile_host(Rc, S, d, background=B, log=math.log)
        return ah[..., None], mu, st
    th, _, mu, st = detector.fit_host(Rc, S, d, T, prior=prior, background=B, log=math.log)
    return th, mu, st


@pytest.mark.parametrize("C,K", CLASSES)
def test_observed_side(C, K):
    """theta_obs, words_obs equal fit_components_host and fit_host / profile_host on compose_host's rows; q_obs equals
    max(2 composition_statistic, 0): bit for bit."""
    (R3, S, T, prior, B, data), out = belt(C, K)
    accept, status, best, exceed, tally, q_obs, th_obs, w_obs = out[:8]
    ntab, Q, G = R3.shape[0], S.shape[0], len(PHI)
    assert accept.shape == (ntab, Q, G) and accept.dtype == bool and status.shape == best.shape == (ntab, Q)
    assert exceed.shape == (ntab, Q, G) and tally.shape == (ntab, Q, G, 4) and q_obs.shape == (ntab, Q, G)
    assert th_obs.shape == (ntab, Q, 1 + G, 3 + K) and w_obs.shape == (ntab, Q, 1 + G)
    assert status.dtype == best.dtype == exceed.dtype == tally.dtype == w_obs.dtype == np.int32
    free = detector.fit_components_host(R3, S, data, T, prior=prior, background=B, log=math.log)
    assert np.array_equal(th_obs[:, :, 0], free[0]) and np.array_equal(w_obs[:, :, 0], free[3])
    Rc = compose_host(R3, PHI)
    for t in range(ntab):
        th, mu, st = _held(Rc[t], S, data, T, prior, B)             # (G, Q, .)
        assert np.array_equal(th_obs[t, :, 1:, :1 + K], np.swapaxes(th, 0, 1))
        assert np.all(th_obs[t, :, 1:, 1 + K:] == 0.0) and not np.any(np.signbit(th_obs[t, :, 1:, 1 + K:]))
        assert np.array_equal(w_obs[t, :, 1:], st.T)
        lam, _ = detector.composition_statistic(mu, th, free[2][t][None], free[0][t][None], data, prior=prior, log=math.log)
        assert not np.any((st | free[3][t][None]) & FAIL)
        assert np.array_equal(q_obs[t], np.maximum(2.0 * lam, 0.0).T)
    assert np.any(q_obs > 1e-3) and np.all(best >= 0)


@pytest.mark.parametrize("C,K", CLASSES)
def test_toys_and_their_records(C, K):
    """The toys equal draw_host rows of the observed held fit's mu (stream = t, row = q G + g); a toy's record equals the
    host forms against that toy; exceed and tally follow from the raw arrays; the mask from the counts."""
    (R3, S, T, prior, B, data), out = belt(C, K)
    accept, status, best, exceed, tally, q_obs, th_obs, w_obs, th_all, st_all, words, toys = out
    ntab, Q, G, P = R3.shape[0], S.shape[0], len(PHI), 6
    assert th_all.shape == (ntab, Q, G, P, 3 + K) and st_all.shape == (ntab, Q, G, P)
    assert words.shape == (ntab, Q, G, P, 2) and toys.shape == (ntab, Q, G, P, C)
    Rc = compose_host(R3, PHI)
    seen = 0
    for t in range(ntab):
        _, mu, _ = _held(Rc[t], S, data, T, prior, B)
        mu_inj = np.swapaxes(mu, 0, 1).reshape(Q * G, C)
        want = detector.draw_host(mu_inj, P, SEED, stream=t, exp=math.exp, log=math.log).reshape(Q, G, P, C)
        assert np.array_equal(toys[t], want)
        for q, g, p in ((0, 0, 0), (Q - 1, G - 1, P - 1), (0, 2, 3), (Q - 1, 1, 1)):
            d = toys[t, q, g, p]
            free = detector.fit_components_host(R3[t], S[q], d, T, prior=prior, background=B, log=math.log)
            th, mu_t, st = _held(Rc[t, g], S[q], d, T, prior, B)
            assert words[t, q, g, p].tolist() == [int(free[3]), int(st)]
            assert np.array_equal(th_all[t, q, g, p], free[0])
            lam, _ = detector.composition_statistic(mu_t, th, free[2], free[0], d, prior=prior, log=math.log)
            assert st_all[t, q, g, p] == max(2.0 * float(lam), 0.0)
            seen |= int(free[3])
    assert np.array_equal(tally, detector.composition_tally(words))
    assert np.array_equal(exceed, (st_all >= q_obs[..., None]).sum(axis=-1))
    assert np.all(tally[..., 2] <= P) and tally[..., 2].sum() > 0      # (signal components at zero: the normal case)
    valid = ((w_obs[:, :, :1] | w_obs[:, :, 1:]) & FAIL) == 0
    a2, s2, b2 = detector.composition_accept(exceed, tally, valid, 0.25, P, q_obs)
    assert np.array_equal(a2, accept) and np.array_equal(s2, status) and np.array_equal(b2, best)
    nv = P - tally[..., 0] - tally[..., 1]
    assert np.array_equal(accept, valid & (nv > 0) & (exceed > 0.25 * nv))
    # without raw: the first eight arrays alone, the same bits
    short = detector.composition_belt_host(R3[:1], S, data, PHI, 2, SEED, alpha=0.25, templates=T, prior=prior, background=B,
                                           exp=math.exp, log=math.log)
    assert len(short) == 8 and np.array_equal(short[5], q_obs[:1])


# --- invalid points ------------------------------------------------------------------------------------------------------
def test_singular_is_no_fit():
    """Identical rows with a background: the free fit is SINGULAR, the pair NO_FIT; q_obs NaN, counts 0, raw NaN / 0."""
    R3, S, T, prior, B, data = rows(17, 0, 3, ntab=1)
    R3[:, 1] = R3[:, 0]
    R3[:, 2] = R3[:, 0]
    out = detector.composition_belt_host(R3, S, data, PHI, 3, SEED, background=B, exp=math.exp, log=math.log, raw=True)
    accept, status, best, exceed, tally, q_obs, th_obs, w_obs, th_all, st_all, words, toys = out
    assert np.all(w_obs[:, :, 0] & FIT_SINGULAR)
    assert np.all(status == (REGION_NO_FIT | REGION_EMPTY)) and np.all(best == -1) and not accept.any()
    assert np.all(np.isnan(q_obs)) and not exceed.any() and not tally.any()
    assert np.all(np.isnan(th_all)) and np.all(np.isnan(st_all)) and not words.any() and not toys.any()
    # the held fits are still recorded: one row and a scale, nothing singular about them
    assert not np.any(w_obs[:, :, 1:] & FAIL) and np.all(th_obs[:, :, 1:, 0] > 0)


def test_flat_is_valid():
    """A spectrum of zeros: no signal component is live, both fits are FLAT and nothing is flagged, so the points are
    valid: q_obs is a number (the two fits reach the templates' minimum on their own iterations: 0 up to their stops),
    the toys are drawn from the templates and the background and counted."""
    R3, S, T, prior, B, data = rows(5, 1, 4, ntab=1)
    S[1] = 0.0
    out = detector.composition_belt_host(R3, S, data, PHI, 4, SEED, templates=T, prior=prior, background=B, exp=math.exp,
                                         log=math.log, raw=True)
    accept, status, best, exceed, tally, q_obs, th_obs, w_obs, th_all, st_all, words, toys = out
    assert np.all(w_obs[0, 1] & FIT_FLAT) and not np.any(w_obs[0, 1] & FAIL)
    assert np.all(th_obs[0, 1, 0, :3] == 0.0) and np.all(th_obs[0, 1, 0, 3:] > 0)
    assert np.all(th_obs[0, 1, 1:, 0] == 0.0) and np.all(th_obs[0, 1, 1:, 1] > 0)
    assert np.all(words[0, 1, :, :, 0] & FIT_FLAT) and not np.any(words[0, 1] & FAIL)
    assert np.all(q_obs[0, 1] >= 0.0) and np.all(q_obs[0, 1] < 1e-9) and np.all(st_all[0, 1] < 1e-9)
    assert np.array_equal(exceed[0, 1], (st_all[0, 1] >= q_obs[0, 1][:, None]).sum(axis=-1))
    assert np.array_equal(tally[0, 1], np.array([[0, 0, 4, 0]] * 4))
    assert best[0, 1] >= 0 and (status[0, 1] & (REGION_NO_FIT | REGION_BAD_POINT)) == 0
    assert toys[0, 1].any()                                       # (the templates and the background are drawn)


# --- the acceptance rule -----------------------------------------------------------------------------------------------------
def test_accept_by_hand():
    P, alpha = 8, 0.25
    ty = np.zeros((1, 4, 4), dtype=np.int32)
    q = np.array([[3.0, 1.0, 1.0, 2.0]])
    # strict at exceed == alpha nv: nv = 8, alpha nv = 2.0
    acc, st, best = detector.composition_accept(np.array([[2, 3, 1, 8]]), ty, None, alpha, P, q)
    assert acc.tolist() == [[False, True, False, True]] and st.tolist() == [0] and best.tolist() == [1]   # (a tie: the lowest g)
    assert acc.dtype == bool and st.dtype == best.dtype == np.int32
    # nv shrinks with tally[0] + tally[1]: nv = 4, alpha nv = 1.0; tally[2] and [3] do not enter
    ty2 = ty.copy()
    ty2[0, :, 0], ty2[0, :, 1], ty2[0, :, 2], ty2[0, :, 3] = 3, 1, 7, 5
    acc, st, best = detector.composition_accept(np.array([[1, 2, 0, 4]]), ty2, None, alpha, P, q)
    assert acc.tolist() == [[False, True, False, True]] and st.tolist() == [0]
    # _EMPTY; _ALL; both words with flags
    acc, st, _ = detector.composition_accept(np.array([[0, 2, 1, 0]]), ty, None, alpha, P, q)
    assert not acc.any() and st.tolist() == [REGION_EMPTY]
    acc, st, _ = detector.composition_accept(np.array([[3, 8, 4, 5]]), ty, None, alpha, P, q, flags=np.array([REGION_BAD_POINT]))
    assert acc.all() and st.tolist() == [REGION_ALL | REGION_BAD_POINT]
    # an invalid point is never accepted, does not stand in the way of _ALL and cannot be best
    valid = np.array([[True, False, False, True]])
    acc, st, best = detector.composition_accept(np.array([[3, 8, 8, 5]]), ty, valid, alpha, P, q)
    assert acc.tolist() == [[True, False, False, True]] and st.tolist() == [REGION_ALL] and best.tolist() == [3]
    # nv = 0 at a valid point: _BAD_POINT, not accepted; at an invalid one it says nothing
    ty3 = ty.copy()
    ty3[0, 1, 0], ty3[0, 1, 1] = 5, 3
    acc, st, _ = detector.composition_accept(np.array([[3, 8, 4, 5]]), ty3, None, alpha, P, q)
    assert acc.tolist() == [[True, False, True, True]] and st.tolist() == [REGION_BAD_POINT]
    acc, st, _ = detector.composition_accept(np.array([[3, 8, 4, 5]]), ty3, np.array([[True, False, True, True]]), alpha, P, q)
    assert st.tolist() == [REGION_ALL]
    # no valid point: _EMPTY without _ALL, best -1
    acc, st, best = detector.composition_accept(np.array([[3, 8, 4, 5]]), ty, np.zeros((1, 4), dtype=bool), alpha, P, q,
                                                flags=REGION_NO_FIT)
    assert not acc.any() and st.tolist() == [REGION_NO_FIT | REGION_EMPTY] and best.tolist() == [-1]
    with pytest.raises(ValueError):
        detector.composition_accept(np.zeros((1, 4)), ty[:, :3], None, alpha, P, q)


def test_tally_by_hand():
    w = np.zeros((1, 6, 2), dtype=np.int32)
    w[0, 0] = (FIT_SINGULAR, FIT_NOT_CONVERGED)                     # the free fit failed (and the held fit: counted once)
    w[0, 1] = (3, FIT_SINGULAR | 2)                                 # the held fit alone
    w[0, 2] = (FIT_ZERO << 1 | 4, 0)                                # a signal component at zero
    w[0, 3] = (FIT_ZERO << 3 | 4, FIT_BOUNDARY)                     # a TEMPLATE at zero; the held fit's BOUNDARY: neither counts
    w[0, 4] = (FIT_FLAT | FIT_INFINITE, 0)
    w[0, 5] = (FIT_BOUNDARY | 7 * FIT_ZERO, 0)
    assert detector.composition_tally(w).tolist() == [[1, 1, 3, 1]]


def test_refusals():
    R3, S, T, prior, B, data = rows(5, 0, 1, ntab=1)
    ok = dict(R3=R3, S=S, data=data, phi=PHI, P=2, seed=1)
    for bad in (dict(phi=np.array([[1.0, -0.5, 0.5]])), dict(phi=np.array([[np.nan, 0.5, 0.5]])), dict(phi=np.zeros((2, 3))),
                dict(phi=np.ones((2, 4))), dict(phi=np.ones((3, 2, 3))), dict(phi=np.ones((detector.REGION_GRID_MAX + 1, 3))),
                dict(P=0), dict(alpha=0.0), dict(alpha=1.0), dict(data=-data), dict(data=data[:-1]), dict(R3=R3[:, :2]),
                dict(S=S[:, :-1])):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            detector.composition_belt_host(kw.pop("R3"), kw.pop("S"), kw.pop("data"), kw.pop("phi"), kw.pop("P"), kw.pop("seed"), **kw)
    # phi per table
    out = detector.composition_belt_host(R3, S, data, PHI[None], 1, 1, background=B)
    assert out[0].shape == (1, 2, 4)
