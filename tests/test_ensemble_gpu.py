"""Ensembles of pseudo-experiments on the GPU: k_ensemble_profile, k_ensemble_fit<NC> and k_ensemble_best
(nusi_plan_response_ensemble).

Yardstick 1, bit-exact: the plan's own per-data-set call.  For every data set p, plan.fit(R, S, data[p]) (plan.profile
on a plan without templates) reduced over the spectra with detector.argbest must equal the ensemble's q, nll, theta and
status under np.array_equal: the record of a spectrum is DEFINED as that call's, the log included.  Every shape here
is held to it, and every shape runs with the slice options at (1, 1), (2, 2) and automatic, which must agree to the bit.

Yardstick 2, the host form: detector.ensemble_host with the oracle's log.  Where q agrees with the host's, theta and
status are bit-equal and nll is within test_fit_gpu._check's bound, 2 (C + 3 + 3 K) u (sum_c (mu_c + |data_c log mu_c|)
+ sum_j pen_j).  q itself is asserted where the host's runner-up lies further from its best than the sum of the two
records' bounds -- otherwise the log's last bits may decide -- and at most 10 % of the (p, t) may be left out that way.
On one bin every spectrum fits the datum exactly and all records tie to rounding, so the host comparison runs at
C >= 5; C = 1 rests on yardstick 1.

Shapes: C = 1 (groups of one lane), 5 and 17 (padded butterflies), 64 (one group per wave); K = 0, 1, 3; Q = 1, 5, 19;
P = 1, 3, 37 (with two p-slices P = 3 splits 1 + 2); several spectrum blocks per table at Q = 600 (C = 1, 2; K = 1: 256
and 128 fits a block) and Q = 1100 (C = 1, K = 0: 1024 a block).
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from nusiprop_amd.detector import FIT_INFINITE
from tests import test_fit_gpu, test_profile_gpu
from tests.test_detector_gpu import (GRIDS, MAXIS, _B, _D, _Dev, _folded, _hip, _ora_log, _plan, _spectra,
                                     nusi)  # noqa: F401  (nusi: the fixture)
from tests.test_fit_gpu import FIT_CLASSES, _fit_case, _prior_of, _templates
from tests.test_profile_gpu import _fetch_int, _synthetic

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
N = GRIDS["G6"][0]
U = 2.0 ** -53
SLICES = ((1, 1), (2, 2), (0, 0))


def _setup(nusi, D, B, T=None, prior=None):  # noqa: F811
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    if T is not None and len(T):
        plan.set_templates(T, prior=prior)
    return plan


def _single(plan, R, S, data):
    """Yardstick 1: per data set the plan's existing call, reduced over the spectra with detector.argbest."""
    K, P, ntab = plan.templates(), len(data), R.shape[0]
    q, st = np.zeros((P, ntab), dtype=np.int32), np.zeros((P, ntab), dtype=np.int32)
    nll, theta = np.zeros((P, ntab)), np.zeros((P, ntab, 1 + K))
    rows = np.arange(ntab)
    for p in range(P):
        if K:
            th, n, _, s = plan.fit(R, S, data[p])
        else:
            a, n, _, s = plan.profile(R, S, data[p])
            th = a[..., None]
        best = detector.argbest(n)
        q[p], nll[p], theta[p], st[p] = best, n[rows, best], th[rows, best], s[rows, best]
    return q, nll, theta, st


def _same(a, b, what):
    for x, y, name in zip(a, b, ("q", "nll", "theta", "status")):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x, y, equal_nan=True), (what, name, np.argwhere(x != y)[:4], x[x != y][:4], y[x != y][:4])


def _ensemble(plan, R, S, data, what, slices=SLICES):
    """The ensemble under every slicing, bitwise equal; and equal to yardstick 1.  Returns it."""
    got = []
    for qs, ps in slices:
        plan.set_option(_lib.OPT_ENSEMBLE_QSLICES, qs)
        plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, ps)
        got.append(plan.ensemble(R, S, data))
        assert got[-1][0].dtype == np.int32 and got[-1][3].dtype == np.int32
        _same(got[-1], got[0], "%s: slices %s against %s" % (what, (qs, ps), slices[0]))
    plan.set_option(_lib.OPT_ENSEMBLE_QSLICES, 0)
    plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, 0)
    _same(got[0], _single(plan, R, S, data), what + ": against the per-data-set call")
    return got[0]


def _toys(base, P, seed):
    """P data sets of different scale around base (C,): counts, some bins emptied."""
    rng = np.random.default_rng(seed)
    d = np.floor(base[None] * (0.5 + rng.random((P, len(base)))) * 10.0 ** rng.uniform(-0.7, 0.7, (P, 1)))
    d[0] = base
    return d


def _prior_for(T, C):
    K = len(T)
    if K == 0:
        return None
    return (np.full(K, 1.2), np.full(K, 0.5)) if C <= K else _prior_of(T, "mixed")     # few bins: priors determine them


# --- a real fold: the G6 tables, every shape and slicing against the per-data-set call -----------------------------------
@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_ensemble_equals_the_per_data_set_calls(nusi, C, K):  # noqa: F811
    R, D, B = _folded(nusi, C)
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    plan = _setup(nusi, D, B, T, _prior_for(T, C))
    for Q in (1, 5, 19):
        S = _spectra(M, Q)
        base = test_fit_gpu._data(R, S, T, B, C, seed=C + Q) if K else test_profile_gpu._data(R, S, B, C, seed=C + Q)
        if C > 1:
            base[C - 1] = 0.0                               # the bin nothing ever fills
        for P in (1, 3, 37):
            data = _toys(base, P, seed=Q + P)
            got = _ensemble(plan, R, S, data, "G6 C=%d K=%d Q=%d P=%d" % (C, K, Q, P))
            assert got[0].shape == (P, 3) and got[2].shape == (P, 3, 1 + K)
            assert np.all(got[0] >= 0) and np.all(got[0] < Q) and np.all(np.isfinite(got[1]))
            if C > 1 and P == 3:                            # a count in the dead bin of ONE data set: its nll are all +inf
                d2 = data.copy()
                d2[1, C - 1] = 2.0
                got2 = _ensemble(plan, R, S, d2, "... a count where nothing is expected")
                assert np.all(got2[0][1] == 0) and np.all(np.isinf(got2[1][1])) and np.all(got2[3][1] & FIT_INFINITE)
                for x, y in zip(got2, got):                 # the other data sets are unchanged
                    assert np.array_equal(x[[0, 2]], y[[0, 2]])
    plan.close()


# --- the host form ---------------------------------------------------------------------------------------------------------
def _bounds(theta, nll_host, mu, data, T, prior, C, K):
    """test_fit_gpu._check's bound on |nll - host| for records (.., 1 + K) with their mu (.., C)."""
    m, w = detector._prior(K, prior) if K else (np.zeros(1), np.zeros(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.sum(mu + np.where(data > 0, np.abs(data * np.log(np.where(mu > 0, mu, 1.0))), 0.0), axis=-1)
    mag = mag + np.sum(0.5 * w * (theta - m) ** 2, axis=-1)
    return 2 * (C + 3 + 3 * K) * U * mag


@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (5, 17, 64))
def test_ensemble_against_the_host_form(nusi, oracle_mod, C, K):  # noqa: F811
    log = _ora_log(oracle_mod)
    ntab, Q, P = 3, 19, 3
    R, S = _synthetic(C, ntab, Q, seed=5, decades=False)
    rng = np.random.default_rng(C + K)
    ev = detector.events_host(R, S)[1]
    ref = ev[np.argsort(ev.sum(axis=-1))[Q // 2]]           # table 1's median spectrum
    T = _templates(C, K, scale=50.0) if K else np.zeros((0, C))
    B = 30.0 * (0.5 + rng.random(C))
    data = detector.pseudo_data(1e3 / ref.max() * ref + T.sum(axis=0) + B, P, rng)
    prior = _prior_for(T, C)
    plan = _setup(nusi, _D(C, N), B, T, prior)
    q, nll, theta, st = _ensemble(plan, R, S, data, "synthetic C=%d K=%d" % (C, K))
    plan.close()
    hq, hn, hth, hs = detector.ensemble_host(R, S, data, templates=T if K else None, prior=prior, background=B, log=log)
    rows = np.arange(ntab)
    asserted, ratio_max, gap_min = 0, 0.0, np.inf
    for p in range(P):
        if K:
            ath, an, amu, _ = detector.fit_host(R, S, data[p], T, prior=prior, background=B, log=log)
        else:
            a, an, amu, _ = detector.profile_host(R, S, data[p], background=B, log=log)
            ath = a[..., None]
        bound = _bounds(ath, an, amu, data[p], T, prior, C, K)                      # (ntab, Q)
        assert np.array_equal(detector.argbest(an), hq[p]) and np.array_equal(an[rows, hq[p]], hn[p])
        order = np.argsort(an, axis=-1, kind="stable")
        gap = an[rows, order[:, 1]] - an[rows, order[:, 0]]
        sure = gap > bound[rows, order[:, 0]] + bound[rows, order[:, 1]]
        gap_min = min(gap_min, float(np.min(gap / (bound[rows, order[:, 0]] + bound[rows, order[:, 1]]))))
        asserted += int(sure.sum())
        assert np.array_equal(q[p][sure], hq[p][sure]), (p, q[p], hq[p])
        agree = q[p] == hq[p]
        assert np.array_equal(theta[p][agree], hth[p][agree]) and np.array_equal(st[p][agree], hs[p][agree])
        b = bound[rows, hq[p]]
        fin = agree & np.isfinite(hn[p])
        assert np.array_equal(np.isinf(nll[p][agree]), np.isinf(hn[p][agree]))
        if fin.any():
            ratio_max = max(ratio_max, float(np.max(np.abs(nll[p][fin] - hn[p][fin]) / b[fin])))
    print("synthetic C=%d K=%d: nll ratio to the bound %.3f; q asserted at %d of %d; smallest gap %.3g bounds" % (
        C, K, ratio_max, asserted, P * ntab, gap_min))
    assert ratio_max <= 1.0
    assert asserted >= 0.9 * P * ntab, (asserted, P * ntab)


# --- several spectrum blocks per table -------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K,Q", ((1, 1, 600), (2, 1, 600), (1, 0, 1100)))
def test_many_spectra_on_few_bins(nusi, C, K, Q):  # noqa: F811
    """256 (C = 1) and 128 (C = 2) fits a block, 1024 spectra a block of the profile: several blocks per table, a
    partial last one, and with two q-slices a boundary between blocks."""
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T = np.array([[4.0, 7.0][:C]]) if K else None
    plan = _setup(nusi, D, B, T, (np.array([1.0]), np.array([0.2])) if K else None)
    data = np.array([[9.0, 0.0][:C], [2.0, 0.0][:C], [40.0, 0.0][:C]])
    got = _ensemble(plan, R, S, data, "G6 C=%d K=%d Q=%d" % (C, K, Q), slices=SLICES + ((3, 1), (1, 3)))
    assert np.all(np.isfinite(got[1]))
    plan.close()


# --- ties: the lowest q ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 1))
def test_identical_spectra_resolve_to_the_lowest_q(nusi, K):  # noqa: F811
    """Spectrum 10 again at q = 300, both the family's best fit for table 0: at C = 5 a block holds 32 fits (128 spectra
    of the profile), so the pair lies in different blocks, and with two q-slices in different slices."""
    C, Q = 5, 320
    R, D, B = _folded(nusi, C)
    S = np.array(_spectra(M, Q))
    S[300] = S[10]
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    s10 = detector.events_host(R, S)[0, 10]
    data = np.stack([a * s10 + T.sum(axis=0) + B for a in (100.0 / s10.max(), 700.0 / s10.max())])   # table 0, q = 10: exact
    plan = _setup(nusi, D, B, T, None)
    got = _ensemble(plan, R, S, data, "the pair, K=%d" % K, slices=((1, 1), (2, 1), (2, 2), (10, 2), (0, 0)))
    assert np.all(got[0][:, 0] == 10), got[0]
    assert not np.any(got[0] == 300)
    # the pair does tie: alone, the copy's record has the original's bits
    one = plan.ensemble(R, S[[300, 10]], data)
    assert np.all(one[0][:, 0] == 0)
    for x, y in zip(one[1:], got[1:]):
        assert np.array_equal(x[:, 0], y[:, 0])
    plan.close()


# --- zeros, and fits that part ways across the data sets -----------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 2))
def test_spectra_and_data_of_zeros(nusi, K):  # noqa: F811
    C, Q = 5, 7
    R, D, B = _folded(nusi, C)
    S = np.array(_spectra(M, Q))
    S[2] = 0.0                                      # spectra of zeros among the groups of a wave
    S[4] = 0.0
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    base = test_fit_gpu._data(R, S, T, B, C, seed=1)
    base[C - 1] = 0.0
    data = np.stack([base, np.zeros(C), 2.0 * base])            # a data set of zeros between two others
    plan = _setup(nusi, D, B, T, None)
    got = _ensemble(plan, R, S, data, "zeros, K=%d" % K)
    assert np.all(got[2][1] == 0.0) and np.all(got[0][1] == 0)  # data of zeros: theta = 0 for every spectrum, q = 0
    assert np.all(got[1][1] == detector.poisson_host(B, np.zeros(C)))
    plan.close()


@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_fits_that_part_ways_across_data_sets(nusi, C):  # noqa: F811
    """test_fit_gpu's classes, whose fits stop after different numbers of steps, halvings and free sets inside a wave,
    with three data rows of different scale: the run masks and counters are set anew for every data set."""
    plan = _plan(nusi, "G6")
    D = _D(C, N)
    differ = False
    for what, decades, bkind, pkind, K in FIT_CLASSES:
        R, S, data, T, prior, B = _fit_case(C, what, decades, bkind, pkind, K)
        plan.set_detector(D, background=B)
        plan.set_templates(T, prior=prior)
        rows = np.stack([data, np.floor(0.05 * data), 7.0 * data + 1.0])
        got = _ensemble(plan, R, S, rows, "C=%d K=%d %s" % (C, K, what))
        differ |= len({got[3][p].tobytes() for p in range(3)}) > 1
        plan.set_templates(None)                                # ... and the profile's iteration on the same rows
        _ensemble(plan, R, S, rows, "C=%d K=0 %s" % (C, what), slices=((1, 1), (2, 2)))
    plan.close()
    assert differ


# --- the device form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 3))
def test_device_form(nusi, K):  # noqa: F811
    C, Q, P = 17, 19, 3
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    base = test_fit_gpu._data(R, S, T, B, C, seed=2)
    base[C - 1] = 0.0
    data = _toys(base, P, seed=4)
    plan = _setup(nusi, D, B, T, _prior_for(T, C))
    q, nll, theta, st = plan.ensemble(R, S, data)
    H = _hip()
    with _Dev(H) as dev:                            # into NaN / -1 filled buffers, each optional output NULL in turn
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        for qs in (1, 2):
            plan.set_option(_lib.OPT_ENSEMBLE_QSLICES, qs)
            for skip in (None, "theta", "status"):
                dQ, dS = dev.alloc(q.nbytes, np.full(q.shape, -1, dtype=np.int32)), dev.alloc(st.nbytes, np.full(st.shape, -1, dtype=np.int32))
                dN, dT = dev.alloc(nll.nbytes, np.full(nll.shape, np.nan)), dev.alloc(theta.nbytes, np.full(theta.shape, np.nan))
                assert plan.ensemble_device(dR, 3, S, data, dQ, dN, None if skip == "theta" else dT,
                                            None if skip == "status" else dS) == (Q, P)
                assert H.hipDeviceSynchronize() == 0
                assert np.array_equal(_fetch_int(H, dQ, q.shape), q) and np.array_equal(dev.fetch(dN, nll.shape), nll), (qs, skip)
                t2, s2 = dev.fetch(dT, theta.shape), _fetch_int(H, dS, st.shape)
                assert np.all(np.isnan(t2)) if skip == "theta" else np.array_equal(t2, theta), (qs, skip)
                assert np.all(s2 == -1) if skip == "status" else np.array_equal(s2, st), (qs, skip)
    plan.close()


# --- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(nusi):  # noqa: F811
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    C, K, P = 5, 2, 3
    R, D, B = _folded(nusi, C)
    S = _spectra(M, 2)
    data = np.ones((P, C))
    T = _templates(C, K)
    plan = _plan(nusi, "G6")

    def refused(code, f, *a, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*a, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    refused(_lib.NUSI_ESTATE, plan.ensemble, np.ones((1, M, C)), S, data)                  # no detector
    ens = L.nusi_plan_response_ensemble
    assert ens(plan._h, None, 1, Sp, 2, datap, P, None, None, None, None, None) == _lib.NUSI_ESTATE
    plan.set_detector(D, background=B)
    want_profile = plan.profile(R, S, data[0])
    want0 = plan.ensemble(R, S, data)                                                       # K = 0: the profile's iteration
    assert want0[2].shape == (P, 3, 1)
    plan.set_templates(T)
    want_fit = plan.fit(R, S, data[0])
    want = plan.ensemble(R, S, data)
    for bad in (-1.0, np.nan, np.inf):
        db, Sb = data.copy(), np.array(S)
        db[P - 1, C - 1] = bad                                                              # (in the last data row)
        Sb[1, M - 1] = bad
        refused(_lib.NUSI_EPARAM, plan.ensemble, R, S, db)
        refused(_lib.NUSI_EPARAM, plan.ensemble, R, Sb, data)
    with pytest.raises(ValueError):
        plan.ensemble(R[:, :-1], S, data)
    with pytest.raises(ValueError):
        plan.ensemble(R, S, data[:, :-1])
    with pytest.raises(ValueError):
        plan.ensemble(R, S, data[:0])
    for opt in (_lib.OPT_ENSEMBLE_QSLICES, _lib.OPT_ENSEMBLE_PSLICES):
        refused(_lib.NUSI_EPARAM, plan.set_option, opt, -1)
        refused(_lib.NUSI_EPARAM, plan.set_option, opt, 65536)
    H = _hip()
    with _Dev(H) as dev:
        dR, dQ, dN = dev.alloc(R.nbytes, np.ascontiguousarray(R)), dev.alloc(P * 3 * 4), dev.alloc(P * 3 * 8)
        E = _lib.NUSI_EPARAM
        assert ens(plan._h, None, 3, Sp, 2, datap, P, dQ, dN, None, None, None) == E       # NULL d_R
        assert ens(plan._h, dR, 3, None, 2, datap, P, dQ, dN, None, None, None) == E       # NULL S
        assert ens(plan._h, dR, 3, Sp, 2, None, P, dQ, dN, None, None, None) == E          # NULL data
        assert ens(plan._h, dR, 3, Sp, 2, datap, P, None, dN, None, None, None) == E       # NULL d_q
        assert ens(plan._h, dR, 3, Sp, 2, datap, P, dQ, None, None, None, None) == E       # NULL d_nll
        assert ens(plan._h, dR, 3, Sp, 2, datap, 0, dQ, dN, None, None, None) == E         # P outside 1 .. the maximum
        assert ens(plan._h, dR, 3, Sp, 2, datap, _lib.ENSEMBLE_DATASETS_MAX + 1, dQ, dN, None, None, None) == E
        assert ens(plan._h, dR, 0, Sp, 2, datap, P, dQ, dN, None, None, None) == E
        assert ens(plan._h, dR, 3, Sp, 0, datap, P, dQ, dN, None, None, None) == E
        assert ens(plan._h, dR, 3, Sp, (1 << 19) + 1, datap, P, dQ, dN, None, None, None) == E
    # the refusals changed nothing: the ensemble, the fit and the profile return what they did
    _same(plan.ensemble(R, S, data), want, "after the refusals")
    for x, y in zip(plan.fit(R, S, data[0]), want_fit):
        assert np.array_equal(x, y)
    for x, y in zip(plan.profile(R, S, data[0]), want_profile):
        assert np.array_equal(x, y)
    plan.set_templates(None)
    _same(plan.ensemble(R, S, data), want0, "without templates again")
    plan.close()
