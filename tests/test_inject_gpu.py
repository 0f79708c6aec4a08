"""The calibration call on the GPU: k_inject<NC> and k_toys_band (nusi_plan_response_inject).

  * the toys: data_all[t] equals plan.draw of mu_inj[t] with stream = t, every integer; mu_inj is formed here on the host
    from plan.events' accumulator in the defined order;
  * through EXISTING device code, on every toy of two spectra and every spectrum of two toys (of two tables): theta_hat
    and word [0] are the bits of plan.fit (plan.profile without templates) against data_all[t, q, p], word [1] is
    plan.fit_fixed's, and stat is within 2 (bound_cond + bound_hat) + 2 eps_lambda of 2 (nll_fixed - nll_hat) from those
    calls -- tests/test_limit_gpu.py's bounds for the same comparison: bound = 2 (C + 3 + 3 K) u (sum_c (mu_c +
    |d_c log mu_c|) + penalties), eps_lambda = kappa_lambda(C, K) u times lambda's magnitude;
  * against detector.inject_host with the oracle's exp and log (table 0, two spectra, the first toys): the same toys,
    theta_hat and flags, stat within 2 eps_lambda;
  * bands, tally and exceed from the raw arrays to the bit; then every shape again without raw arrays under a budget of at
    least three chunks with a partial last one, with two p-slices, and with both: the same bits.

Shapes as for the ensemble limit: C = 1, 5, 17, 64; K = 0, 1, 3; Q = 1, 5, 19; P = 1, 3, 37; five tables; Q = 600 at C = 1.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from nusiprop_amd.detector import FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_NOT_CONVERGED, FIT_SINGULAR
from tests.test_detector_gpu import (GRIDS, MAXIS, _Dev, _folded, _hip, _ora_log, _spectra, nusi)  # noqa: F401  (nusi: the fixture)
from tests.test_ensemble_limit_gpu import _chunk_budget, _five, _prior_for, _ranks, _setup
from tests.test_fit_gpu import _templates
from tests.test_limit_gpu import _mag
from tests.test_profile_gpu import _fetch_int

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
U = 2.0 ** -53
SEED = 0x9E3779B97F4A7C15
FAIL = FIT_NOT_CONVERGED | FIT_SINGULAR
NAMES = ("band_theta", "band_stat", "tally", "exceed", "theta_all", "stat_all", "words_all", "data_all")


def _ora(oracle_mod):
    L = oracle_mod.lib()
    L.ora_exp.restype, L.ora_exp.argtypes = ctypes.c_double, [ctypes.c_double]
    return L.ora_exp, _ora_log(oracle_mod)


def _same(a, b, what, names=NAMES):
    assert len(a) == len(b), (what, len(a), len(b))
    for x, y, name in zip(a, b, names):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x, y, equal_nan=True), (what, name, np.argwhere(~((x == y) | ((x != x) & (y != y))))[:4])


def _case(nusi, C, K, Q):  # noqa: F811
    """(plan, R (5 tables), S, T, prior, B, acc, a_inj, th_inj): per spectrum 0, 50 or 100 signal events in table 0's
    fullest bin (a_inj = 0: background-only toys; the spectrum of zeros keeps a_inj > 0)."""
    R3, D, B = _folded(nusi, C)
    R, S = _five(R3), _spectra(M, Q)
    if Q > 2:
        S[2] = 0.0                                                  # a spectrum of zeros
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    prior = _prior_for(T, C)
    plan = _setup(nusi, D, None)
    acc = plan.events(R, S)                                         # no background: the accumulator itself
    plan.set_detector(D, background=B)
    if K:
        plan.set_templates(T, prior=prior)
    peak = acc[0].max(axis=-1)
    a_inj = np.where(peak > 0, 50.0 * (np.arange(Q) % 3) / np.where(peak > 0, peak, 1.0), 1.0)
    return plan, R, S, T, prior, B, acc, a_inj, np.array([1.1, 0.9, 1.3])[:K]


def _mu_inj(acc, a_inj, th_inj, T, B):
    mu = a_inj[None, :, None] * acc
    for j in range(len(T)):
        mu = mu + th_inj[j] * T[j][None, None, :]
    return mu + B[None, None, :]


def _from_raw(raw, ranks, q_obs, P):
    th_all, st_all, words = raw[:3]
    with np.errstate(invalid="ignore"):
        exceed = (st_all >= q_obs[..., None]).sum(-1).astype(np.int32)
    return detector.order_stat(th_all, ranks), detector.order_stat(st_all, ranks), detector.inject_tally(words), exceed


def _through_device_calls(plan, R, S, T, prior, B, a_test, out, what):
    """The second check of the module docstring on a subset of (t, q, p)."""
    th_all, st_all, words, data = out[4:]
    ntab, Q, P, C = data.shape
    K = len(T)
    m, w = detector._prior(K, prior)
    pairs = sorted({(q, p) for q in {0, Q - 1} for p in range(P)} | {(q, p) for q in range(Q) for p in {0, P - 1}})
    worst = 0.0
    for t in sorted({0, ntab - 2}):
        R1 = R[t:t + 1]
        for q, p in pairs:
            d, S1 = data[t, q, p], S[q:q + 1]
            if K:
                thh, nh, muh, sth = (x[0, 0] for x in plan.fit(R1, S1, d))
                thc, nc, muc, stc = (x[0, 0] for x in plan.fit_fixed(R1, S1, a_test[q], d))
            else:
                ah, nh, muh, sth = (x[0, 0] for x in plan.profile(R1, S1, d))
                thh, thc, stc = np.array([ah]), np.array([a_test[q]]), 0
                muc, nc = (x[0, 0] for x in plan.events(R1, S1, scale=a_test[q], data=d))
            assert words[t, q, p, 0] == sth and words[t, q, p, 1] == stc, (what, t, q, p, hex(words[t, q, p, 0]), hex(sth), hex(words[t, q, p, 1]), hex(stc))
            if sth & FAIL:
                assert np.isnan(th_all[t, q, p]) and np.isnan(st_all[t, q, p]), (what, t, q, p)
                continue
            assert th_all[t, q, p] == thh[0] and not np.signbit(th_all[t, q, p]), (what, t, q, p, th_all[t, q, p], thh[0])
            if stc & FAIL:
                assert np.isnan(st_all[t, q, p]), (what, t, q, p)
                continue
            stat = st_all[t, q, p]
            assert stat >= 0 and not np.signbit(stat), (what, t, q, p, stat)
            if not (np.isfinite(nh) and np.isfinite(nc)):
                continue
            with np.errstate(all="ignore"):
                _, mg = detector._limit_lambda(a_test[q], thc[1:], muc, muh, thh[1:], (d > 0) & (muh > 0), d, m[1:], w[1:], np.log)
            allow = 2.0 * (2 * (C + 3 + 3 * K) * U * (_mag(muc, d, thc, m, w) + _mag(muh, d, thh, m, w))) + 2.0 * detector.limit_kappa(C, K) * U * mg
            err = abs(stat - 2.0 * (nc - nh))
            assert err <= allow, (what, t, q, p, stat, 2.0 * (nc - nh), allow)
            worst = max(worst, err / allow if allow > 0 else 0.0)
    print("%s: %d records through the existing calls, |stat - 2 (nll_fixed - nll_hat)| / allowance max %.3f" % (what, 2 * len(pairs), worst))


def _against_host_form(R, S, T, prior, B, a_inj, th_inj, a_test, P, out, exp, log, what):
    th_all, st_all, words, data = out[4:]
    K, C, nq, np_ = len(T), R.shape[2], min(len(S), 2), min(P, 4)
    m, w = detector._prior(K, prior)
    h = detector.inject_host(R[0], S[:nq], a_inj[:nq], np_, SEED, theta_inj=th_inj, a_test=a_test[:nq], ranks=[0],
                             templates=T if K else None, prior=prior, background=B, exp=exp, log=log, raw=True)
    hth, hst, hwords, hdata = h[3:]
    assert np.array_equal(hdata[0], data[0, :nq, :np_]), what
    assert np.array_equal(hth[0], th_all[0, :nq, :np_], equal_nan=True), what
    flags = ~(detector.FIT_STEPS_MASK | (detector.FIT_TRIALS_MASK << detector.FIT_TRIALS_SHIFT))
    assert np.array_equal(hwords[0] & flags, words[0, :nq, :np_] & flags), what
    assert np.array_equal(np.isnan(hst[0]), np.isnan(st_all[0, :nq, :np_])), what
    for q in range(nq):
        for p in range(np_):
            a, b = hst[0, q, p], st_all[0, q, p]
            if np.isnan(a) or a == b:
                continue
            d = data[0, q, p]
            if K:
                thh, _, muh, _ = detector.fit_host(R[0], S[q], d, T, prior=prior, background=B, log=log)
                thc, _, muc, _ = detector.fit_fixed_host(R[0], S[q], a_test[q], d, T, prior=prior, background=B, log=log)
            else:
                ah, _, muh, _ = detector.profile_host(R[0], S[q], d, background=B, log=log)
                thh, thc = np.array([ah]), np.array([a_test[q]])
                muc = detector.events_host(R[0], S[q], scale=a_test[q], background=B)
            with np.errstate(all="ignore"):
                _, mg = detector._limit_lambda(a_test[q], thc[1:], muc, muh, thh[1:], (d > 0) & (muh > 0), d, m[1:], w[1:], np.log)
            assert abs(a - b) <= 2.0 * detector.limit_kappa(C, K) * U * mg, (what, q, p, a, b)
    print("%s: %d of %d statistics equal the host form's to the bit" % (
        what, int(np.sum((hst[0] == st_all[0, :nq, :np_]) | np.isnan(hst[0]))), nq * np_))


@pytest.mark.parametrize("P", (1, 3, 37))
@pytest.mark.parametrize("Q", (1, 5, 19))
@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_inject_on_the_real_fold(nusi, oracle_mod, C, K, Q, P):  # noqa: F811
    exp, log = _ora(oracle_mod)
    what = "G6 C=%d K=%d Q=%d P=%d" % (C, K, Q, P)
    plan, R, S, T, prior, B, acc, a_inj, th_inj = _case(nusi, C, K, Q)
    try:
        ntab, ranks = R.shape[0], _ranks(P)
        q_obs = np.broadcast_to(np.array([0.0, 0.5, 2.706, np.nan, 1e3])[:, None], (ntab, Q)).copy()
        kw = dict(theta_inj=th_inj if K else None, ranks=ranks, q_obs=q_obs)
        base = plan.inject(R, S, a_inj, P, SEED, raw=True, **kw)
        assert len(base) == 8 and base[2].dtype == base[3].dtype == base[6].dtype == np.int32
        data = base[7]
        # the toys are plan.draw's
        mu = _mu_inj(acc, a_inj, th_inj, T, B)
        for t in range(ntab):
            assert np.array_equal(data[t], plan.draw(mu[t], P, SEED, stream=t)), (what, t)
        if data[0].size >= 64:
            assert np.array_equal(mu[0], mu[4]) and not np.array_equal(data[0], data[4]), what   # the table enters the identity
        _through_device_calls(plan, R, S, T, prior, B, a_inj, base, what)
        _against_host_form(R, S, T, prior, B, a_inj, th_inj, a_inj, P, base, exp, log, what)
        _same(base[:4], _from_raw(base[4:], ranks, q_obs, P), what + ": bands, tally and exceed from the raw arrays", NAMES[:4])
        assert np.array_equal(np.isnan(base[5]).sum(-1), base[2][..., 0] + base[2][..., 1]), what
        # every budget and slicing: the same bits, without the raw arrays (the series then live in the plan's scratch)
        budget = _chunk_budget(ntab, Q, C, P, 2)
        for nbytes, ps in ((0, 0), (budget, 0), (0, 2), (budget, 2)):
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
            plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, ps)
            _same(plan.inject(R, S, a_inj, P, SEED, **kw), base[:4], "%s: no raw arrays, budget %d, p-slices %d" % (what, nbytes, ps))
            if ps:
                _same(plan.inject(R, S, a_inj, P, SEED, raw=True, **kw), base, "%s: raw arrays, p-slices %d" % (what, ps))
    finally:
        plan.close()


@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_modes_and_a_test(nusi, C, K):  # noqa: F811
    """The three conventions differ only where they say so; a_test given, and a_test = 0 under an injected signal."""
    Q, P = 5, 9
    what = "modes C=%d K=%d" % (C, K)
    plan, R, S, T, prior, B, acc, a_inj, th_inj = _case(nusi, C, K, Q)
    try:
        peak = acc[0].max(axis=-1)                                  # 50, 100 or 150 signal events: a_inj > 0 everywhere
        a_inj = np.where(peak > 0, 50.0 * (1 + np.arange(Q) % 3) / np.where(peak > 0, peak, 1.0), 1.0)
        for a_test in (0.0, 0.5 * a_inj, 2.0 * a_inj):
            at = np.broadcast_to(np.asarray(a_test, dtype=np.float64), (Q,))
            kw = dict(theta_inj=th_inj if K else None, a_test=a_test, ranks=[0, P // 2, P - 1], raw=True)
            two = plan.inject(R, S, a_inj, P, SEED, mode="two-sided", **kw)
            up = plan.inject(R, S, a_inj, P, SEED, mode="upper", **kw)
            dis = plan.inject(R, S, a_inj, P, SEED, mode=_lib.INJECT_DISCOVERY, **kw)
            th, st = two[3], two[4]
            for other in (up, dis):
                for k in (0, 2, 3, 5, 6):                           # all but the statistic and its band
                    assert np.array_equal(other[k], two[k], equal_nan=True), (what, k)
            above, below = th > at[None, :, None], th < at[None, :, None]
            num = ~np.isnan(st)                                     # (a failed fit stays NaN under every convention)
            assert np.array_equal(up[4], np.where(above & num, 0.0, st), equal_nan=True), what
            assert np.array_equal(dis[4], np.where(below & num, 0.0, st), equal_nan=True), what
            assert np.array_equal(up[1], detector.order_stat(up[4], [0, P // 2, P - 1]), equal_nan=True), what
            if np.ndim(a_test) == 0:
                assert not below.any() and np.array_equal(dis[4], st, equal_nan=True)       # nothing is below zero
                live = [q for q in range(Q) if q != 2]
                assert np.nanmedian(st[:, live]) > 1.0, what        # an injected signal is seen against a_test = 0
            _through_device_calls(plan, R, S, T, prior, B, at, (None,) * 4 + two[3:], what + " a_test %s" % ("0" if np.ndim(a_test) == 0 else "given"))
    finally:
        plan.close()


def test_many_spectra_on_one_bin(nusi):  # noqa: F811
    """Q = 600 at C = 1: 256 chains a block, a partial last block, several units a table."""
    C, Q, P = 1, 600, 3
    for K in (0, 1):
        plan, R, S, T, prior, B, acc, a_inj, th_inj = _case(nusi, C, K, Q)
        try:
            kw = dict(theta_inj=th_inj if K else None, ranks=[0, 1, 2], q_obs=1.0)
            base = plan.inject(R, S, a_inj, P, SEED, raw=True, **kw)
            mu = _mu_inj(acc, a_inj, th_inj, T, B)
            for t in (0, 3):
                assert np.array_equal(base[7][t], plan.draw(mu[t], P, SEED, stream=t))
            q_obs = np.full((R.shape[0], Q), 1.0)
            _same(base[:4], _from_raw(base[4:], [0, 1, 2], q_obs, P), "Q=600 K=%d from the raw arrays" % K, NAMES[:4])
            for q in (0, 255, 256, 599):                            # either side of a block's edge, through the existing calls
                for t in (0, 4):
                    d = base[7][t, q, 1]
                    if K:
                        thh, _, _, sth = (x[0, 0] for x in plan.fit(R[t:t + 1], S[q:q + 1], d))
                        _, _, _, stc = (x[0, 0] for x in plan.fit_fixed(R[t:t + 1], S[q:q + 1], a_inj[q], d))
                    else:
                        ah, _, _, sth = (x[0, 0] for x in plan.profile(R[t:t + 1], S[q:q + 1], d))
                        thh, stc = [ah], 0
                    assert tuple(base[6][t, q, 1]) == (sth, stc) and (base[4][t, q, 1] == thh[0] or sth & FAIL)
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, _chunk_budget(R.shape[0], Q, C, P, 2))
            plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, 2)
            _same(plan.inject(R, S, a_inj, P, SEED, **kw), base[:4], "Q=600 K=%d chunks and slices" % K)
        finally:
            plan.close()


def test_the_device_form_and_refusals(nusi):  # noqa: F811
    C, K, Q, P = 17, 3, 19, 5
    plan, R, S, T, prior, B, acc, a_inj, th_inj = _case(nusi, C, K, Q)
    H = _hip()
    try:
        ntab, ranks = R.shape[0], [0, 2, 4]
        q_obs = np.full((ntab, Q), 0.7)
        base = plan.inject(R, S, a_inj, P, SEED, theta_inj=th_inj, ranks=ranks, q_obs=q_obs, raw=True)
        ints = (2, 3, 6)
        with _Dev(H) as dev:
            dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
            for skip in (None,) + NAMES:
                bufs = []
                for k, x in enumerate(base):
                    fill = np.full(x.shape, -1, dtype=np.int32) if k in ints else np.full(x.shape, np.nan)
                    bufs.append(dev.alloc(fill.nbytes, fill))
                args = [None if NAMES[k] == skip else bufs[k] for k in range(8)]
                assert plan.inject_device(dR, ntab, S, a_inj, P, SEED, theta_inj=th_inj, ranks=ranks,
                                          q_obs=None if skip == "exceed" else q_obs, d_band_theta_ptr=args[0], d_band_stat_ptr=args[1],
                                          d_tally_ptr=args[2], d_exceed_ptr=args[3], d_theta_all_ptr=args[4], d_stat_all_ptr=args[5],
                                          d_words_all_ptr=args[6], d_data_all_ptr=args[7]) == (Q, 3)
                assert H.hipDeviceSynchronize() == 0
                for k, x in enumerate(base):
                    got = _fetch_int(H, bufs[k], x.shape) if k in ints else dev.fetch(bufs[k], x.shape)
                    if NAMES[k] == skip:
                        assert np.all(got == -1) if k in ints else np.all(np.isnan(got)), (skip, NAMES[k])
                    else:
                        assert np.array_equal(got, x, equal_nan=True), (skip, NAMES[k])
            # one band alone and no raw arrays: its series is the only one in the plan's scratch, whole and in chunks
            for k in (0, 1):
                for nbytes in (0, _chunk_budget(ntab, Q, C, P, 1)):
                    plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
                    nan = np.full(base[k].shape, np.nan)
                    dOne, dOther = dev.alloc(nan.nbytes, nan), dev.alloc(nan.nbytes, nan)
                    assert plan.inject_device(dR, ntab, S, a_inj, P, SEED, theta_inj=th_inj, ranks=ranks,
                                              d_band_theta_ptr=dOne if k == 0 else None,
                                              d_band_stat_ptr=dOne if k == 1 else None) == (Q, 3)
                    assert H.hipDeviceSynchronize() == 0
                    assert np.array_equal(dev.fetch(dOne, nan.shape), base[k], equal_nan=True), (NAMES[k], nbytes)
                    assert np.all(np.isnan(dev.fetch(dOther, nan.shape)))
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
            # no band at all: NR = 0, the tally alone
            dT = dev.alloc(base[2].nbytes, np.full(base[2].shape, -1, dtype=np.int32))
            assert plan.inject_device(dR, ntab, S, a_inj, P, SEED, theta_inj=th_inj, ranks=[], d_tally_ptr=dT) == (Q, 0)
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(_fetch_int(H, dT, base[2].shape), base[2])
            # refusals change nothing: neither this call's outputs nor what limit and ensemble_limit return
            data = base[7][0, 1]
            lim = plan.limit(R, S, data[0], 2.706, which="both")
            ens = plan.ensemble_limit(R, S, data, 2.706, which="upper", ranks=ranks)
            dB = dev.alloc(base[1].nbytes, np.full(base[1].shape, np.nan))
            ok = dict(theta_inj=th_inj, ranks=ranks, d_band_stat_ptr=dB)
            bad = [dict(ok, P_=0), dict(ok, P_=_lib.BAND_DATASETS_MAX + 1), dict(ok, ranks=[5]), dict(ok, ranks=[-1]),
                   dict(ok, ranks=list(range(5)) * 4), dict(ok, mode=3), dict(ok, mode=-1), dict(ok, a_inj_=-1.0),
                   dict(ok, a_inj_=np.nan), dict(ok, a_test=np.inf), dict(ok, a_test=-0.5), dict(ok, theta_inj=[1.0, -1.0, 1.0]),
                   dict(ok, theta_inj=[1.0, np.nan, 1.0]), dict(ok, q_obs=q_obs), dict(ok, d_exceed_ptr=dT),
                   dict(theta_inj=th_inj, ranks=ranks), dict(theta_inj=th_inj, ranks=[])]
            for kw in bad:
                kw = dict(kw)
                Pb, ab = kw.pop("P_", P), kw.pop("a_inj_", a_inj)
                with pytest.raises(_lib.NusiError) as e:
                    plan.inject_device(dR, ntab, S, ab, Pb, SEED, **kw)
                assert e.value.code == _lib.NUSI_EPARAM, kw
            with pytest.raises(_lib.NusiError) as e:
                plan.inject_device(0, ntab, S, a_inj, P, SEED, **ok)
            assert e.value.code == _lib.NUSI_EPARAM
            Sbad = S.copy()
            Sbad[0, 3] = -1.0
            with pytest.raises(_lib.NusiError):
                plan.inject_device(dR, ntab, Sbad, a_inj, P, SEED, **ok)
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 8 * P * 8 - 1)      # one byte short of a unit (QB = 8 at C = 17)
            with pytest.raises(_lib.NusiError) as e:
                plan.inject_device(dR, ntab, S, a_inj, P, SEED, **ok)
            assert e.value.code == _lib.NUSI_EPARAM and "NUSI_OPT_ENSEMBLE_LIMIT" in _lib.last_error()
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
            assert H.hipDeviceSynchronize() == 0
            assert np.all(np.isnan(dev.fetch(dB, base[1].shape)))
            for x, y in zip(plan.limit(R, S, data[0], 2.706, which="both"), lim):
                assert np.array_equal(x, y, equal_nan=True)
            for x, y in zip(plan.ensemble_limit(R, S, data, 2.706, which="upper", ranks=ranks), ens):
                assert np.array_equal(x, y, equal_nan=True)
            _same(plan.inject(R, S, a_inj, P, SEED, theta_inj=th_inj, ranks=ranks, q_obs=q_obs, raw=True), base, "after the refusals")
        plan.set_detector(None)
        with pytest.raises(_lib.NusiError) as e:
            plan.inject(R, S, a_inj, P, SEED)
        assert e.value.code == _lib.NUSI_ESTATE
    finally:
        plan.close()
