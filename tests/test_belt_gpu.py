"""The toy-calibrated interval on the GPU: k_belt<NC> and k_belt_accept (nusi_plan_response_belt).

On G6's five tables; the data are plan.draw of a background-plus-signal expectation, ref is plan.limit's upper limit at
delta = 2.706 per (t, q) (a spectrum of zeros gives an unbounded one: BELT_NO_GRID for free), frac = (0, 0.5, 1, 2).

  * the observed side through EXISTING device code: theta_obs[.., 0] and words_obs[.., 0] are the bits of plan.fit
    (plan.profile at K = 0) against the data, [.., 1 + g] plan.fit_fixed's at a[t, q, g], and q_obs is within
    tests/test_inject_gpu.py's allowance of 2 (nll_fixed - nll_hat) from those calls;
  * the toys through plan.inject on the spectrum list repeated G times (entry q G + g = S[q]) with a_inj = a_test = a and
    theta_inj the observed conditional fit's: data_all, theta_all, stat_all, words_all, tally, and exceed against the
    belt's q_obs, to the bit -- at K = 0 one call a table covers every record, at K > 0 two tables x q in {0, Q - 1} x
    every g;
  * against detector.belt_host with the oracle's exp and log (table 0, two spectra, the first toys): the same toys,
    theta_hat and flags; q_obs and stat within 2 limit_kappa(C, K) u times lambda's magnitude;
  * exceed and tally from the call's own raw arrays and q_obs to the bit; lo, hi, idx, status equal detector.belt_accept
    with valid and flags rebuilt from words_obs as belt_host does;
  * every shape again without raw arrays: under a budget of at least three chunks with a partial last one (the interval
    alone, so exceed, tally and words_obs live in the plan's scratch), with two p-slices, and with both: the same bits.

No call here passes a size other than its arrays' own: the size limits are tests/test_belt_abi.py's, on the CPU, through
nusi_belt_shape.  The device form and the refusals are a test function of their own at the end.
"""
import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from nusiprop_amd.detector import (BELT_BAD_POINT, BELT_EMPTY, BELT_LO_EDGE, BELT_NO_FIT, BELT_NO_GRID, FIT_NOT_CONVERGED,
                                   FIT_SINGULAR)
from tests.test_detector_gpu import nusi  # noqa: F401  (the fixture)
from tests.test_inject_gpu import SEED, _case, _Dev, _fetch_int, _hip, _ora, _same
from tests.test_limit_gpu import _mag

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FAIL = FIT_NOT_CONVERGED | FIT_SINGULAR
NAMES = ("lo", "hi", "idx", "status", "exceed", "tally", "q_obs", "theta_obs", "words_obs", "theta_all", "stat_all",
         "words_all", "data_all")
INTS = (2, 3, 4, 5, 8, 11)
FRAC = {1: np.array([1.0]), 3: np.array([0.0, 1.0, 2.0]), 4: np.array([0.0, 0.5, 1.0, 2.0]), 64: np.linspace(0.0, 3.0, 64)}
ALPHA = 0.1


def _setting(nusi, C, K, Q):  # noqa: F811
    """(plan, R, S, T, prior, B, data, ref): _case's plan; the data drawn around 30 signal events of spectrum 0 in table
    0's fullest bin on the templates at 1 and the background; ref the upper limits at delta = 2.706."""
    plan, R, S, T, prior, B, acc, _, _ = _case(nusi, C, K, Q)
    peak = acc[0, 0].max()
    mu = (30.0 / peak if peak > 0 else 0.0) * acc[0, 0]
    for j in range(K):
        mu = mu + T[j]
    data = plan.draw(mu + B, 1, SEED + 1)[0]
    ref = plan.limit(R, S, data, 2.706)[1]
    return plan, R, S, T, prior, B, data, ref


def _grid(frac, ref):
    with np.errstate(invalid="ignore"):
        a = frac[None, None, :] * ref[:, :, None]
        agood = (ref >= 0)[:, :, None] & (a < np.inf)
    return a, agood


def _valid_flags(words_obs, agood):
    """valid (ntab, Q, G) and the observed side's flags (ntab, Q), as belt_host forms them."""
    nofit = (words_obs[..., 0] & FAIL) != 0
    nocond = (words_obs[..., 1:] & FAIL) != 0
    flags = np.where(nofit, BELT_NO_FIT, 0) | np.where((~agood).any(-1), BELT_NO_GRID, 0)
    flags |= np.where((agood & ~nofit[..., None] & nocond).any(-1), BELT_BAD_POINT, 0)
    return agood & ~nofit[..., None] & ~nocond, flags.astype(np.int32)


def _observed_through_device_calls(plan, R, S, T, prior, data, a, agood, mode, out, what):
    q_obs, th_obs, w_obs = out[6:9]
    ntab, Q, G = a.shape
    K, C = len(T), R.shape[2]
    m, w = detector._prior(K, prior)
    if K:
        thh, nh, muh, sth = plan.fit(R, S, data)
    else:
        ah, nh, muh, sth = plan.profile(R, S, data)
        thh = ah[..., None]
    assert np.array_equal(th_obs[:, :, 0], thh, equal_nan=True) and np.array_equal(w_obs[:, :, 0], sth), what
    worst, n = 0.0, 0
    for t in range(ntab):
        for g in range(G):
            at = np.where(agood[t, :, g], a[t, :, g], 0.0)
            if K:
                thc, nc, muc, stc = (x[0] for x in plan.fit_fixed(R[t:t + 1], S, at, data))
            else:
                muc, nc = (x[0] for x in plan.events(R[t:t + 1], S, scale=at, data=data))
                thc, stc = at[:, None], np.zeros(Q, dtype=np.int32)
            for q in range(Q):
                if not agood[t, q, g]:
                    assert np.all(np.isnan(th_obs[t, q, 1 + g])) and w_obs[t, q, 1 + g] == 0 and np.isnan(q_obs[t, q, g]), (what, t, q, g)
                    continue
                assert np.array_equal(th_obs[t, q, 1 + g], thc[q]) and w_obs[t, q, 1 + g] == stc[q], (what, t, q, g)
                if (sth[t, q] | stc[q]) & FAIL:
                    assert np.isnan(q_obs[t, q, g]), (what, t, q, g)
                    continue
                stat = q_obs[t, q, g]
                assert stat >= 0 and not np.signbit(stat), (what, t, q, g, stat)
                if mode == "upper" and thh[t, q, 0] > a[t, q, g]:
                    assert stat == 0.0, (what, t, q, g, stat)
                    continue
                if not (np.isfinite(nh[t, q]) and np.isfinite(nc[q])):
                    continue
                with np.errstate(all="ignore"):
                    _, mg = detector._limit_lambda(at[q], thc[q, 1:], muc[q], muh[t, q], thh[t, q, 1:],
                                                   (data > 0) & (muh[t, q] > 0), data, m[1:], w[1:], np.log)
                allow = 2.0 * (2 * (C + 3 + 3 * K) * U * (_mag(muc[q], data, thc[q], m, w) + _mag(muh[t, q], data, thh[t, q], m, w))) \
                    + 2.0 * detector.limit_kappa(C, K) * U * mg
                err = abs(stat - 2.0 * (nc[q] - nh[t, q]))
                assert err <= allow, (what, t, q, g, stat, 2.0 * (nc[q] - nh[t, q]), allow)
                worst, n = max(worst, err / allow if allow > 0 else 0.0), n + 1
    print("%s: %d observed records through the existing calls, |q_obs - 2 (nll_fixed - nll_hat)| / allowance max %.3f" % (what, n, worst))


def _toys_through_inject(plan, R, S, K, a, valid, P, mode, out, what):
    exceed, tally, q_obs, th_obs = out[4:8]
    th_all, st_all, words, toys = out[9:]
    ntab, Q, G = a.shape
    Srep = np.repeat(S, G, axis=0)                                  # entry q G + g = S[q]
    qo = q_obs.reshape(ntab, Q * G)
    if K == 0:
        calls = [(t, None, [(q, g) for q in range(Q) for g in range(G)]) for t in range(ntab)]
    else:
        calls = [(t, th_obs[t, q, 1 + g, 1:], [(q, g)]) for t in sorted({0, ntab - 2}) for q in sorted({0, Q - 1})
                 for g in range(G) if valid[t, q, g]]
    n = 0
    for t, th_inj, records in calls:
        at = np.where(valid[t], a[t], 0.0).reshape(-1)
        inj = plan.inject(R, Srep, at, P, SEED, theta_inj=th_inj, a_test=at, mode=mode, ranks=[], q_obs=qo, raw=True)
        ity, iex, ith, ist, iw, idata = inj[2:]
        for q, g in records:
            if not valid[t, q, g]:
                continue
            r = q * G + g
            for x, y, name in ((toys[t, q, g], idata[t, r], "data_all"), (th_all[t, q, g], ith[t, r], "theta_all"),
                               (st_all[t, q, g], ist[t, r], "stat_all"), (words[t, q, g], iw[t, r], "words_all"),
                               (tally[t, q, g], ity[t, r], "tally"), (exceed[t, q, g], iex[t, r], "exceed")):
                assert np.array_equal(x, y, equal_nan=True), (what, name, t, q, g)
            n += 1
    print("%s: %d records' toys equal plan.inject's to the bit" % (what, n))


def _against_host_form(R, S, T, prior, B, data, frac, ref, P, mode, out, exp, log, what):
    K, C, nq, np_ = len(T), R.shape[2], min(len(S), 2), min(P, 4)
    m, w = detector._prior(K, prior)
    h = detector.belt_host(R[0], S[:nq], data, frac, np_, SEED, ref=ref[0:1, :nq], mode=mode, alpha=ALPHA,
                           templates=T if K else None, prior=prior, background=B, exp=exp, log=log, raw=True)
    flags = ~(detector.FIT_STEPS_MASK | (detector.FIT_TRIALS_MASK << detector.FIT_TRIALS_SHIFT))
    a, _ = _grid(frac, ref)
    got = [x[0:1, :nq] for x in out]
    got[9], got[10], got[11], got[12] = (x[:, :, :, :np_] for x in got[9:])
    assert np.array_equal(h[12], got[12]), what                       # the toys
    assert np.array_equal(h[7], got[7], equal_nan=True), what         # theta_obs
    assert np.array_equal(h[9], got[9], equal_nan=True), what         # theta_hat_0 of every toy
    assert np.array_equal(h[8] & flags, got[8] & flags) and np.array_equal(h[11] & flags, got[11] & flags), what
    same = total = 0
    for hx, gx, toy in ((h[6], got[6], False), (h[10], got[10], True)):
        assert np.array_equal(np.isnan(hx), np.isnan(gx)), what
        for i in zip(*np.nonzero(~np.isnan(hx))):
            total += 1
            if hx[i] == gx[i]:
                same += 1
                continue
            q, g = i[1], i[2]
            d = got[12][i] if toy else data
            at = float(a[0, q, g])
            mg = detector._inject_one(R[0], S[q], at, d, T, prior, B, m, w, detector.INJECT_TWO_SIDED, log)[7]
            assert abs(hx[i] - gx[i]) <= 2.0 * detector.limit_kappa(C, K) * U * mg, (what, i, hx[i], gx[i])
    print("%s: %d of %d statistics (q_obs and stat) equal the host form's to the bit" % (what, same, total))


def _interval_budget(ntab, Q, G):
    """The largest budget in bytes that cuts the call into at least three chunks of whole (t, q) pairs, the last one
    partial, when exceed, tally and words_obs all live in the scratch (include/nusi.h: 4 G + 16 G + 4 (1 + G) bytes a pair)."""
    pairs, per = ntab * Q, 24 * G + 4
    for ppc in range(pairs // 2, 0, -1):
        if (pairs + ppc - 1) // ppc >= 3 and pairs % ppc:
            return ppc * per
    raise AssertionError("no such budget for %d pairs" % pairs)


def _interval_alone(plan, H, dev, dR, ntab, S, data, frac, ref, P, mode):
    """(lo, hi, idx, status) of the device form with no other output: the counts and the words live in the scratch."""
    Q = len(S)
    shapes = ((ntab, Q), (ntab, Q), (ntab, Q, 2), (ntab, Q))
    bufs = [dev.alloc(8 * int(np.prod(s))) for s in shapes]
    assert plan.belt_device(dR, ntab, S, data, frac, P, SEED, ref=ref, mode=mode, alpha=ALPHA, d_lo_ptr=bufs[0],
                            d_hi_ptr=bufs[1], d_idx_ptr=bufs[2], d_status_ptr=bufs[3]) == (Q, len(frac))
    assert H.hipDeviceSynchronize() == 0
    return (dev.fetch(bufs[0], shapes[0]), dev.fetch(bufs[1], shapes[1]), _fetch_int(H, bufs[2], shapes[2]),
            _fetch_int(H, bufs[3], shapes[3]))


def _every_way(nusi, oracle_mod, C, K, Q, G, P, mode):  # noqa: F811
    exp, log = _ora(oracle_mod)
    what = "G6 C=%d K=%d Q=%d G=%d P=%d %s" % (C, K, Q, G, P, mode)
    plan, R, S, T, prior, B, data, ref = _setting(nusi, C, K, Q)
    H = _hip()
    try:
        ntab, frac = R.shape[0], FRAC[G]
        a, agood = _grid(frac, ref)
        base = plan.belt(R, S, data, frac, P, SEED, ref=ref, mode=mode, alpha=ALPHA, raw=True)
        assert len(base) == 13 and all(base[k].dtype == np.int32 for k in INTS)
        assert base[7].shape == (ntab, Q, 1 + G, 1 + K) and base[12].shape == (ntab, Q, G, P, C)
        valid, flags = _valid_flags(base[8], agood)
        assert np.array_equal(np.isnan(base[6]), ~valid), what
        if Q > 2:
            assert np.all(base[3][:, 2] & BELT_NO_GRID) and not valid[:, 2].any(), what   # the spectrum of zeros: no upper limit
        assert valid.any(), what
        # a point without toys: NaN / 0
        for k in (9, 10):
            assert np.all(np.isnan(base[k][~valid])), (what, NAMES[k])
        for k in (4, 5, 11, 12):
            assert not np.any(base[k][~valid]), (what, NAMES[k])
        _observed_through_device_calls(plan, R, S, T, prior, data, a, agood, mode, base, what)
        _toys_through_inject(plan, R, S, K, a, valid, P, mode, base, what)
        _against_host_form(R, S, T, prior, B, data, frac, ref, P, mode, base, exp, log, what)
        # the counts from the raw arrays, the interval from the counts
        with np.errstate(invalid="ignore"):
            exceed = (base[10] >= base[6][..., None]).sum(-1).astype(np.int32)
        tally = np.where(valid[..., None], detector.inject_tally(base[11]), 0).astype(np.int32)
        assert np.array_equal(exceed, base[4]) and np.array_equal(tally, base[5]), what
        _same(base[:4], detector.belt_accept(exceed, tally, a, ALPHA, valid, P, flags), what + ": the interval from the counts", NAMES[:4])
        # every budget and slicing: the same bits, without the raw arrays
        budget = _interval_budget(ntab, Q, G)
        with _Dev(H) as dev:
            dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
            for nbytes, ps in ((0, 0), (budget, 0), (0, 2), (budget, 2)):
                plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
                plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, ps)
                tag = "%s: budget %d, p-slices %d" % (what, nbytes, ps)
                _same(plan.belt(R, S, data, frac, P, SEED, ref=ref, mode=mode, alpha=ALPHA), base[:9], tag + ", no raw arrays", NAMES[:9])
                _same(_interval_alone(plan, H, dev, dR, ntab, S, data, frac, ref, P, mode), base[:4], tag + ", the interval alone", NAMES[:4])
                if ps:
                    _same(plan.belt(R, S, data, frac, P, SEED, ref=ref, mode=mode, alpha=ALPHA, raw=True), base, tag + ", raw arrays", NAMES)
    finally:
        plan.close()


@pytest.mark.parametrize("mode", ("two-sided", "upper"))
@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_belt_on_the_real_fold(nusi, oracle_mod, C, K, mode):  # noqa: F811
    _every_way(nusi, oracle_mod, C, K, 5, 4, 3, mode)


@pytest.mark.parametrize("C,K,Q,G,P", [(5, 0, 19, 3, 37), (5, 3, 19, 3, 37), (64, 0, 19, 3, 37), (64, 3, 19, 3, 37),
                                       (17, 1, 1, 1, 1), (1, 0, 100, 3, 2), (1, 1, 100, 3, 2), (5, 1, 2, 64, 2)])
def test_belt_shapes(nusi, oracle_mod, C, K, Q, G, P):  # noqa: F811
    """Several row blocks a table and a partial last one ((19, 3) at C = 64: 57 rows in blocks of 4; (100, 3) at C = 1: 300
    rows, a block's edge inside a table), one record in all, and the widest grid."""
    _every_way(nusi, oracle_mod, C, K, Q, G, P, "two-sided")


def test_a_reference_shared_by_the_tables(nusi):  # noqa: F811
    """ref as (Q,) and as a number are broadcast; at K = 0 one plan.inject call then covers every record of every table."""
    C, K, Q, G, P = 5, 0, 5, 4, 3
    plan, R, S, T, prior, B, data, ref = _setting(nusi, C, K, Q)
    try:
        ntab, frac = R.shape[0], FRAC[G]
        base = plan.belt(R, S, data, frac, P, SEED, ref=ref[0], raw=True)
        _same(plan.belt(R, S, data, frac, P, SEED, ref=np.broadcast_to(ref[0], (ntab, Q)), raw=True), base, "ref (Q,)", NAMES)
        a, agood = _grid(frac, np.broadcast_to(ref[0], (ntab, Q)))
        valid, _ = _valid_flags(base[8], agood)
        at = np.where(valid[0], a[0], 0.0).reshape(-1)
        assert np.array_equal(valid, np.broadcast_to(valid[0], valid.shape))
        inj = plan.inject(R, np.repeat(S, G, axis=0), at, P, SEED, a_test=at, ranks=[], q_obs=base[6].reshape(ntab, Q * G), raw=True)
        v = valid.reshape(ntab, Q * G)
        for k, j in ((5, 2), (4, 3), (9, 4), (10, 5), (11, 6), (12, 7)):
            x = base[k].reshape((ntab, Q * G) + base[k].shape[3:])
            assert np.array_equal(x[v], inj[j][v], equal_nan=True), NAMES[k]
        one = plan.belt(R, S, data, frac, P, SEED, ref=1.0)
        _same(plan.belt(R, S, data, frac, P, SEED), one, "ref None and 1", NAMES[:9])
        assert np.array_equal(one[7][:, :, 1:, 0], np.broadcast_to(frac, (ntab, Q, G)))
    finally:
        plan.close()


def test_a_toy_equal_to_the_data(nusi):  # noqa: F811
    """At C = 1 and K = 0 the toys do not depend on the data (mu_inj = a s + B): with the data set to a toy's own count
    that toy has stat == q_obs to the bit, and counts."""
    C, K, Q, G, P = 1, 0, 5, 4, 3
    plan, R, S, T, prior, B, data, ref = _setting(nusi, C, K, Q)
    try:
        frac = FRAC[G]
        ref = np.where(np.isfinite(ref) & (ref >= 0), ref, 1.0)
        first = plan.belt(R, S, data, frac, P, SEED, ref=ref, raw=True)
        assert not np.isnan(first[6][0, 0, 1])
        dstar = first[12][0, 0, 1, 0]
        again = plan.belt(R, S, dstar, frac, P, SEED, ref=ref, raw=True)
        assert np.array_equal(again[12][0, 0, 1], first[12][0, 0, 1])
        assert again[10][0, 0, 1, 0] == again[6][0, 0, 1] and again[4][0, 0, 1] >= 1
    finally:
        plan.close()


def test_flags_on_the_device(nusi):  # noqa: F811
    C, K, Q, G, P = 5, 1, 5, 4, 3
    plan, R, S, T, prior, B, data, ref = _setting(nusi, C, K, Q)
    try:
        ntab, frac = R.shape[0], FRAC[G]
        fit = plan.fit(R, S, data)
        bad = ref.copy()
        bad[0, 0], bad[1, 1], bad[2, 3] = np.nan, np.inf, -1.0
        out = plan.belt(R, S, data, frac, P, SEED, ref=bad, raw=True)
        for t, q in ((0, 0), (1, 1), (2, 3)):
            assert out[3][t, q] & BELT_NO_GRID and out[3][t, q] & BELT_EMPTY and np.isnan(out[0][t, q]) and np.isnan(out[1][t, q])
            assert tuple(out[2][t, q]) == (-1, -1) and not out[4][t, q].any() and not out[5][t, q].any()
            assert np.all(np.isnan(out[6][t, q])) and np.all(np.isnan(out[9][t, q])) and np.all(np.isnan(out[10][t, q]))
            assert not out[11][t, q].any() and not out[12][t, q].any() and not out[8][t, q, 1:].any()
            assert np.all(np.isnan(out[7][t, q, 1:]))
            assert np.array_equal(out[7][t, q, 0], fit[0][t, q]) and out[8][t, q, 0] == fit[3][t, q]   # the best fit is still returned
        good = plan.belt(R, S, data, frac, P, SEED, ref=ref, raw=True)
        other = np.ones((ntab, Q), dtype=bool)
        other[0, 0] = other[1, 1] = other[2, 3] = False
        for x, y in zip(out, good):
            assert np.array_equal(x[other], y[other], equal_nan=True)
        # data of zeros in upper mode: theta_hat_0 = 0, every q_obs at or above it is what the toys give; frac[0] = 0 is accepted
        zero = plan.belt(R, S, np.zeros(C), frac, 20, SEED, ref=np.where(np.isfinite(ref), ref, 1.0), mode="upper")
        assert np.all(zero[3] & BELT_LO_EDGE) and np.all(zero[2][..., 0] == 0) and np.all(zero[0] == 0.0)
        # two identical templates without priors: a singular best fit
        T2 = np.stack([T[0], T[0]])
        plan.set_templates(T2)
        sing = plan.belt(R, S, data, frac, P, SEED, ref=np.where(np.isfinite(ref), ref, 1.0), raw=True)
        assert np.all(sing[8][:, :, 0] & FAIL) and np.all(sing[3] & BELT_NO_FIT) and np.all(sing[3] & BELT_EMPTY)
        assert np.all(np.isnan(sing[6])) and not sing[4].any() and not sing[5].any() and np.all(np.isnan(sing[10]))
    finally:
        plan.close()


def test_the_device_form_and_refusals(nusi):  # noqa: F811
    """Every size passed here is its array's own (ntab, Q, G, P, C): the refusal cases vary values only, and sizes only
    where an argument check refuses them whatever the other sizes are (P = 0, G = 0, G = 65)."""
    C, K, Q, G, P = 17, 3, 5, 4, 3
    plan, R, S, T, prior, B, data, ref = _setting(nusi, C, K, Q)
    H = _hip()
    try:
        ntab, frac = R.shape[0], FRAC[G]
        kw = dict(ref=ref, mode="two-sided", alpha=ALPHA)
        base = plan.belt(R, S, data, frac, P, SEED, raw=True, **kw)
        keys = ["d_%s_ptr" % n for n in NAMES]
        with _Dev(H) as dev:
            dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
            for skip in (None,) + NAMES:
                bufs = []
                for k, x in enumerate(base):
                    fill = np.full(x.shape, -1, dtype=np.int32) if k in INTS else np.full(x.shape, np.nan)
                    bufs.append(dev.alloc(fill.nbytes, fill))
                args = {keys[k]: None if NAMES[k] == skip else bufs[k] for k in range(13)}
                assert plan.belt_device(dR, ntab, S, data, frac, P, SEED, **kw, **args) == (Q, G)
                assert H.hipDeviceSynchronize() == 0
                for k, x in enumerate(base):
                    got = _fetch_int(H, bufs[k], x.shape) if k in INTS else dev.fetch(bufs[k], x.shape)
                    if NAMES[k] == skip:
                        assert np.all(got == -1) if k in INTS else np.all(np.isnan(got)), (skip, NAMES[k])
                    else:
                        assert np.array_equal(got, x, equal_nan=True), (skip, NAMES[k])
            # the interval alone: the counts and the words in the plan's scratch, whole and in chunks
            for nbytes in (0, _interval_budget(ntab, Q, G)):
                plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
                _same(_interval_alone(plan, H, dev, dR, ntab, S, data, frac, ref, P, "two-sided"), base[:4], "the interval alone, budget %d" % nbytes, NAMES[:4])
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
            # refusals change nothing: neither this call's outputs nor what inject and limit return
            a, agood = _grid(frac, ref)
            at = np.where(agood[0, :, 1], a[0, :, 1], 0.0)
            inj = plan.inject(R, S, at, P, SEED, ranks=[0], raw=True)
            lim = plan.limit(R, S, data, 2.706, which="both")
            dL = dev.alloc(base[0].nbytes, np.full(base[0].shape, np.nan))
            ok = dict(kw, d_lo_ptr=dL)
            neg, nan_, inf_ = data.copy(), data.copy(), data.copy()
            neg[0], nan_[C - 1], inf_[1] = -1.0, np.nan, np.inf
            bad = [dict(ok, alpha=0.0), dict(ok, alpha=1.0), dict(ok, alpha=-0.1), dict(ok, alpha=np.nan), dict(ok, mode="discovery"),
                   dict(ok, mode=3), dict(ok, mode=-1), dict(ok, frac_=[0.0, 0.5, 0.5, 2.0]), dict(ok, frac_=[0.0, 1.0, 0.5, 2.0]),
                   dict(ok, frac_=[-0.5, 0.0, 1.0, 2.0]), dict(ok, frac_=[0.0, 0.5, 1.0, np.inf]), dict(ok, frac_=[0.0, np.nan, 1.0, 2.0]),
                   dict(ok, data_=neg), dict(ok, data_=nan_), dict(ok, data_=inf_), dict(ok, P_=0), dict(ok, frac_=[]),
                   dict(ok, frac_=np.arange(65.0)), dict(kw)]
            for b in bad:
                b = dict(b)
                Pb, fb, db = b.pop("P_", P), b.pop("frac_", frac), b.pop("data_", data)
                with pytest.raises(_lib.NusiError) as e:
                    plan.belt_device(dR, ntab, S, db, fb, Pb, SEED, **b)
                assert e.value.code == _lib.NUSI_EPARAM, b
            with pytest.raises(_lib.NusiError) as e:
                plan.belt_device(0, ntab, S, data, frac, P, SEED, **ok)
            assert e.value.code == _lib.NUSI_EPARAM
            Sbad = S.copy()
            Sbad[0, 3] = -1.0
            with pytest.raises(_lib.NusiError):
                plan.belt_device(dR, ntab, Sbad, data, frac, P, SEED, **ok)
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 24 * G + 4 - 1)      # one byte short of a pair's scratch
            with pytest.raises(_lib.NusiError) as e:
                plan.belt_device(dR, ntab, S, data, frac, P, SEED, **ok)
            assert e.value.code == _lib.NUSI_EPARAM and "NUSI_OPT_ENSEMBLE_LIMIT" in _lib.last_error()
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
            assert H.hipDeviceSynchronize() == 0
            assert np.all(np.isnan(dev.fetch(dL, base[0].shape)))
            for x, y in zip(plan.limit(R, S, data, 2.706, which="both"), lim):
                assert np.array_equal(x, y, equal_nan=True)
            for x, y in zip(plan.inject(R, S, at, P, SEED, ranks=[0], raw=True), inj):
                assert np.array_equal(x, y, equal_nan=True)
            _same(plan.belt(R, S, data, frac, P, SEED, raw=True, **kw), base, "after the refusals", NAMES)
        plan.set_detector(None)
        with pytest.raises(_lib.NusiError) as e:
            plan.belt(R, S, data, frac, P, SEED)
        assert e.value.code == _lib.NUSI_ESTATE
    finally:
        plan.close()
