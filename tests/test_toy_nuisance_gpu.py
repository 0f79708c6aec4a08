"""The toys' ensembles on the GPU (NUSI_OPT_TOY_NUISANCE): k_nuis_inject<NC, MODE> under GLOBAL and PRIOR, k_nuis_belt<NC>
under GLOBAL, against what include/nusi.h says a toy's record is.

Shapes: C = 1, 5, 17, 64 (one lane; padded butterflies; one group a wave), K = 1 and K = 3 (tests/test_inject_gpu.py's
priors: at C > 3 one of the three templates has no prior), Q = 3 with a spectrum of zeros, P = 5, and for belt G = 3.
The calls run on G6's five tables, because the budget check below needs three chunks with a partial last one and two
tables hold two units; the record-by-record checks read the first two tables.

Per case, three things:
  1. data_all equals plan.draw of the right expectation: inject under GLOBAL and belt under GLOBAL the FIXED call's (mu_inj,
     and the observed conditional fit's mu from plan.fit_fixed); inject under PRIOR a_inj s + sum_j theta*_j T_j + B per toy.
  2. nuis_all is rebuilt through plan.draw_normal with the documented identity and centres (theta_inj; the prior means;
     theta_obs[t, q, 1 + g, 1 + j]).  Under GLOBAL every toy's theta_hat_0 and both words are the bits of plan.fit /
     plan.fit_fixed after plan.set_templates(T, prior=(m*, sigma)), and stat is within tests/test_inject_gpu.py's
     allowance of 2 (nll_fixed - nll_hat) from those calls (a non-finite nll: skipped, as there).  Under PRIOR the same
     with the plan's own prior.
  3. Against detector.inject_host / belt_host with the oracle's exp and log (table 0, the first two spectra, the first
     four toys): the same nuis_all, toys, theta_hat, flags and counts to the bit, stat within 2 eps_lambda.
Then the same bits without raw arrays under a budget of three chunks with a partial last one, with two p-slices, and with
both; FIXED set explicitly equals a fresh plan's call; with every prior removed GLOBAL and PRIOR are FIXED; and the
refusals -- a bad option value, belt under PRIOR -- vary values only: no call passes a size other than its arrays' own.
"""
import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from tests.test_belt_gpu import ALPHA, FRAC, _grid, _interval_alone, _interval_budget, _setting, _valid_flags
from tests.test_detector_gpu import nusi  # noqa: F401  (the fixture)
from tests.test_ensemble_limit_gpu import _chunk_budget
from tests.test_inject_gpu import FAIL, SEED, U, _case, _Dev, _hip, _mu_inj, _ora, _same
from tests.test_inject_gpu import NAMES as INJECT_NAMES
from tests.test_belt_gpu import NAMES as BELT_NAMES
from tests.test_limit_gpu import _mag

pytestmark = pytest.mark.gpu

Q, P, G, NT = 3, 5, 3, 2
FLAGS = ~(detector.FIT_STEPS_MASK | (detector.FIT_TRIALS_MASK << detector.FIT_TRIALS_SHIFT))
ENS = {"global": _lib.TOYS_GLOBAL, "prior": _lib.TOYS_PRIOR}


def _sigma(K, prior):
    m, w = detector._prior(K, prior)
    return m, w, detector._prior_sigma(K, prior, w)


def _record(plan, R1, S1, at, d, T, prior_p, th0, stat, words, what):
    """One toy's record through the existing calls on the plan as it stands: theta_hat_0 and both words to the bit, stat
    within tests/test_inject_gpu.py's allowance.  Returns err / allowance, or None where stat is not compared."""
    K, C = len(T), len(d)
    m, w = detector._prior(K, prior_p)
    thh, nh, muh, sth = (x[0, 0] for x in plan.fit(R1, S1, d))
    thc, nc, muc, stc = (x[0, 0] for x in plan.fit_fixed(R1, S1, at, d))
    assert (words[0], words[1]) == (sth, stc), (what, hex(words[0]), hex(sth), hex(words[1]), hex(stc))
    if sth & FAIL:
        assert np.isnan(th0) and np.isnan(stat), what
        return None
    assert th0 == thh[0] and not np.signbit(th0), (what, th0, thh[0])
    if stc & FAIL:
        assert np.isnan(stat), what
        return None
    assert stat >= 0 and not np.signbit(stat), (what, stat)
    if not (np.isfinite(nh) and np.isfinite(nc)):
        return None
    with np.errstate(all="ignore"):
        _, mg = detector._limit_lambda(at, thc[1:], muc, muh, thh[1:], (d > 0) & (muh > 0), d, m[1:], w[1:], np.log)
    allow = 2.0 * (2 * (C + 3 + 3 * K) * U * (_mag(muc, d, thc, m, w) + _mag(muh, d, thh, m, w))) + 2.0 * detector.limit_kappa(C, K) * U * mg
    err = abs(stat - 2.0 * (nc - nh))
    assert err <= allow, (what, stat, 2.0 * (nc - nh), allow)
    return err / allow if allow > 0 else 0.0


def _stat_close(a, b, R0, Sq, at, d, T, prior_p, B, log, what):
    """stat of the host form and of the device within 2 eps_lambda (tests/test_inject_gpu.py's third check)."""
    if np.isnan(a) or a == b:
        return
    K, C = len(T), len(d)
    m, w = detector._prior(K, prior_p)
    mg = detector._inject_one(R0, Sq, at, d, T, prior_p, B, m, w, detector.INJECT_TWO_SIDED, log)[7]
    assert abs(a - b) <= 2.0 * detector.limit_kappa(C, K) * U * mg, (what, a, b)


@pytest.mark.parametrize("ens", ("global", "prior"))
@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_inject_ensembles(nusi, oracle_mod, C, K, ens):  # noqa: F811
    exp, log = _ora(oracle_mod)
    what = "inject %s C=%d K=%d" % (ens, C, K)
    plan, R, S, T, prior, B, acc, a_inj, th_inj = _case(nusi, C, K, Q)
    try:
        ntab = R.shape[0]
        m, w, sg = _sigma(K, prior)
        assert (w[1:] > 0).any() and (C <= 3 or K == 1 or (w[1:] == 0).sum() == 1), what
        q_obs = np.broadcast_to(np.array([0.0, 0.5, 2.706, np.nan, 1e3])[:, None], (ntab, Q)).copy()
        kw = dict(theta_inj=th_inj, ranks=list(range(P)), q_obs=q_obs)
        fixed = plan.inject(R, S, a_inj, P, SEED, raw=True, **kw)
        base = plan.inject(R, S, a_inj, P, SEED, raw=True, nuisance=ens, **kw)
        assert len(base) == 8
        th_all, st_all, words, data = base[4:]
        # nuis_all through plan.draw_normal
        centre = th_inj if ens == "global" else np.where(w[1:] > 0, m[1:], th_inj)
        nuis = np.stack([plan.draw_normal(np.broadcast_to(centre, (Q, K)), sg, P, SEED, stream=t) for t in range(ntab)])
        assert nuis.shape == (ntab, Q, P, K) and np.all(nuis >= 0)
        assert np.array_equal(nuis[..., w[1:] == 0], np.broadcast_to(th_inj[w[1:] == 0], nuis[..., w[1:] == 0].shape))
        # 1. the toys
        if ens == "global":
            assert np.array_equal(data, fixed[7]), what
            mu = _mu_inj(acc, a_inj, th_inj, T, B)
            for t in range(ntab):
                assert np.array_equal(data[t], plan.draw(mu[t], P, SEED, stream=t)), (what, t)
            assert not np.array_equal(th_all, fixed[4], equal_nan=True), what
        else:
            for t in range(ntab):
                for p in range(P):
                    mu = a_inj[:, None] * acc[t]
                    for j in range(K):
                        mu = mu + nuis[t, :, p, j][:, None] * T[j][None, :]
                    mu = mu + B[None, :]
                    assert np.array_equal(data[t, :, p], plan.draw(mu, P, SEED, stream=t)[:, p]), (what, t, p)
            assert not np.array_equal(data, fixed[7]), what
        # 3. the host form (before the plan's templates are set anew below)
        nq, np_ = 2, 4
        h = detector.inject_host(R[0], S[:nq], a_inj[:nq], np_, SEED, theta_inj=th_inj, ranks=[0], templates=T, prior=prior,
                                 background=B, exp=exp, log=log, raw=True, nuisance=ens)
        hth, hst, hwords, hdata, hnuis = h[3:]
        assert np.array_equal(hnuis[0], nuis[0, :nq, :np_]), what
        assert np.array_equal(hdata[0], data[0, :nq, :np_]), what
        assert np.array_equal(hth[0], th_all[0, :nq, :np_], equal_nan=True), what
        assert np.array_equal(hwords[0] & FLAGS, words[0, :nq, :np_] & FLAGS), what
        assert np.array_equal(np.isnan(hst[0]), np.isnan(st_all[0, :nq, :np_])), what
        for q in range(nq):
            for p in range(np_):
                pr_p = (nuis[0, q, p], sg) if ens == "global" else prior
                _stat_close(hst[0, q, p], st_all[0, q, p], R[0], S[q], a_inj[q], data[0, q, p], T, pr_p, B, log, (what, q, p))
        # the bands and the counts follow the raw arrays
        with np.errstate(invalid="ignore"):
            exceed = (st_all >= q_obs[..., None]).sum(-1).astype(np.int32)
        _same(base[:4], (detector.order_stat(th_all, list(range(P))), detector.order_stat(st_all, list(range(P))),
                         detector.inject_tally(words), exceed), what + ": from the raw arrays", INJECT_NAMES[:4])
        # every budget and slicing: the same bits, without the raw arrays
        budget = _chunk_budget(ntab, Q, C, P, 2)
        for nbytes, ps in ((0, 0), (budget, 0), (0, 2), (budget, 2)):
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
            plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, ps)
            _same(plan.inject(R, S, a_inj, P, SEED, **kw), base[:4], "%s: no raw arrays, budget %d, p-slices %d" % (what, nbytes, ps))
            if ps:
                _same(plan.inject(R, S, a_inj, P, SEED, raw=True, **kw), base, "%s: raw arrays, p-slices %d" % (what, ps))
        plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
        plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, 0)
        # FIXED set explicitly is the fresh plan's call
        _same(plan.inject(R, S, a_inj, P, SEED, raw=True, nuisance="fixed", **kw), fixed, what + ": back to fixed")
        _same(plan.inject(R, S, a_inj, P, SEED, raw=True, **kw), fixed, what + ": the option stays")
        # 2. every toy of the first two tables through the existing calls
        worst, n = 0.0, 0
        for t in range(NT):
            for q in range(Q):
                for p in range(P):
                    pr_p = (nuis[t, q, p], sg) if ens == "global" else prior
                    if ens == "global":
                        plan.set_templates(T, prior=pr_p)
                    r = _record(plan, R[t:t + 1], S[q:q + 1], a_inj[q], data[t, q, p], T, pr_p, th_all[t, q, p], st_all[t, q, p],
                                words[t, q, p], (what, t, q, p))
                    if r is not None:
                        worst, n = max(worst, r), n + 1
        print("%s: %d toys through the existing calls, %d statistics compared, err / allowance max %.3f" % (what, NT * Q * P, n, worst))
        # nothing constrained: every ensemble is FIXED
        plan.set_templates(T, prior=None)
        free = plan.inject(R[:NT], S, a_inj, P, SEED, raw=True, nuisance="fixed", **dict(kw, q_obs=q_obs[:NT]))
        for e in ("global", "prior"):
            _same(plan.inject(R[:NT], S, a_inj, P, SEED, raw=True, nuisance=e, **dict(kw, q_obs=q_obs[:NT])), free, what + ": no prior, " + e)
    finally:
        plan.close()


@pytest.mark.parametrize("K", (1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_belt_global(nusi, oracle_mod, C, K):  # noqa: F811
    exp, log = _ora(oracle_mod)
    what = "belt global C=%d K=%d" % (C, K)
    plan, R, S, T, prior, B, data, ref = _setting(nusi, C, K, Q)
    H = _hip()
    try:
        ntab, frac = R.shape[0], FRAC[G]
        m, w, sg = _sigma(K, prior)
        a, agood = _grid(frac, ref)
        fixed = plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA, raw=True)
        base = plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA, raw=True, nuisance="global")
        assert len(base) == 13
        q_obs, th_obs, w_obs, th_all, st_all, words, toys = base[6:]
        valid, flags = _valid_flags(w_obs, agood)
        assert valid[:NT].any() and not valid[:, 2].any(), what
        # the observed side reads the plan's means; 1. the toys are FIXED's, plan.draw of the conditional fit's mu
        for k in (6, 7, 8, 12):
            assert np.array_equal(base[k], fixed[k], equal_nan=True), (what, BELT_NAMES[k])
        for t in range(NT):
            mu = np.zeros((Q, G, C))
            for g in range(G):
                at = np.where(agood[t, :, g], a[t, :, g], 0.0)
                mu[:, g] = np.where(valid[t, :, g][:, None], plan.fit_fixed(R[t:t + 1], S, at, data)[2][0], 0.0)
            assert np.array_equal(toys[t].reshape(Q * G, P, C), plan.draw(mu.reshape(Q * G, C), P, SEED, stream=t)), (what, t)
        assert not np.array_equal(st_all, fixed[10], equal_nan=True), what
        # nuis_all through plan.draw_normal: the centres are the observed conditional fits'
        nuis = np.zeros((ntab, Q, G, P, K))
        for t in range(ntab):
            centre = np.where(valid[t][..., None], th_obs[t, :, 1:, 1:], 0.0).reshape(Q * G, K)
            nuis[t] = plan.draw_normal(centre, sg, P, SEED, stream=t).reshape(Q, G, P, K)
        # 3. the host form
        nq, np_ = 2, 4
        h = detector.belt_host(R[0], S[:nq], data, frac, np_, SEED, ref=ref[0:1, :nq], alpha=ALPHA, templates=T, prior=prior,
                               background=B, exp=exp, log=log, raw=True, nuisance="global")
        got = [x[0:1, :nq] for x in base]
        got[9:] = [x[:, :, :, :np_] for x in got[9:]]
        v0 = valid[0:1, :nq]
        assert np.array_equal(h[13][v0], nuis[0:1, :nq, :, :np_][v0]), what
        assert np.array_equal(h[12], got[12]) and np.array_equal(h[7], got[7], equal_nan=True), what
        assert np.array_equal(h[9], got[9], equal_nan=True), what
        assert np.array_equal(h[8] & FLAGS, got[8] & FLAGS) and np.array_equal(h[11] & FLAGS, got[11] & FLAGS), what
        assert np.array_equal(np.isnan(h[10]), np.isnan(got[10])), what
        for _, q, g, p in zip(*np.nonzero(~np.isnan(h[10]))):
            _stat_close(h[10][0, q, g, p], got[10][0, q, g, p], R[0], S[q], float(a[0, q, g]), got[12][0, q, g, p], T,
                        (nuis[0, q, g, p], sg), B, log, (what, q, g, p))
        # the counts from the raw arrays, the interval from the counts
        with np.errstate(invalid="ignore"):
            exceed = (st_all >= q_obs[..., None]).sum(-1).astype(np.int32)
        tally = np.where(valid[..., None], detector.inject_tally(words), 0).astype(np.int32)
        assert np.array_equal(exceed, base[4]) and np.array_equal(tally, base[5]), what
        _same(base[:4], detector.belt_accept(exceed, tally, a, ALPHA, valid, P, flags), what + ": the interval from the counts", BELT_NAMES[:4])
        # every budget and slicing: the same bits, without the raw arrays
        budget = _interval_budget(ntab, Q, G)
        with _Dev(H) as dev:
            dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
            for nbytes, ps in ((0, 0), (budget, 0), (0, 2), (budget, 2)):
                plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
                plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, ps)
                tag = "%s: budget %d, p-slices %d" % (what, nbytes, ps)
                _same(plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA), base[:9], tag + ", no raw arrays", BELT_NAMES[:9])
                _same(_interval_alone(plan, H, dev, dR, ntab, S, data, frac, ref, P, "two-sided"), base[:4], tag + ", the interval alone", BELT_NAMES[:4])
                if ps:
                    _same(plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA, raw=True), base, tag + ", raw arrays", BELT_NAMES)
        plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
        plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, 0)
        _same(plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA, raw=True, nuisance="fixed"), fixed, what + ": back to fixed", BELT_NAMES)
        # 2. every toy of the first two tables' valid records through the existing calls
        worst, n, toys_n = 0.0, 0, 0
        for t, q, g in zip(*np.nonzero(valid[:NT])):
            for p in range(P):
                pr_p = (nuis[t, q, g, p], sg)
                plan.set_templates(T, prior=pr_p)
                r = _record(plan, R[t:t + 1], S[q:q + 1], float(a[t, q, g]), toys[t, q, g, p], T, pr_p, th_all[t, q, g, p],
                            st_all[t, q, g, p], words[t, q, g, p], (what, t, q, g, p))
                toys_n += 1
                if r is not None:
                    worst, n = max(worst, r), n + 1
        print("%s: %d toys through the existing calls, %d statistics compared, err / allowance max %.3f" % (what, toys_n, n, worst))
    finally:
        plan.close()


def test_the_option_and_refusals(nusi):  # noqa: F811
    """Values only: a bad option value, and belt under PRIOR, which does no device work and changes nothing."""
    C, K = 5, 1
    plan, R, S, T, prior, B, data, ref = _setting(nusi, C, K, Q)
    H = _hip()
    try:
        for bad in (-1, 3):
            with pytest.raises(_lib.NusiError) as e:
                plan.set_option(_lib.OPT_TOY_NUISANCE, bad)
            assert e.value.code == _lib.NUSI_EPARAM
        with pytest.raises(_lib.NusiError):
            plan.inject(R, S, 1.0, P, SEED, nuisance=3)
        for ok in (_lib.TOYS_PRIOR, _lib.TOYS_GLOBAL, _lib.TOYS_FIXED):
            plan.set_option(_lib.OPT_TOY_NUISANCE, ok)
        frac = FRAC[G]
        base = plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA)
        with _Dev(H) as dev:
            dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
            dLo = dev.alloc(base[0].nbytes, np.full(base[0].shape, np.nan))
            with pytest.raises(_lib.NusiError) as e:
                plan.belt_device(dR, R.shape[0], S, data, frac, P, SEED, ref=ref, alpha=ALPHA, d_lo_ptr=dLo, nuisance="prior")
            assert e.value.code == _lib.NUSI_EPARAM and "NUSI_TOYS_PRIOR" in _lib.last_error()
            assert H.hipDeviceSynchronize() == 0
            assert np.all(np.isnan(dev.fetch(dLo, base[0].shape)))
        with pytest.raises(_lib.NusiError):
            plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA)        # the option stays: still PRIOR
        # inject takes PRIOR; then belt again under the name that it takes
        plan.inject(R[:NT], S, 1.0, P, SEED)
        _same(plan.belt(R, S, data, frac, P, SEED, ref=ref, alpha=ALPHA, nuisance=_lib.TOYS_FIXED), base, "after the refusals", BELT_NAMES[:9])
    finally:
        plan.close()
