"""Limits on the signal's scale on the GPU: k_interval (nusi_plan_response_limit).

  * strict: theta_hat, nll_hat and the best fit's word are the bits of plan.fit (plan.profile without templates), and
    a record does not depend on the call's other tables and spectra;
  * through EXISTING device code: at a returned limit a, q = 2 (nll(a) - nll_hat) with nll(a) from plan.events at the
    scale a (K = 0) or plan.fit_fixed (K >= 1) and nll_hat from plan.profile / plan.fit is within
    2 (bound_cond + bound_hat) + 2 eps_lambda of delta: the bounds are test_detector_gpu._check_nll's and
    test_fit_gpu._check's, 2 (C + 3 + 3 K) u (sum_c (mu_c + |d_c log mu_c|) + penalties), eps_lambda the stop's
    allowance as detector.limit_host reports it;
  * against detector.limit_host with the oracle's log: the flags are equal and |a_gpu - a_host| <= 2 eps_lambda /
    min(|g_0(a_gpu)|, |g_0(a_host)|) + 4 u a (lambda is convex, so between two points that both meet the stop the
    slope is at least the smaller of theirs); the step counts are printed, not asserted, because the device log's last
    bits may decide a step.  No record is left out on the real fold; the share that agrees to the bit is printed.

Shapes as for the fit: C = 1 (a group is one lane), 5 and 17 (padded butterflies), 64 (one group a wave); Q = 1, 5, 19
(partial blocks), 600 at C = 1 (several blocks); K = 0, 1, 3 are the smallest and the largest instance, K = 2 runs in the
synthetic classes.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (LIMIT_AT_ZERO, LIMIT_INNER_SHIFT, LIMIT_ITER_MAX, LIMIT_NO_FIT, LIMIT_NOT_CONVERGED,
                                   LIMIT_STEPS_MASK, LIMIT_UNBOUNDED)
from tests.test_detector_gpu import (GRIDS, MAXIS, _D, _Dev, _folded, _hip, _ora_log, _plan, _spectra,
                                     nusi)  # noqa: F401  (nusi: the fixture)
from tests.test_fit_gpu import FIT_CLASSES, _data, _fit_case, _prior_of, _templates
from tests.test_profile_gpu import EDGE_CLASSES, _edge_case, _fetch_int
from tests.test_profile_gpu import _data as _data0

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
N = GRIDS["G6"][0]
U = 2.0 ** -53
DELTA = 2.706
FLAGS = LIMIT_AT_ZERO | LIMIT_UNBOUNDED | LIMIT_NO_FIT | LIMIT_NOT_CONVERGED


def _mag(mu, data, theta, m, w):
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.sum(mu + np.where(data > 0, np.abs(data * np.log(np.where(mu > 0, mu, 1.0))), 0.0), axis=-1)
    return x + np.sum(0.5 * w * (theta - m) ** 2, axis=-1)


def _cond(plan, R, S, a, data, K):
    """(nll, mu, theta) at the held scales a (ntab, Q) through the existing device calls, table by table."""
    ntab, Q = a.shape
    nll, mu, th = np.zeros((ntab, Q)), np.zeros((ntab, Q, R.shape[2])), np.zeros((ntab, Q, 1 + K))
    for t in range(ntab):
        if K:
            th[t], nll[t], mu[t], _ = (x[0] for x in plan.fit_fixed(R[t:t + 1], S, a[t], data))
        else:
            m1, n1 = plan.events(R[t:t + 1], S, scale=a[t], data=data)
            mu[t], nll[t], th[t, :, 0] = m1[0], n1[0], a[t]
    return nll, mu, th


def _slope(R, S, a, mu, data):
    """g_0 = sum_c s_c - sum_c d_c s_c / mu_c at given counts (plain numpy: it enters a bound)."""
    s = detector.events_host(R, S)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s.sum(axis=-1) - np.sum(np.where((data > 0) & (mu > 0), data * s / np.where(mu > 0, mu, 1.0), 0.0), axis=-1)


def _check(plan, got, R, S, data, T, prior, B, log, what, which="both", strict_records=True):
    """The module docstring's three checks of one call.  Returns (the host's results, the share of bit-equal limits)."""
    lo, hi, th, nll, st = got
    K = 0 if T is None else len(T)
    C = len(data)
    det = {}
    hlo, hhi, hth, hnll, hst = detector.limit_host(R, S, data, DELTA, which, templates=T, prior=prior, background=B, log=log,
                                                   details=det)
    best = plan.fit(R, S, data) if K else plan.profile(R, S, data)
    bth = best[0] if K else best[0][..., None]
    assert np.array_equal(th, bth) and np.array_equal(nll, best[1], equal_nan=True) and np.array_equal(st[..., 0], best[3]), what
    assert np.array_equal(th, hth) and np.array_equal(st[..., 0], hst[..., 0]), what
    assert np.array_equal(st & FLAGS, hst & FLAGS), (what, np.argwhere((st & FLAGS) != (hst & FLAGS))[:4])
    m, w = detector._prior(K, prior)
    bound_hat = 2 * (C + 3 + 3 * K) * U * _mag(best[2], data, bth, m, w)
    left_out = equal = total = 0
    for side, (g, h) in enumerate(((lo, hlo), (hi, hhi))):
        word, hword = st[..., 1 + side], hst[..., 1 + side]
        if not which in ("both", ("lower", "upper")[side]):
            assert np.all(np.isnan(g)) and np.all(word == 0), what
            continue
        assert np.array_equal(np.isnan(g), np.isnan(h)) and np.array_equal(np.isinf(g), np.isinf(h)), what
        live = np.isfinite(h) & (word & LIMIT_STEPS_MASK > 0) & ((word & (LIMIT_AT_ZERO | LIMIT_NOT_CONVERGED)) == 0)
        assert np.array_equal(g[~live], h[~live], equal_nan=True), what       # NaN, +inf and the zeros
        if not live.any():
            continue
        eps = det["eps"][..., side]
        ag, ah = np.where(live, g, 1.0), np.where(live, h, 1.0)
        ng, mug, thg = _cond(plan, R, S, ag, data, K)
        nh, muh, thh = _cond(plan, R, S, ah, data, K)
        fin = live & np.isfinite(ng) & np.isfinite(best[1])
        with np.errstate(invalid="ignore"):         # (inf - inf where both are INFINITE: not in `fin`)
            q = 2.0 * (ng - best[1])
        allow = 2.0 * (2 * (C + 3 + 3 * K) * U * _mag(mug, data, thg, m, w) + bound_hat) + 2.0 * eps
        assert np.all(np.abs(q - DELTA)[fin] <= allow[fin]), (what, side, np.max(np.abs(q - DELTA)[fin] / allow[fin]))
        g0 = np.minimum(np.abs(_slope(R, S, ag, mug, data)), np.abs(_slope(R, S, ah, muh, data)))
        tol = 2.0 * eps / g0 + 4 * U * np.abs(h)
        with np.errstate(invalid="ignore"):         # (inf - inf of the unbounded records: not in `live`)
            off = live & ~(np.abs(g - h) <= tol)
        # a record may be left out only where the host's last |h| lies within 2 eps of its stop
        near = np.abs(np.abs(det["h"][..., side]) - eps) <= 2.0 * eps
        assert not np.any(off & ~near), (what, side, np.argwhere(off & ~near)[:4])
        left_out += int(np.count_nonzero(off))
        equal += int(np.count_nonzero(live & (g == h)))
        total += int(np.count_nonzero(live))
        if fin.any():
            print("%s %s: |q - delta| / allowance max %.3f; outer steps gpu %d .. %d host %d .. %d, inner mean %.1f" % (
                what, ("lower", "upper")[side], float(np.max(np.abs(q - DELTA)[fin] / allow[fin])),
                (word & 0xFF)[live].min(), (word & 0xFF)[live].max(), (hword & 0xFF)[live].min(), (hword & 0xFF)[live].max(),
                float(((word >> LIMIT_INNER_SHIFT) & 0x7FFF)[live].mean())))
    if strict_records:
        assert left_out == 0, (what, left_out)
    assert left_out <= 0.1 * max(total, 1), (what, left_out, total)
    share = equal / total if total else 1.0
    print("%s: %d of %d limits equal the host's to the bit (%.0f %%), %d left out" % (what, equal, total, 100 * share, left_out))
    return (hlo, hhi, hth, hnll, hst), share


# --- a real fold: the G6 tables ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
@pytest.mark.parametrize("Q", (1, 5, 19))
def test_limits_on_the_real_fold(nusi, oracle_mod, Q, C, K):  # noqa: F811
    log = _ora_log(oracle_mod)
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0) if K else None
    data = _data(R, S, T, B, C, seed=C + Q) if K else _data0(R, S, B, C, seed=C + Q)
    if C > 1:
        data[C - 1] = 0.0                           # the bin nothing ever fills
    prior = _prior_of(T, "loose" if C == 1 else "mixed") if K else None    # (one bin: the priors determine the templates)
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    if K:
        plan.set_templates(T, prior=prior)
    got = plan.limit(R, S, data, DELTA, which="both")
    (hlo, hhi, hth, hnll, hst), _ = _check(plan, got, R, S, data, T, prior, B, log, "G6 C=%d Q=%d K=%d" % (C, Q, K))
    # the input contract: no record fails, and the search stays far below its cap
    assert not np.any(hst[..., 1:] & (LIMIT_NOT_CONVERGED | LIMIT_NO_FIT)) and not np.any(got[4][..., 1:] & LIMIT_NOT_CONVERGED)
    assert (hst[..., 1:] & LIMIT_STEPS_MASK).max() < LIMIT_ITER_MAX // 2 and (got[4][..., 1:] & LIMIT_STEPS_MASK).max() < LIMIT_ITER_MAX // 2
    assert np.all(got[0] <= got[2][..., 0]) and np.all(got[2][..., 0] <= got[1])
    # upper alone: the bits of hi from the call for both sides, the lower outputs NaN / 0
    up = plan.limit(R, S, data, DELTA, which="upper")
    assert np.array_equal(up[1], got[1]) and np.array_equal(up[4][..., 2], got[4][..., 2]) and np.array_equal(up[4][..., 0], got[4][..., 0])
    assert np.all(np.isnan(up[0])) and np.all(up[4][..., 1] == 0) and np.array_equal(up[2], got[2]) and np.array_equal(up[3], got[3])
    plan.close()


# --- synthetic matrices: a wave whose groups part ways -------------------------------------------------------------------------
def _waves(words, per_wave):
    for t in range(words.shape[0]):
        for q0 in range(0, words.shape[1], per_wave):
            yield words[t, q0:q0 + per_wave]


@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_a_wave_whose_groups_part_ways(nusi, oracle_mod, C):  # noqa: F811
    """The synthetic classes of the profile's and the fit's tests, signals decades apart: one wave holds different outer
    step counts, a lower limit at zero beside a two-sided interval, and a record without signal (unbounded) beside live
    ones -- all of it read from the DEVICE's words.  At C = 64 a wave holds one group: there the same is held over the
    block's four waves.  With one bin lambda(0) = B - d + d log(d / B) whatever the signal -- any signal fits the one count
    -- so the live records of a call have their lower limits on the same side of zero; at C = 1 the lower limit at zero
    beside the two-sided intervals is therefore that of a record without signal (a_lo = 0, `UNBOUNDED | AT_ZERO`), at
    C > 1 it is a live record's."""
    log = _ora_log(oracle_mod)
    plan = _plan(nusi, "G6")
    D = _D(C, N)
    lg = int(np.ceil(np.log2(C))) if C > 1 else 0
    per_wave = max(64 >> lg, 4)
    steps_part = zero_beside = unb_beside = False
    cases = [(w, None, None) + _edge_case(C, w, dec, bk, ntab=3, Q=40) for w, dec, bk in EDGE_CLASSES[::2]]
    cases += [(w,) + (lambda c: (c[3], c[4], c[0], c[1], c[2], c[5]))(_fit_case(C, w, dec, bk, pk, K))
              for w, dec, bk, pk, K in (FIT_CLASSES[1], FIT_CLASSES[6], FIT_CLASSES[7])]
    for what, T, prior, R, S, data, B in cases:
        if T is None:
            S = np.array(S)
            S[3::16] = 0.0                          # spectra of zeros among the groups of a wave
        plan.set_detector(D, background=B)
        plan.set_templates(T, prior=prior)
        got = plan.limit(R, S, data, DELTA, which="both")
        (hlo, hhi, hth, hnll, hst), _ = _check(plan, got, R, S, data, T, prior, B, log,
                                               "C=%d K=%d %s" % (C, 0 if T is None else len(T), what), strict_records=False)
        st = got[4]                                 # the device's words
        for lo_w, hi_w in zip(_waves(st[..., 1], per_wave), _waves(st[..., 2], per_wave)):
            live = (hi_w & (LIMIT_UNBOUNDED | LIMIT_NO_FIT)) == 0
            at_zero = (lo_w & LIMIT_AT_ZERO) != 0
            two_sided = live & ((lo_w & (LIMIT_AT_ZERO | LIMIT_NOT_CONVERGED)) == 0) & ((lo_w & LIMIT_STEPS_MASK) > 0)
            steps_part |= len(set((hi_w & LIMIT_STEPS_MASK)[live].tolist())) > 1
            zero_beside |= bool(np.any(at_zero & (live | (C == 1))) and np.any(two_sided))
            unb_beside |= bool(np.any(hi_w & LIMIT_UNBOUNDED) and np.any(live))
    plan.close()
    assert steps_part and zero_beside and unb_beside, (steps_part, zero_beside, unb_beside)


# --- equivalence and the device form --------------------------------------------------------------------------------------
def test_records_alone_and_the_device_form(nusi):  # noqa: F811
    C, Q, K = 17, 19, 3
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0)
    data = _data(R, S, T, B, C, seed=2)
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=_prior_of(T, "mixed"))
    got = plan.limit(R, S, data, DELTA, which="both")
    lo, hi, th, nll, st = got
    for t in range(3):                              # a 3-table call against each table alone, and a spectrum alone
        one = plan.limit(R[t:t + 1], S, data, DELTA, which="both")
        for x, y in zip(one, got):
            assert np.array_equal(x[0], y[t]), t
    one = plan.limit(R, S[6:7], data, DELTA, which="both")
    for x, y in zip(one, got):
        assert np.array_equal(x[:, 0], y[:, 6])
    H = _hip()
    with _Dev(H) as dev:                            # into NaN-filled buffers, each optional output NULL in turn
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        for skip in (None, "theta", "nll", "status", "lo"):
            dL, dH = dev.alloc(lo.nbytes, np.full(lo.shape, np.nan)), dev.alloc(hi.nbytes, np.full(hi.shape, np.nan))
            dT, dN = dev.alloc(th.nbytes, np.full(th.shape, np.nan)), dev.alloc(nll.nbytes, np.full(nll.shape, np.nan))
            dS = dev.alloc(st.nbytes, np.full(st.shape, -1, dtype=np.int32))
            assert plan.limit_device(dR, 3, S, data, DELTA, "upper" if skip == "lo" else "both", None if skip == "lo" else dL, dH,
                                     None if skip == "theta" else dT, None if skip == "nll" else dN,
                                     None if skip == "status" else dS) == Q
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(dev.fetch(dH, hi.shape), hi), skip
            l2, t2, n2, s2 = dev.fetch(dL, lo.shape), dev.fetch(dT, th.shape), dev.fetch(dN, nll.shape), _fetch_int(H, dS, st.shape)
            assert np.all(np.isnan(l2)) if skip == "lo" else np.array_equal(l2, lo), skip
            assert np.all(np.isnan(t2)) if skip == "theta" else np.array_equal(t2, th), skip
            assert np.all(np.isnan(n2)) if skip == "nll" else np.array_equal(n2, nll), skip
            if skip == "status":
                assert np.all(s2 == -1)
            elif skip == "lo":
                assert np.array_equal(s2[..., 0], st[..., 0]) and np.array_equal(s2[..., 2], st[..., 2]) and np.all(s2[..., 1] == 0)
            else:
                assert np.array_equal(s2, st), skip
    plan.close()


def test_many_spectra_on_one_bin(nusi, oracle_mod):  # noqa: F811
    """Q = 600 at C = 1: 256 chains a block, a partial last block; no templates.  The device form writes into buffers of
    NaNs (status: of -1): no entry may be left unwritten."""
    log = _ora_log(oracle_mod)
    C, Q = 1, 600
    R, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    data = np.array([9.0])
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    got = plan.limit(R, S, data, DELTA, which="both")
    _check(plan, got, R, S, data, None, None, B, log, "G6 C=1 Q=600 K=0")
    H = _hip()
    with _Dev(H) as dev:
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        dL, dH = dev.alloc(got[0].nbytes, np.full((3, Q), np.nan)), dev.alloc(got[1].nbytes, np.full((3, Q), np.nan))
        dT, dN = dev.alloc(got[2].nbytes, np.full((3, Q, 1), np.nan)), dev.alloc(got[3].nbytes, np.full((3, Q), np.nan))
        dS = dev.alloc(got[4].nbytes, np.full((3, Q, 3), -1, dtype=np.int32))
        assert plan.limit_device(dR, 3, S, data, DELTA, "both", dL, dH, dT, dN, dS) == Q
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dL, (3, Q)), got[0]) and np.array_equal(dev.fetch(dH, (3, Q)), got[1])
        assert np.array_equal(dev.fetch(dT, (3, Q, 1)), got[2]) and np.array_equal(dev.fetch(dN, (3, Q)), got[3])
        assert np.array_equal(_fetch_int(H, dS, (3, Q, 3)), got[4])
    plan.close()


# --- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(nusi):  # noqa: F811
    from nusiprop_amd import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    C, K = 5, 2
    R, D, B = _folded(nusi, C)
    S = _spectra(M, 2)
    data = np.full(C, 30.0)
    plan = _plan(nusi, "G6")

    def refused(code, f, *args, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*args, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    refused(_lib.NUSI_ESTATE, plan.limit, np.ones((1, M, C)), S, data, DELTA)                 # no detector
    plan.set_detector(D, background=B)
    want0 = plan.limit(R, S, data, DELTA, which="both")                                     # without templates: K = 0
    assert want0[2].shape == (3, 2, 1)
    plan.set_templates(_templates(C, K), prior=([1.0, 1.0], [np.inf, 0.5]))
    want_fit, want = plan.fit(R, S, data), plan.limit(R, S, data, DELTA, which="both")
    assert want[2].shape == (3, 2, 1 + K)
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(_lib.NUSI_EPARAM, plan.limit, R, S, data, bad)                              # delta
    for bad in (0, 4, -1):
        refused(_lib.NUSI_EPARAM, plan.limit, R, S, data, DELTA, which=bad)
    refused(_lib.NUSI_EPARAM, plan.limit, R, S, None, DELTA)                                # NULL data
    for bad in (-1.0, np.nan, np.inf):
        db, Sb = data.copy(), np.array(S)
        db[C - 1] = bad
        Sb[1, M - 1] = bad
        refused(_lib.NUSI_EPARAM, plan.limit, R, S, db, DELTA)
        refused(_lib.NUSI_EPARAM, plan.limit, R, Sb, data, DELTA)
    with pytest.raises(ValueError):
        plan.limit(R[:, :-1], S, data, DELTA)
    with pytest.raises(ValueError):
        plan.limit(R, S, data[:-1], DELTA)
    H = _hip()
    with _Dev(H) as dev:
        dR, dA = dev.alloc(R.nbytes, np.ascontiguousarray(R)), dev.alloc(3 * 2 * 8)
        lm = L.nusi_plan_response_limit
        d = ctypes.c_double(DELTA)
        assert lm(plan._h, dR, 3, Sp, 2, datap, d, 2, None, None, None, None, None, None) == _lib.NUSI_EPARAM    # no hi
        assert lm(plan._h, dR, 3, Sp, 2, datap, d, 3, None, dA, None, None, None, None) == _lib.NUSI_EPARAM      # no lo
        assert lm(plan._h, dR, 3, Sp, 2, datap, d, 1, None, dA, None, None, None, None) == _lib.NUSI_EPARAM
        assert lm(plan._h, dR, 3, Sp, 2, None, d, 2, None, dA, None, None, None, None) == _lib.NUSI_EPARAM       # no data
        assert lm(plan._h, None, 3, Sp, 2, datap, d, 2, None, dA, None, None, None, None) == _lib.NUSI_EPARAM
        assert lm(plan._h, dR, 0, Sp, 2, datap, d, 2, None, dA, None, None, None, None) == _lib.NUSI_EPARAM
        assert lm(plan._h, dR, 3, Sp, 0, datap, d, 2, None, dA, None, None, None, None) == _lib.NUSI_EPARAM
        assert lm(plan._h, dR, 3, Sp, 2, datap, d, 2, None, dA, None, None, None, None) == _lib.NUSI_OK          # upper alone
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dA, (3, 2)), want[1])
    for x, y in zip(plan.limit(R, S, data, DELTA, which="both"), want):                     # the refusals changed nothing
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(plan.fit(R, S, data), want_fit):                                        # ... and fit gives what it did
        assert np.array_equal(x, y)
    plan.set_templates(None)
    for x, y in zip(plan.limit(R, S, data, DELTA, which="both"), want0):
        assert np.array_equal(x, y, equal_nan=True)
    plan.close()
