"""Limits on ensembles of pseudo-experiments on the GPU: k_toys_limit<NC> and k_toys_band
(nusi_plan_response_ensemble_limit).

Yardstick 1, bit-exact: the plan's own per-data-set call.  For every data set p, plan.limit(R, S, data[p], delta, which):
its limits and side words, stacked over p, must equal the raw outputs under np.array_equal(..., equal_nan=True) -- the
record of (p, t, q) is DEFINED as that call's, the log included --, detector.order_stat of the stack must equal the
bands, and the counted flags the tally.  Every shape here is held to it, and every shape runs again without the raw
arrays (the limits then live in the plan's scratch), with a budget that cuts the call into at least three chunks with a
partial last one, with two p-slices, and with both: all of these must agree to the bit.

Yardstick 2, the host form: detector.ensemble_limit_host's loop of limit_host with the oracle's log, at C >= 5.  The flags
and the tallies are equal.  A toy's limit lies within tests/test_limit_gpu.py's allowance, 2 eps_lambda / min |g_0| +
4 u a, of the host's; a band is held to the allowance of the toy at its rank, at the ranks at which the host's
neighbouring order statistics lie further apart than the sum of the two toys' allowances -- elsewhere the log's last
bits may decide the rank -- and at most 10 % of the ranks may be left out that way (the ensemble test's cap).  The toys
have continuous scales; tests/test_ensemble_limit.py holds on the CPU that the host form alone, at twice its own
allowance, leaves out none of these cases' ranks.

Shapes: C = 1 (groups of one lane), 5 and 17 (padded butterflies), 64 (one group per wave); K = 0, 1, 3; Q = 1, 5, 19
(partial blocks); P = 1, 3, 37; Q = 600 at C = 1 (several spectrum blocks).  Five tables (the G6 fold's three, two of
them again), so that every shape has at least five units to cut into chunks.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from nusiprop_amd.detector import (LIMIT_AT_ZERO, LIMIT_NO_FIT, LIMIT_NOT_CONVERGED, LIMIT_STEPS_MASK,
                                   LIMIT_UNBOUNDED)
from tests import test_fit_gpu, test_profile_gpu
from tests.test_ensemble_limit import _host_form_case, _sure
from tests.test_detector_gpu import (GRIDS, MAXIS, _D, _Dev, _folded, _hip, _ora_log, _plan, _spectra,
                                     nusi)  # noqa: F401  (nusi: the fixture)
from tests.test_fit_gpu import FIT_CLASSES, _fit_case, _prior_of, _templates
from tests.test_limit_gpu import _cond, _slope
from tests.test_profile_gpu import _fetch_int

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
N = GRIDS["G6"][0]
U = 2.0 ** -53
DELTA = 2.706
FLAGS = LIMIT_AT_ZERO | LIMIT_UNBOUNDED | LIMIT_NO_FIT | LIMIT_NOT_CONVERGED
NAMES = ("band_lo", "band_hi", "tally", "lo_all", "hi_all", "words_all")


def _setup(nusi, D, B, T=None, prior=None):  # noqa: F811
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    if T is not None and len(T):
        plan.set_templates(T, prior=prior)
    return plan


def _five(R):
    return np.ascontiguousarray(np.concatenate([R, R[1:2], R[0:1]]))


def _prior_for(T, C):
    K = len(T)
    if K == 0:
        return None
    return (np.full(K, 1.2), np.full(K, 0.5)) if C <= K else _prior_of(T, "mixed")     # few bins: priors determine them


def _toys(base, P, seed):
    """P data sets of different scale around base (C,): counts, some bins emptied."""
    rng = np.random.default_rng(seed)
    d = np.floor(base[None] * (0.5 + rng.random((P, len(base)))) * 10.0 ** rng.uniform(-0.7, 0.7, (P, 1)))
    d[0] = base
    return d


def _ranks(P):
    return list(range(P)) if P <= 16 else [0] + [int(r) for r in detector.band_ranks(P)] + [P - 1]


def _single(plan, R, S, data, which):
    """Yardstick 1: per data set the plan's existing call, stacked with the toy index last."""
    lo, hi, words = [], [], []
    for d in data:
        a, b, _, _, st = plan.limit(R, S, d, DELTA, which=which)
        lo.append(a)
        hi.append(b)
        words.append(st[..., 1:])
    return np.stack(lo, axis=-1), np.stack(hi, axis=-1), np.stack(words, axis=-2)


def _same(a, b, what):
    for x, y, name in zip(a, b, NAMES):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, name, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x, y, equal_nan=True), (what, name, np.argwhere(~((x == y) | ((x != x) & (y != y))))[:4])


def _qb(C):
    lg = 0
    while (1 << lg) < C:
        lg += 1
    return 256 >> lg


def _chunk_budget(ntab, Q, C, P, sides):
    """The largest budget in bytes that cuts the call into at least three chunks, the last one partial (include/nusi.h:
    a unit is one table and one block of QB spectra, QB P 8 bytes per side kept in the scratch)."""
    QB = _qb(C)
    units, per = ntab * ((Q + QB - 1) // QB), QB * P * 8 * sides
    for upc in range(units // 2, 0, -1):
        if (units + upc - 1) // upc >= 3 and units % upc:
            return upc * per
    raise AssertionError("no such budget for %d units" % units)


def _every_way(plan, R, S, data, which, what, ranks=None):
    """The call with the raw arrays against yardstick 1; then without them under every budget and slicing, bitwise equal.
    Returns the call's six arrays."""
    ntab, Q, C, P = R.shape[0], len(S), R.shape[2], len(data)
    ranks = _ranks(P) if ranks is None else ranks
    base = plan.ensemble_limit(R, S, data, DELTA, which=which, ranks=ranks, raw=True)
    assert base[2].dtype == np.int32 and base[5].dtype == np.int32
    lo, hi, words = _single(plan, R, S, data, which)
    want = (detector.order_stat(lo, ranks), detector.order_stat(hi, ranks), detector.limit_tally(words), lo, hi, words)
    _same(base, want, what + ": against the per-data-set call")
    sides = 2 if which == "both" else 1
    budget = _chunk_budget(ntab, Q, C, P, sides)
    for nbytes, ps in ((0, 0), (budget, 0), (0, 2), (budget, 2)):
        plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
        plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, ps)
        got = plan.ensemble_limit(R, S, data, DELTA, which=which, ranks=ranks)
        assert len(got) == 3
        _same(got, base[:3], "%s: no raw arrays, budget %d, p-slices %d" % (what, nbytes, ps))
        if ps:
            _same(plan.ensemble_limit(R, S, data, DELTA, which=which, ranks=ranks, raw=True), base,
                  "%s: raw arrays, p-slices %d" % (what, ps))
    plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
    plan.set_option(_lib.OPT_ENSEMBLE_PSLICES, 0)
    return base


# --- a real fold: the G6 tables, every shape, budget and slicing against the per-data-set call ------------------------
@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_ensemble_limit_equals_the_per_data_set_calls(nusi, C, K):  # noqa: F811
    R3, D, B = _folded(nusi, C)
    R = _five(R3)
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    plan = _setup(nusi, D, B, T, _prior_for(T, C))
    for Q in (1, 5, 19):
        S = _spectra(M, Q)
        base = test_fit_gpu._data(R, S, T, B, C, seed=C + Q) if K else test_profile_gpu._data(R, S, B, C, seed=C + Q)
        if C > 1:
            base[C - 1] = 0.0                               # the bin nothing ever fills
        for P in (1, 3, 37):
            data = _toys(base, P, seed=Q + P)
            what = "G6 C=%d K=%d Q=%d P=%d" % (C, K, Q, P)
            got = _every_way(plan, R, S, data, "both", what)
            assert got[0].shape == (5, Q, len(_ranks(P))) and got[3].shape == (5, Q, P) and got[5].shape == (5, Q, P, 2)
            for x in got:                                   # tables 3 and 4 are tables 1 and 0 again
                assert np.array_equal(x[3], x[1], equal_nan=True) and np.array_equal(x[4], x[0], equal_nan=True)
            if Q == 5 and P == 3:                           # one side alone: its bits, the other side NaN / 0
                for which, mine, other in (("upper", (1, 4), (0, 3)), ("lower", (0, 3), (1, 4))):
                    one = _every_way(plan, R, S, data, which, what + " " + which)
                    side = 1 if which == "upper" else 0
                    assert all(np.array_equal(one[i], got[i]) for i in mine)
                    assert all(np.all(np.isnan(one[i])) for i in other)
                    assert np.array_equal(one[5][..., side], got[5][..., side]) and not one[5][..., 1 - side].any()
                    assert np.array_equal(one[2][:, :, side], got[2][:, :, side]) and not one[2][:, :, 1 - side].any()
    plan.close()


# --- several spectrum blocks per table ---------------------------------------------------------------------------------------
def test_many_spectra_on_one_bin(nusi):  # noqa: F811
    """Q = 600 at C = 1: 256 chains a block, three blocks per table, a partial last one; no templates."""
    C, Q = 1, 600
    R3, D, B = _folded(nusi, C)
    plan = _setup(nusi, D, B)
    data = np.array([[9.0], [2.0], [40.0]])
    got = _every_way(plan, _five(R3), _spectra(M, Q), data, "both", "G6 C=1 Q=600 K=0")
    assert np.all(np.isfinite(got[1]))
    plan.close()


# --- searches that part ways inside a wave and across the data sets ------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_searches_that_part_ways_across_data_sets(nusi, C):  # noqa: F811
    """test_fit_gpu's classes, whose fits and searches stop after different numbers of steps inside a wave, with three
    data rows of different scale: the per-toy state is set anew for every data set."""
    plan = _plan(nusi, "G6")
    D = _D(C, N)
    differ = parted = False
    for what, decades, bkind, pkind, K in FIT_CLASSES[::2] + FIT_CLASSES[7:]:
        R, S, data, T, prior, B = _fit_case(C, what, decades, bkind, pkind, K, ntab=5, Q=24)
        plan.set_detector(D, background=B)
        plan.set_templates(T, prior=prior)
        rows = np.stack([data, np.floor(0.05 * data), 7.0 * data + 1.0])
        got = _every_way(plan, R, S, rows, "both", "C=%d K=%d %s" % (C, K, what))
        words = got[5]
        differ |= len({words[:, :, p].tobytes() for p in range(3)}) > 1
        steps = words[..., 1] & LIMIT_STEPS_MASK             # the upper side's outer steps (ntab, Q, P)
        parted |= any(len(set(steps[t, q0:q0 + 4, p].tolist())) > 1 for t in range(5) for q0 in range(0, 24, 4) for p in range(3))
    plan.close()
    assert differ and parted


# --- zeros, weak toys and a singular class ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 2))
def test_zeros_and_weak_toys(nusi, K):  # noqa: F811
    """Spectra of zeros beside live ones (unbounded: the band is +inf, the tally counts every toy), a toy of zeros, and
    background-only toys so weak that the lower limit is at zero (AT_ZERO)."""
    C, Q, P = 5, 7, 6
    R3, D, B = _folded(nusi, C)
    S = np.array(_spectra(M, Q))
    S[2] = 0.0
    S[4] = 0.0
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    data = detector.pseudo_data(T.sum(axis=0) + B, P, np.random.default_rng(K + 1))
    data[:, C - 1] = 0.0
    data[3] = 0.0
    plan = _setup(nusi, D, B, T, _prior_for(T, C))
    blo, bhi, tally, lo, hi, words = _every_way(plan, _five(R3), S, data, "both", "zeros, K=%d" % K)
    plan.close()
    live = np.array([0, 1, 3, 5, 6])
    assert np.all(np.isinf(bhi[:, [2, 4]])) and np.all(tally[:, [2, 4], 1, 1] == P) and np.all(tally[:, [2, 4], 0, 1] == P)
    assert not tally[:, live, :, 1].any() and not np.any(np.isinf(hi[:, live]))
    assert np.all(tally[:, :, 0, 0] >= 1) and np.all(lo[:, :, 3] == 0.0)         # the toy of zeros: a_lo = 0
    assert np.all(blo[:, :, 0] == 0.0)
    assert np.any((words[:, live, :, 0] & LIMIT_AT_ZERO) != 0)


def test_a_singular_class(nusi):  # noqa: F811
    """Two identical templates without priors: the best fit is singular, the limits are NaN (NO_FIT) and sort behind the
    numbers; a toy of zeros is fitted at the boundary without a solve and has limits."""
    C, Q = 5, 5
    R3, D, B = _folded(nusi, C)
    S = _spectra(M, Q)
    T1 = _templates(C, 1, scale=20.0)
    T = np.concatenate([T1, T1])
    mean = 2.0 * T1[0] + B
    data = np.stack([np.floor(3.0 * mean), np.zeros(C), np.floor(5.0 * mean)])
    data[:, C - 1] = 0.0
    plan = _setup(nusi, D, B, T, None)
    blo, bhi, tally, lo, hi, words = _every_way(plan, _five(R3), S, data, "both", "singular")
    plan.close()
    nofit = (words[..., 1] & LIMIT_NO_FIT) != 0
    assert nofit.any() and not nofit.all()
    assert np.array_equal(np.isnan(hi), nofit) and np.array_equal(tally[:, :, 1, 2], nofit.sum(axis=-1))
    assert np.array_equal(tally[:, :, 0, 2], tally[:, :, 1, 2])
    n = nofit.sum(axis=-1)
    for t in range(5):
        for q in range(Q):
            assert np.all(np.isnan(bhi[t, q, 3 - n[t, q]:])) and not np.any(np.isnan(bhi[t, q, :3 - n[t, q]]))


# --- the host form ---------------------------------------------------------------------------------------------------------------
def _host(R, S, data, T, prior, B, log):
    """ensemble_limit_host's loop, keeping limit_host's details: (lo, hi (ntab, Q, P), words (ntab, Q, P, 2), eps, h
    (ntab, Q, P, 2))."""
    lo, hi, words, eps, h = [], [], [], [], []
    for d in data:
        det = {}
        a, b, _, _, st = detector.limit_host(R, S, d, DELTA, "both", templates=T, prior=prior, background=B, log=log, details=det)
        lo.append(a)
        hi.append(b)
        words.append(st[..., 1:])
        eps.append(det["eps"])
        h.append(det["h"])
    return np.stack(lo, -1), np.stack(hi, -1), np.stack(words, -2), np.stack(eps, -2), np.stack(h, -2)


@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (5, 17, 64))
def test_ensemble_limit_against_the_host_form(nusi, oracle_mod, C, K):  # noqa: F811
    log = _ora_log(oracle_mod)
    R, S, T, B, data, prior = _host_form_case(C, K)
    ntab, Q, P = R.shape[0], len(S), len(data)
    plan = _setup(nusi, _D(C, N), B, T, prior)
    ranks = list(range(P))
    blo, bhi, tally, lo, hi, words = plan.ensemble_limit(R, S, data, DELTA, which="both", ranks=ranks, raw=True)
    Tk = T if K else None
    hlo, hhi, hwords, eps, hh = _host(R, S, data, Tk, prior, B, log)
    assert np.array_equal(words & FLAGS, hwords & FLAGS)
    assert np.array_equal(tally, detector.limit_tally(hwords))
    left_out = total = toys_off = 0
    worst = 0.0
    for side, (g, h, band) in enumerate(((lo, hlo, blo), (hi, hhi, bhi))):
        word = words[..., side]
        live = np.isfinite(h) & (word & LIMIT_STEPS_MASK > 0) & ((word & (LIMIT_AT_ZERO | LIMIT_NOT_CONVERGED)) == 0)
        assert np.array_equal(g[~live], h[~live], equal_nan=True)                 # NaN, +inf and the zeros
        tol = np.zeros(h.shape)
        for p in range(P):
            lv = live[..., p]
            if not lv.any():
                continue
            ag, ah = np.where(lv, g[..., p], 1.0), np.where(lv, h[..., p], 1.0)
            _, mug, _ = _cond(plan, R, S, ag, data[p], K)
            _, muh, _ = _cond(plan, R, S, ah, data[p], K)
            g0 = np.minimum(np.abs(_slope(R, S, ag, mug, data[p])), np.abs(_slope(R, S, ah, muh, data[p])))
            tol[..., p] = np.where(lv, 2.0 * eps[..., p, side] / g0 + 4 * U * np.abs(h[..., p]), 0.0)
        with np.errstate(invalid="ignore"):
            off = live & ~(np.abs(g - h) <= tol)
        near = np.abs(np.abs(hh[..., side]) - eps[..., side]) <= 2.0 * eps[..., side]      # (test_limit_gpu's rule)
        assert not np.any(off & ~near), (side, np.argwhere(off & ~near)[:4])
        toys_off += int(off.sum())
        for t in range(ntab):
            for q in range(Q):
                order = np.argsort(h[t, q], kind="stable")                         # (NaN last, behind +inf)
                hs, ts = h[t, q][order], tol[t, q][order]
                assert np.array_equal(hs, detector.order_stat(h[t, q], ranks), equal_nan=True)
                sure = _sure(hs, ts) & ~off[t, q].any()                  # (a toy beyond its allowance: none of its ranks)
                total += P
                left_out += int((~sure).sum())
                for r in np.flatnonzero(sure):
                    if ts[r] == 0.0:
                        assert np.array_equal(band[t, q, r], hs[r], equal_nan=True), (side, t, q, r)
                    else:
                        assert abs(band[t, q, r] - hs[r]) <= ts[r], (side, t, q, r, band[t, q, r], hs[r], ts[r])
                        worst = max(worst, abs(band[t, q, r] - hs[r]) / ts[r])
    plan.close()
    print("synthetic C=%d K=%d: %d of %d ranks left out, %d toys beyond their allowance, worst ratio %.3f" % (
        C, K, left_out, total, toys_off, worst))
    assert left_out <= 0.1 * total, (left_out, total)


# --- NR = 0 and the device form ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 3))
def test_device_form_and_the_tally_alone(nusi, K):  # noqa: F811
    C, Q, P = 17, 19, 5
    R3, D, B = _folded(nusi, C)
    R = _five(R3)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0) if K else np.zeros((0, C))
    base = test_fit_gpu._data(R, S, T, B, C, seed=2)
    base[C - 1] = 0.0
    data = _toys(base, P, seed=4)
    plan = _setup(nusi, D, B, T, _prior_for(T, C))
    ranks = [4, 0, 2, 2]
    want = plan.ensemble_limit(R, S, data, DELTA, which="both", ranks=ranks, raw=True)
    blo, bhi, tally, lo, hi, words = want
    none = plan.ensemble_limit(R, S, data, DELTA, which="both", ranks=[])          # NR = 0: the tally alone
    assert none[0].shape == none[1].shape == (5, Q, 0) and np.array_equal(none[2], tally)
    H = _hip()
    with _Dev(H) as dev:                            # into NaN / -1 filled buffers, each optional output NULL in turn
        dR = dev.alloc(R.nbytes, np.ascontiguousarray(R))
        for nbytes in (0, _chunk_budget(5, Q, C, P, 2)):
            plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, nbytes)
            for skip in (None, "tally", "lo_all", "hi_all", "words_all", "raw", "band_lo", "band_hi", "bands"):
                ptr = {}
                for name, x in zip(NAMES, want):
                    fill = np.full(x.shape, -1, dtype=np.int32) if x.dtype == np.int32 else np.full(x.shape, np.nan)
                    ptr[name] = dev.alloc(x.nbytes, fill)
                gone = {"raw": ("lo_all", "hi_all", "words_all"), "bands": ("band_lo", "band_hi")}.get(skip, (skip,))
                which = {"band_lo": "upper", "band_hi": "lower"}.get(skip, "both")
                side = 0 if which == "lower" else 1             # (the side asked for, where only one is)
                r = [] if skip == "bands" else ranks
                args = [None if n in gone else ptr[n] for n in NAMES]
                assert plan.ensemble_limit_device(dR, 5, S, data, DELTA, which, r, *args) == (Q, P, len(r))
                assert H.hipDeviceSynchronize() == 0
                for name, x in zip(NAMES, want):
                    got = _fetch_int(H, ptr[name], x.shape) if x.dtype == np.int32 else dev.fetch(ptr[name], x.shape)
                    if name in gone:
                        assert np.all(got == -1) if x.dtype == np.int32 else np.all(np.isnan(got)), (nbytes, skip, name)
                    elif which != "both" and name == ("lo_all", "hi_all")[1 - side]:
                        assert np.all(np.isnan(got)), (nbytes, skip, name)
                    elif which != "both" and name == "words_all":
                        assert np.array_equal(got[..., side], x[..., side]) and not got[..., 1 - side].any(), (nbytes, skip, name)
                    elif which != "both" and name == "tally":
                        assert np.array_equal(got[:, :, side], x[:, :, side]) and not got[:, :, 1 - side].any(), (nbytes, skip, name)
                    else:
                        assert np.array_equal(got, x, equal_nan=True), (nbytes, skip, name)
    plan.close()


# --- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals(nusi):  # noqa: F811
    L = _lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    C, K, P, NR = 5, 2, 3, 2
    R, D, B = _folded(nusi, C)
    S = _spectra(M, 2)
    data = np.full((P, C), 30.0) * np.array([[1.0], [0.5], [2.0]])
    T = _templates(C, K)
    plan = _plan(nusi, "G6")

    def refused(code, f, *a, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*a, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    ranks = np.array([0, 2], dtype=np.int32)
    Sp, datap, rp = S.ctypes.data_as(dp), data.ctypes.data_as(dp), ranks.ctypes.data_as(ip)
    refused(_lib.NUSI_ESTATE, plan.ensemble_limit, np.ones((1, M, C)), S, data, DELTA)                # no detector
    el = L.nusi_plan_response_ensemble_limit
    d = ctypes.c_double(DELTA)
    assert el(plan._h, None, 1, Sp, 2, datap, P, d, 2, rp, NR, None, None, None, None, None, None, None) == _lib.NUSI_ESTATE
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=([1.0, 1.0], [np.inf, 0.5]))
    want_limit = plan.limit(R, S, data[0], DELTA, which="both")
    want_ens = plan.ensemble(R, S, data)
    want = plan.ensemble_limit(R, S, data, DELTA, which="both", raw=True)
    for bad in (0.0, -1.0, np.nan, np.inf):
        refused(_lib.NUSI_EPARAM, plan.ensemble_limit, R, S, data, bad)                                # delta
    for bad in (0, 4, -1):
        refused(_lib.NUSI_EPARAM, plan.ensemble_limit, R, S, data, DELTA, which=bad)
    for bad in ([P], [-1], [0, 1, P], list(range(3)) * 6):                                            # a rank, NR = 18
        refused(_lib.NUSI_EPARAM, plan.ensemble_limit, R, S, data, DELTA, ranks=bad)
    for bad in (-1.0, np.nan, np.inf):
        db, Sb = data.copy(), np.array(S)
        db[P - 1, C - 1] = bad                                                                        # (in the last data row)
        Sb[1, M - 1] = bad
        refused(_lib.NUSI_EPARAM, plan.ensemble_limit, R, S, db, DELTA)
        refused(_lib.NUSI_EPARAM, plan.ensemble_limit, R, Sb, data, DELTA)
    with pytest.raises(ValueError):
        plan.ensemble_limit(R[:, :-1], S, data, DELTA)
    with pytest.raises(ValueError):
        plan.ensemble_limit(R, S, data[:, :-1], DELTA)
    with pytest.raises(ValueError):
        plan.ensemble_limit(R, S, data[:0], DELTA)
    for opt, top in ((_lib.OPT_ENSEMBLE_LIMIT_MB, 1 << 20), (_lib.OPT_ENSEMBLE_LIMIT_BYTES, 1 << 30)):
        refused(_lib.NUSI_EPARAM, plan.set_option, opt, -1)
        refused(_lib.NUSI_EPARAM, plan.set_option, opt, top + 1)
    plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, _qb(C) * P * 8 * 2 - 1)                            # one byte short of a unit
    refused(_lib.NUSI_EPARAM, plan.ensemble_limit, R, S, data, DELTA, which="both")
    assert "NUSI_OPT_ENSEMBLE_LIMIT" in _lib.last_error()
    _same(plan.ensemble_limit(R, S, data, DELTA, which="both", raw=True), want, "the raw arrays need no scratch")
    plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, _qb(C) * P * 8 * 2)                                # exactly one unit: three chunks
    _same(plan.ensemble_limit(R, S, data, DELTA, which="both"), want[:3], "a budget of one unit")
    plan.set_option(_lib.OPT_ENSEMBLE_LIMIT_BYTES, 0)
    H = _hip()
    with _Dev(H) as dev:
        dR, dL, dH = dev.alloc(R.nbytes, np.ascontiguousarray(R)), dev.alloc(3 * 2 * NR * 8), dev.alloc(3 * 2 * NR * 8)
        dT = dev.alloc(3 * 2 * 8 * 4)
        E = _lib.NUSI_EPARAM
        tail = (None, None, None, None)
        assert el(plan._h, None, 3, Sp, 2, datap, P, d, 3, rp, NR, dL, dH, dT, *tail) == E           # NULL d_R
        assert el(plan._h, dR, 3, None, 2, datap, P, d, 3, rp, NR, dL, dH, dT, *tail) == E           # NULL S
        assert el(plan._h, dR, 3, Sp, 2, None, P, d, 3, rp, NR, dL, dH, dT, *tail) == E              # NULL data
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 3, None, NR, dL, dH, dT, *tail) == E           # NULL rank with NR > 0
        assert el(plan._h, dR, 3, Sp, 2, datap, 0, d, 3, rp, NR, dL, dH, dT, *tail) == E             # P outside 1 .. the maximum
        assert el(plan._h, dR, 3, Sp, 2, datap, _lib.BAND_DATASETS_MAX + 1, d, 3, rp, NR, dL, dH, dT, *tail) == E
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 3, rp, -1, dL, dH, dT, *tail) == E             # NR
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 3, rp, _lib.BAND_RANKS_MAX + 1, dL, dH, dT, *tail) == E
        assert el(plan._h, dR, 0, Sp, 2, datap, P, d, 3, rp, NR, dL, dH, dT, *tail) == E
        assert el(plan._h, dR, 3, Sp, 0, datap, P, d, 3, rp, NR, dL, dH, dT, *tail) == E
        assert el(plan._h, dR, 3, Sp, (1 << 19) + 1, datap, P, d, 3, rp, NR, dL, dH, dT, *tail) == E
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 3, rp, NR, None, dH, dT, *tail) == E           # no band of a side asked for
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 3, rp, NR, dL, None, dT, *tail) == E
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 2, rp, NR, dL, None, dT, *tail) == E
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 3, None, 0, dL, dH, None, *tail) == E          # NR = 0: nothing to do
        assert el(plan._h, dR, 3, Sp, 2, datap, P, d, 2, rp, NR, None, dH, None, *tail) == _lib.NUSI_OK   # upper alone
        assert H.hipDeviceSynchronize() == 0
        assert np.array_equal(dev.fetch(dH, (3, 2, NR)), detector.order_stat(want[4], ranks))
    # the refusals changed nothing: the call, the limit and the ensemble return what they did
    _same(plan.ensemble_limit(R, S, data, DELTA, which="both", raw=True), want, "after the refusals")
    for x, y in zip(plan.limit(R, S, data[0], DELTA, which="both"), want_limit):
        assert np.array_equal(x, y, equal_nan=True)
    for x, y in zip(plan.ensemble(R, S, data), want_ens):
        assert np.array_equal(x, y, equal_nan=True)
    plan.close()
