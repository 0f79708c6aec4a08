"""The host form of the ensemble limit (CPU, numpy only): detector.order_stat -- the band's rule of
nusi_plan_response_ensemble_limit, the order statistics under the key (isnan(x), x) --, detector.band_ranks -- the
inverted empirical CDF --, detector.ensemble_limit_host -- a loop of limit_host over the data sets, then order_stat and
the tally of the side words -- and the new symbols of the built library.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import LIMIT_AT_ZERO, LIMIT_NO_FIT, LIMIT_NOT_CONVERGED, LIMIT_UNBOUNDED

INF, NAN = np.inf, np.nan
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA = 2.706


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _key(v):
    return (True, 0.0) if np.isnan(v) else (False, float(v))


# --- order_stat: the key (isnan, x) ---------------------------------------------------------------------------------------
def test_order_stat_nan_sorts_after_infinity():
    x = [3.0, NAN, INF, 0.0, NAN, 1.5]
    got = detector.order_stat(x, range(6))
    assert np.array_equal(got, [0.0, 1.5, 3.0, INF, NAN, NAN], equal_nan=True)
    assert np.array_equal(detector.order_stat([NAN, NAN, NAN], [0, 2]), [NAN, NAN], equal_nan=True)     # all NaN
    assert np.array_equal(detector.order_stat([INF, INF], [0, 1]), [INF, INF])


def test_order_stat_ties_one_toy_and_duplicate_ranks():
    assert np.array_equal(detector.order_stat([2.0, 1.0, 2.0, 1.0, 2.0], [0, 1, 2, 3, 4]), [1.0, 1.0, 2.0, 2.0, 2.0])
    assert np.array_equal(detector.order_stat([7.0], [0]), [7.0])                                     # P = 1
    assert np.array_equal(detector.order_stat([7.0], [0, 0, 0]), [7.0, 7.0, 7.0])
    assert np.array_equal(detector.order_stat([5.0, 4.0, 6.0], [2, 0, 2, 1, 0]), [6.0, 4.0, 6.0, 5.0, 4.0])
    assert detector.order_stat([5.0, 4.0], []).shape == (0,)                                          # no rank: an empty band
    for bad in ([-1], [2], [0, 5]):
        with pytest.raises(ValueError):
            detector.order_stat([5.0, 4.0], bad)
    with pytest.raises(ValueError):
        detector.order_stat(np.zeros((3, 0)), [0])


def test_order_stat_over_every_axis_equals_the_sort():
    rng = np.random.default_rng(11)
    x = rng.random((4, 5, 6))
    x[rng.random(x.shape) < 0.2] = INF
    x[rng.random(x.shape) < 0.2] = NAN
    x[rng.random(x.shape) < 0.2] = 0.0                              # ties
    for axis in (0, 1, 2, -1, -2):
        n = x.shape[axis]
        r = [n - 1, 0, n // 2, 0]
        got = detector.order_stat(x, r, axis=axis)
        want = np.sort(np.moveaxis(x, axis, -1))[..., r]
        assert got.shape == want.shape == tuple(np.delete(x.shape, axis)) + (4,)
        assert np.array_equal(_bits(got), _bits(want))
        # the definition: at most r entries before v under the key, more than r before or equal to it
        flat, g = np.moveaxis(x, axis, -1).reshape(-1, n), got.reshape(-1, 4)
        for row, vs in zip(flat, g):
            keys = [_key(v) for v in row]
            for rk, v in zip(r, vs):
                assert sum(k < _key(v) for k in keys) <= rk < sum(k <= _key(v) for k in keys)


def test_order_stat_does_not_depend_on_the_order_of_the_input():
    rng = np.random.default_rng(12)
    x = np.floor(rng.random((3, 41)) * 8.0)
    x[:, ::7] = INF
    x[:, 3::11] = NAN
    r = detector.band_ranks(41)
    want = detector.order_stat(x, r)
    for seed in range(3):
        perm = np.random.default_rng(seed).permutation(41)
        assert np.array_equal(_bits(detector.order_stat(x[:, perm], r)), _bits(want))


# --- band_ranks: the inverted empirical CDF -------------------------------------------------------------------------------
def test_band_ranks():
    assert np.array_equal(detector.band_ranks(1), [0, 0, 0, 0, 0]) and detector.band_ranks(1).dtype == np.int32
    assert np.array_equal(detector.band_ranks(37), [0, 5, 18, 31, 36])
    assert np.array_equal(detector.band_ranks(1000), [24, 159, 499, 839, 974])
    assert np.array_equal(detector.band_ranks(10, probs=(0.0, 1.0, 0.1, 0.11)), [0, 9, 0, 1])
    for bad in (0, -3):
        with pytest.raises(ValueError):
            detector.band_ranks(bad)
    for bad in ((-0.1,), (1.5,), (NAN,)):
        with pytest.raises(ValueError):
            detector.band_ranks(5, probs=bad)


def test_band_ranks_against_numpy_quantile():
    try:
        np.quantile([1.0, 2.0], 0.5, method="inverted_cdf")
    except TypeError:
        pytest.skip("this numpy has no quantile method 'inverted_cdf'")
    probs = (0.025, 0.16, 0.5, 0.84, 0.975)
    for P in (1, 2, 3, 16, 37, 100, 256, 1001):
        x = np.random.default_rng(P).random(P)
        got = detector.order_stat(x, detector.band_ranks(P, probs))
        assert np.array_equal(got, np.quantile(x, probs, method="inverted_cdf")), P


# --- ensemble_limit_host ---------------------------------------------------------------------------------------------------
M, C, NTAB, Q, P = 6, 5, 2, 6, 5


def _case(seed=1):
    rng = np.random.default_rng(seed)
    R = rng.random((NTAB, M, C)) * 10.0 ** rng.uniform(-1, 1, (NTAB, 1, 1))
    S = rng.random((Q, M)) * 10.0 ** rng.uniform(-1, 1, (Q, 1))
    S[3] = 0.0                                                      # a spectrum of zeros: unbounded
    B = 0.5 + rng.random(C)
    T = np.stack([(1.0 + j) * np.exp(-(0.5 + 0.4 * j) * np.linspace(0.0, 3.0, C)) for j in range(3)]) * 5.0
    return R, S, B, T


def _toys(T, B, K, seed):
    """Background-only toys, one of them of zeros and one with a strong excess (a two-sided interval)."""
    mean = T[:K].sum(axis=0) + B
    data = detector.pseudo_data(mean, P, np.random.default_rng(seed))
    data[2] = 0.0
    data[4] = np.floor(40.0 * mean)
    return data


def _loop(R, S, data, which, T, prior, B):
    """The definition: limit_host per data set, stacked with the toy index last."""
    lo, hi, words = [], [], []
    for d in data:
        a, b, _, _, st = detector.limit_host(R, S, d, DELTA, which=which, templates=T, prior=prior, background=B)
        lo.append(a)
        hi.append(b)
        words.append(st[..., 1:])
    return np.stack(lo, axis=-1), np.stack(hi, axis=-1), np.stack(words, axis=-2)


@pytest.mark.parametrize("which", ("upper", "lower", "both"))
@pytest.mark.parametrize("K", (0, 1, 3))
def test_host_form_equals_the_loop_of_limits(K, which):
    R, S, B, T = _case()
    Tk = T[:K] if K else None
    prior = (np.full(K, 1.0), np.full(K, 0.5)) if K else None
    data = _toys(T, B, K, seed=K + 2)
    ranks = [0, 2, 4, 2]
    blo, bhi, tally, lo_all, hi_all, words = detector.ensemble_limit_host(R, S, data, DELTA, which=which, ranks=ranks,
                                                                          templates=Tk, prior=prior, background=B, raw=True)
    assert blo.shape == bhi.shape == (NTAB, Q, 4) and tally.shape == (NTAB, Q, 2, 4) and tally.dtype == np.int32
    assert lo_all.shape == hi_all.shape == (NTAB, Q, P) and words.shape == (NTAB, Q, P, 2) and words.dtype == np.int32
    wlo, whi, wwords = _loop(R, S, data, which, Tk, prior, B)
    assert np.array_equal(_bits(lo_all), _bits(wlo)) and np.array_equal(_bits(hi_all), _bits(whi))
    assert np.array_equal(words, wwords)
    assert np.array_equal(_bits(blo), _bits(detector.order_stat(wlo, ranks)))
    assert np.array_equal(_bits(bhi), _bits(detector.order_stat(whi, ranks)))
    for k, flag in enumerate((LIMIT_AT_ZERO, LIMIT_UNBOUNDED, LIMIT_NO_FIT, LIMIT_NOT_CONVERGED)):
        assert np.array_equal(tally[..., k], np.count_nonzero(words & flag, axis=2)), k      # the counts of the raw words
    assert np.array_equal(tally, detector.limit_tally(words))
    if which != "lower":
        assert np.all(np.isinf(bhi[:, 3])) and np.all(tally[:, 3, 1, 1] == P)               # zeros: unbounded, so +inf
        live = np.delete(np.arange(Q), 3)
        assert np.all(np.isfinite(bhi[:, live])) and np.all(bhi[:, live, 0] <= bhi[:, live, 1])
    else:
        assert np.all(np.isnan(bhi)) and np.all(np.isnan(hi_all)) and not words[..., 1].any() and not tally[:, :, 1].any()
    if which != "upper":
        assert np.all(lo_all[:, :, 2] == 0.0) and np.all(words[:, :, 2, 0] & LIMIT_AT_ZERO)  # the toy of zeros: a_lo = 0
        assert np.all(tally[:, :, 0, 0] >= 1)
        assert np.any(lo_all[:, :, 4] > 0.0)                                                # the excess: a two-sided interval
    else:
        assert np.all(np.isnan(blo)) and np.all(np.isnan(lo_all)) and not words[..., 0].any() and not tally[:, :, 0].any()
    # without raw: the first three; ranks = None: band_ranks(P)
    three = detector.ensemble_limit_host(R, S, data, DELTA, which=which, templates=Tk, prior=prior, background=B)
    assert len(three) == 3 and three[0].shape == (NTAB, Q, 5)
    assert np.array_equal(_bits(three[1]), _bits(detector.order_stat(whi, detector.band_ranks(P))))
    assert np.array_equal(three[2], tally)


def test_host_form_with_one_toy_and_shapes_of_one():
    R, S, B, T = _case(seed=2)
    d = _toys(T, B, 0, seed=3)[0]
    blo, bhi, tally, lo_all, hi_all, words = detector.ensemble_limit_host(R[0], S[1], d, DELTA, which="both", background=B,
                                                                          raw=True)
    lo, hi, _, _, st = detector.limit_host(R[0], S[1], d, DELTA, which="both", background=B)
    assert blo.shape == (1, 1, 5) and lo_all.shape == (1, 1, 1) and words.shape == (1, 1, 1, 2)
    assert np.all(blo == lo) and np.all(bhi == hi) and lo_all[0, 0, 0] == lo and hi_all[0, 0, 0] == hi   # P = 1: every rank
    assert np.array_equal(words[0, 0, 0], np.reshape(st, 3)[1:])


def test_a_singular_best_fit_sorts_last_and_is_counted():
    """Two identical templates without priors: the data do not determine them, the fit's system is singular and the
    limits are NaN (NO_FIT).  A toy of zeros is fitted at the boundary without a solve and has limits: the class holds
    both kinds of record, so NaN must sort behind numbers and behind the +inf of the spectrum of zeros."""
    R, S, B, T = _case(seed=5)
    T2 = np.stack([T[0], T[0]])
    data = np.stack([np.floor(3.0 * (2.0 * T[0] + B)), np.zeros(C), np.floor(5.0 * (2.0 * T[0] + B))])
    blo, bhi, tally, lo_all, hi_all, words = detector.ensemble_limit_host(R, S, data, DELTA, which="both", ranks=[0, 1, 2],
                                                                          templates=T2, background=B, raw=True)
    nofit = (words[..., 1] & LIMIT_NO_FIT) != 0
    assert nofit.any() and not nofit.all()
    assert np.array_equal(np.isnan(hi_all), nofit) and np.array_equal(tally[:, :, 1, 2], nofit.sum(axis=-1))
    n = nofit.sum(axis=-1)                                          # NaN last: the top n ranks of the band, and only they
    for t in range(NTAB):
        for q in range(Q):
            assert np.all(np.isnan(bhi[t, q, 3 - n[t, q]:])) and not np.any(np.isnan(bhi[t, q, :3 - n[t, q]]))
    assert np.all(np.isinf(bhi[:, 3, 0]) | np.isnan(bhi[:, 3, 0]))  # ... +inf of the spectrum of zeros before them


def test_host_form_refusals():
    R, S, B, T = _case(seed=4)
    data = _toys(T, B, 0, seed=1)
    for bad in (data[:, :-1], data[None], np.zeros((0, C))):
        with pytest.raises(ValueError):
            detector.ensemble_limit_host(R, S, bad, DELTA, background=B)
    with pytest.raises(ValueError):
        detector.ensemble_limit_host(R, S[:, :-1], data, DELTA, background=B)
    for bad in (-1.0, NAN, INF):
        d = data.copy()
        d[2, 1] = bad
        with pytest.raises(ValueError):
            detector.ensemble_limit_host(R, S, d, DELTA, background=B)
    for bad in ([P], [-1], [0, 99]):
        with pytest.raises(ValueError):
            detector.ensemble_limit_host(R, S, data, DELTA, ranks=bad, background=B)
    for bad in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            detector.ensemble_limit_host(R, S, data, bad, background=B)
    with pytest.raises(ValueError):
        detector.ensemble_limit_host(R, S, data, DELTA, which="middle", background=B)


# --- the host-form comparison of tests/test_ensemble_limit_gpu.py: its cases and its rule, checked here first -----------------
def _host_form_case(C, K):
    """(R, S, T, B, data, prior) of the GPU test's host-form comparison: synthetic matrices, background-only toys of
    continuous scales (no two toys alike, so no two limits tie)."""
    from tests.test_fit_gpu import _prior_of, _templates
    from tests.test_profile_gpu import _synthetic
    ntab, Q, P = 3, 5, 8
    R, S = _synthetic(C, ntab, Q, seed=5, decades=False)
    rng = np.random.default_rng(C + K)
    T = _templates(C, K, scale=50.0) if K else np.zeros((0, C))
    B = 30.0 * (0.5 + rng.random(C))
    base = T.sum(axis=0) + B
    r2 = np.random.default_rng(C + K)
    data = np.floor(base[None] * (0.5 + r2.random((P, C))) * 10.0 ** r2.uniform(-0.7, 0.7, (P, 1)))
    data[0] = base
    prior = None if K == 0 else ((np.full(K, 1.2), np.full(K, 0.5)) if C <= K else _prior_of(T, "mixed"))
    return R, S, T, B, data, prior


def _sure(hs, ts):
    """Ranks whose sorted host value hs[r] keeps its rank whatever the toys do within their allowances ts: its interval
    hs[r] -+ ts[r] meets no other toy's (two exact records, allowance 0 each, keep their order whatever their distance;
    NaN and +inf are exact and behind every number)."""
    P = len(hs)
    lo = np.where(np.isnan(hs), np.inf, hs - ts)
    hi = np.where(np.isnan(hs), np.inf, hs + ts)
    ok = np.ones(P, dtype=bool)
    for r in range(P):
        for j in range(P):
            if j != r and not (ts[r] == 0.0 and ts[j] == 0.0) and not (hi[j] < lo[r] or hi[r] < lo[j]):
                ok[r] = False
    return ok



@pytest.mark.parametrize("K", (0, 1, 3))
@pytest.mark.parametrize("C", (5, 17, 64))
def test_the_host_form_alone_leaves_no_rank_uncertain(C, K):
    """On the GPU test's cases the host's own order statistics lie further apart than TWICE the limit test's allowance,
    2 eps_lambda / |g_0| + 4 u a, of the toys involved (the slope here is the host's own at its limit): the device
    comparison there can hold every rank, and its 10 % cap has room."""
    R, S, T, B, data, prior = _host_form_case(C, K)
    ntab, Q, P = R.shape[0], len(S), len(data)
    lo, hi, words, eps, g0 = [], [], [], [], []
    for d in data:
        det = {}
        a, b, _, _, st = detector.limit_host(R, S, d, DELTA, "both", templates=T if K else None, prior=prior, background=B,
                                             details=det)
        lo.append(a)
        hi.append(b)
        words.append(st[..., 1:])
        eps.append(det["eps"])
        g0.append(det["g0"])
    lo, hi, words, eps, g0 = np.stack(lo, -1), np.stack(hi, -1), np.stack(words, -2), np.stack(eps, -2), np.stack(g0, -2)
    assert not np.any(words & (LIMIT_NO_FIT | LIMIT_NOT_CONVERGED))
    left_out = 0
    for side, h in enumerate((lo, hi)):
        w = words[..., side]
        live = np.isfinite(h) & (w & detector.LIMIT_STEPS_MASK > 0) & ((w & (LIMIT_AT_ZERO | LIMIT_NOT_CONVERGED)) == 0)
        with np.errstate(all="ignore"):
            tol = np.where(live, 2.0 * (2.0 * eps[..., side] / np.abs(g0[..., side]) + 4 * 2.0 ** -53 * np.abs(h)), 0.0)
        for t in range(ntab):
            for q in range(Q):
                order = np.argsort(h[t, q], kind="stable")
                left_out += int((~_sure(h[t, q][order], tol[t, q][order])).sum())
    assert left_out == 0, left_out


# --- the library ---------------------------------------------------------------------------------------------------------------
def test_abi():
    """The header's constants are the package's; the new calls are declared, bound and exported; without a plan they
    refuse, and the options are known."""
    from nusiprop_amd import _lib
    text = open(os.path.join(ROOT, "include", "nusi.h")).read()
    macro = {k: int(v, 0) for k, v in re.findall(r"^#define (NUSI_[A-Z_]+) (\d+)$", text, flags=re.M)}
    assert macro["NUSI_BAND_RANKS_MAX"] == _lib.BAND_RANKS_MAX == 16
    assert macro["NUSI_BAND_DATASETS_MAX"] == _lib.BAND_DATASETS_MAX == 4096
    assert macro["NUSI_OPT_ENSEMBLE_LIMIT_MB"] == _lib.OPT_ENSEMBLE_LIMIT_MB
    assert macro["NUSI_OPT_ENSEMBLE_LIMIT_BYTES"] == _lib.OPT_ENSEMBLE_LIMIT_BYTES
    opts = [v for k, v in macro.items() if k.startswith("NUSI_OPT_")]
    assert len(opts) == len(set(opts))
    L = _lib.load()
    for name in ("nusi_plan_response_ensemble_limit", "nusi_plan_response_ensemble_limit_host"):
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name).argtypes is not None
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    one, r = np.ones(4), np.zeros(1, dtype=np.int32)
    p, rp = one.ctypes.data_as(dp), r.ctypes.data_as(ip)
    refused = (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_response_ensemble_limit(None, None, 1, p, 1, p, 1, 2.706, 2, rp, 1, None, None, None, None, None,
                                               None, None) in refused
    assert L.nusi_plan_response_ensemble_limit_host(None, p, 1, p, 1, p, 1, 2.706, 2, rp, 1, p, p, None, None, None,
                                                    None) in refused
    assert L.nusi_plan_set_option(None, _lib.OPT_ENSEMBLE_LIMIT_MB, 1) == _lib.NUSI_EPARAM
