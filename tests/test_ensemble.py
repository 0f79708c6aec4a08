"""The host form of the ensemble call (CPU, numpy only): detector.argbest -- the selection rule of
nusi_plan_response_ensemble, the minimum under the key (isnan(nll), nll, q) --, detector.ensemble_host -- a loop of
fit_host / profile_host over the data sets, reduced with argbest -- and detector.pseudo_data.
"""
import numpy as np
import pytest

from nusiprop_amd import detector

INF, NAN = np.inf, np.nan


# --- argbest: the key (isnan, nll, index) ------------------------------------------------------------------------------
def test_argbest_ties_go_to_the_lowest_index():
    assert detector.argbest([3.0, 1.0, 2.0, 1.0, 1.0]) == 1
    assert detector.argbest([0.0, -0.0]) == 0 and detector.argbest([-0.0, 0.0]) == 0       # compared as numbers
    assert detector.argbest([5.0]) == 0


def test_argbest_infinities_and_nans():
    assert detector.argbest([INF, 2.0, INF, 1.5]) == 3              # +inf among finite values loses
    assert detector.argbest([INF, INF, INF]) == 0                   # all +inf: the first
    assert detector.argbest([NAN, INF, 7.0]) == 2
    assert detector.argbest([NAN, INF, NAN, INF]) == 1              # NaN loses to +inf
    assert detector.argbest([NAN, NAN]) == 0                        # all NaN: the first
    assert detector.argbest([NAN, -INF, 1.0]) == 1


def test_argbest_over_an_axis():
    x = np.array([[[1.0, 0.5, 0.5], [NAN, INF, INF]], [[NAN, NAN, NAN], [2.0, 2.0, 1.0]]])
    got = detector.argbest(x)
    assert got.shape == (2, 2) and np.issubdtype(got.dtype, np.integer)
    assert np.array_equal(got, [[1, 1], [0, 2]])
    assert np.array_equal(detector.argbest(x, axis=0), [[0, 0, 0], [1, 1, 1]])
    assert np.array_equal(detector.argbest(x, axis=1), [[0, 0, 0], [1, 1, 1]])
    # any order of reduction gives the same answer: halves first, then the winners
    v = np.array([4.0, NAN, 1.0, 1.0, INF, 1.0, NAN])
    lo, hi = detector.argbest(v[:3]), 3 + detector.argbest(v[3:])
    assert detector.argbest(v) == (lo, hi)[detector.argbest([v[lo], v[hi]])] == 2


# --- ensemble_host -------------------------------------------------------------------------------------------------------
M, C, NTAB, Q, P = 6, 5, 2, 7, 3


def _case(seed=1):
    rng = np.random.default_rng(seed)
    R = rng.random((NTAB, M, C)) * 10.0 ** rng.uniform(-1, 1, (NTAB, 1, 1))
    S = rng.random((Q, M)) * 10.0 ** rng.uniform(-1, 1, (Q, 1))
    S[3] = 0.0                                                      # a spectrum of zeros: flat
    B = 0.5 + rng.random(C)
    T = np.stack([(1.0 + j) * np.exp(-(0.5 + 0.4 * j) * np.linspace(0.0, 3.0, C)) for j in range(3)]) * 5.0
    mean = 30.0 * detector.events_host(R, S)[1, 2] / detector.events_host(R, S)[1, 2].max() + T.sum(axis=0) + B
    data = detector.pseudo_data(mean, P, np.random.default_rng(seed + 1))
    data[1] *= 3.0                                                  # data sets of different scale
    return R, S, B, T, data


@pytest.mark.parametrize("K", (0, 1, 3))
def test_record_equals_the_single_call_at_its_q(K):
    R, S, B, T, data = _case()
    prior = (np.full(K, 1.0), np.full(K, 0.5)) if K else None
    q, nll, theta, st = detector.ensemble_host(R, S, data, templates=T[:K] if K else None, prior=prior, background=B)
    assert q.shape == nll.shape == st.shape == (P, NTAB) and theta.shape == (P, NTAB, 1 + K)
    assert q.dtype == np.int32 and st.dtype == np.int32 and nll.dtype == np.float64
    for p in range(P):
        if K:
            th, n, _, s = detector.fit_host(R, S, data[p], T[:K], prior=prior, background=B)
        else:
            a, n, _, s = detector.profile_host(R, S, data[p], background=B)
            th = a[..., None]
        best = detector.argbest(n)
        assert np.array_equal(q[p], best)
        for t in range(NTAB):
            assert nll[p, t] == n[t, best[t]] == n[t].min() and st[p, t] == s[t, best[t]]
            assert np.array_equal(theta[p, t], th[t, best[t]])
        # P = 1: the single-data-set call reduced with argbest
        one = detector.ensemble_host(R, S, data[p:p + 1], templates=T[:K] if K else None, prior=prior, background=B)
        for x, y in zip(one, (q, nll, theta, st)):
            assert x.shape[0] == 1 and np.array_equal(x[0], y[p])
    assert len({q[p].tobytes() + nll[p].tobytes() for p in range(P)}) > 1       # the data sets differ


def test_ensemble_host_shapes_of_one():
    R, S, B, T, data = _case(seed=2)
    q, nll, theta, st = detector.ensemble_host(R[0], S[1], data[0], background=B)      # one table, spectrum, data set
    assert q.shape == (1, 1) and theta.shape == (1, 1, 1) and q[0, 0] == 0
    a, n, _, s = detector.profile_host(R[0], S[1], data[0], background=B)
    assert nll[0, 0] == n and theta[0, 0, 0] == a and st[0, 0] == s


def test_ensemble_host_identical_spectra_and_infinite_statistics():
    R, S, B, T, data = _case(seed=3)
    best = int(detector.ensemble_host(R, S, data[:1], background=B)[0][0, 0])
    S2 = np.concatenate([S, S[best:best + 1]])                      # the best spectrum again, at the end: the first wins
    assert detector.ensemble_host(R, S2, data[:1], background=B)[0][0, 0] == best
    Rz, Bz = R.copy(), B.copy()
    Rz[:, :, C - 1] = 0.0                                           # a dead bin with a count: every nll = +inf
    Bz[C - 1] = 0.0
    d = data.copy()
    d[:, C - 1] = 0.0
    d[1, C - 1] = 2.0
    q, nll, theta, st = detector.ensemble_host(Rz, S, d, background=Bz)
    assert np.all(q[1] == 0) and np.all(np.isinf(nll[1])) and np.all(st[1] & detector.FIT_INFINITE)
    assert np.all(np.isfinite(nll[[0, 2]])) and not np.any(st[[0, 2]] & detector.FIT_INFINITE)


def test_ensemble_host_refusals():
    R, S, B, T, data = _case(seed=4)
    with pytest.raises(ValueError):
        detector.ensemble_host(R, S, data[:, :-1], background=B)                         # C does not match
    with pytest.raises(ValueError):
        detector.ensemble_host(R, S, data[None], background=B)                           # three axes
    with pytest.raises(ValueError):
        detector.ensemble_host(R, S, np.zeros((0, C)), background=B)                     # no data set
    with pytest.raises(ValueError):
        detector.ensemble_host(R, S[:, :-1], data, background=B)                         # M does not match
    for bad in (-1.0, NAN, INF):
        d = data.copy()
        d[2, 1] = bad
        with pytest.raises(ValueError):
            detector.ensemble_host(R, S, d, background=B)
    with pytest.raises(ValueError):
        detector.ensemble_host(R, S, data, templates=np.ones((4, C)), background=B)     # K = 4


# --- pseudo_data -----------------------------------------------------------------------------------------------------------
def test_pseudo_data():
    mu = np.array([0.0, 0.3, 4.0, 150.0, 1e5])
    x = detector.pseudo_data(mu, 37, np.random.default_rng(5))
    assert x.shape == (37, 5) and x.dtype == np.float64 and x.flags.c_contiguous
    assert np.all(x >= 0) and np.array_equal(x, np.floor(x)) and np.all(x[:, 0] == 0)
    assert np.array_equal(x, detector.pseudo_data(mu, 37, np.random.default_rng(5)))    # reproducible from a seed
    assert not np.array_equal(x, detector.pseudo_data(mu, 37, np.random.default_rng(6)))
    assert abs(x[:, 3].mean() - 150.0) < 5 * np.sqrt(150.0 / 37)
    for bad in (np.array([1.0, -1.0]), np.array([NAN, 1.0]), np.array([INF, 1.0]), np.ones((2, 2))):
        with pytest.raises(ValueError):
            detector.pseudo_data(bad, 3, np.random.default_rng(0))
    with pytest.raises(ValueError):
        detector.pseudo_data(mu, 0, np.random.default_rng(0))
