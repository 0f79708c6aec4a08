"""The fit with J signal components on the GPU: nusi_plan_response_fit_components (k_components_fit<J, J + K>) against
its host form detector.fit_components_host, and Plan.composition_scan ("Signal components:
k_components_fit").

theta, mu and the status word must equal the host's bits whatever the flags are; nll within tests/test_fit_gpu.py's
bound, 2 (C + 3 + 3 K) u (sum_c (mu_c + |data_c log mu_c|) + the penalties), with the oracle's log on the host, and +inf
in the same places.

  * real rows: G6's mass-resolved response, folded as a stack with a detector that tells the flavours apart (with a
    flavour-blind one the three rows coincide and every record is rightly SINGULAR), as it is and composed onto the pure
    flavours; the tally of flags is printed, no share of converged fits is asserted;
  * synthetic rows on all eight (J, K) instances: fits that share a wave stop after different numbers of steps and
    halvings, end with different free sets, and a SINGULAR, a FLAT and a one-dead-component record sit beside converged
    ones -- each of that asserted on the host result first;
  * many spectra on few bins into NaN-filled buffers with a tail, tables alone, the optional outputs, the raw pointers;
  * the refusals, by value only (the size limits are tests/test_fit_components.py's, through nusi_fit_components_shape);
  * composition_scan against the host forms, and its statistic's two properties.

No call here passes a size (ntab, J, Q, C) that differs from its arrays' own.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import (FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_ITER_MAX, FIT_NOT_CONVERGED, FIT_SINGULAR,
                                   FIT_STEPS_MASK, FIT_TRIALS_MASK, FIT_TRIALS_SHIFT, FIT_ZERO)
from tests.test_detector_gpu import _B, _D, _Dev, _hip, _ora_log, _spectra
from tests.test_fit_components import allowance, triangle
from tests.test_fit_gpu import _prior_of, _templates
from tests.test_profile_gpu import _fetch_int
from tests.test_response_mass_gpu import GRIDS, MAXIS, NPT, _mass, _plan, _point, nusi  # noqa: F401 (nusi: a fixture)

pytestmark = pytest.mark.gpu

M = MAXIS["G6"]
N = GRIDS["G6"][0]
U = 2.0 ** -53
JK = [(J, K) for J in (2, 3) for K in (0, 1, 2, 3)]


def _detector(C):
    """tests/test_detector_gpu.py's D with the flavours told apart: bin c sees flavour c % 3 in full and the others at 5 %."""
    D = _D(C, N)
    for c in range(C):
        for f in range(3):
            if c % 3 != f:
                D[c, f] *= 0.05
    return D


_STACK = {}


def _stacks(nusi, C):  # noqa: F811
    """(raw (NPT, 3, M, C): the folded mass-resolved rows, pure: those composed onto the pure flavours e, mu, tau with each
    table's own ordering, D, B), once per C, read-only."""
    if C not in _STACK:
        from nusiprop_amd import sources
        G3f = _mass(nusi, "G6", True)[1]
        D, B = _detector(C), _B(C)
        plan = _plan(nusi, "G6", max_points=NPT)
        plan.set_detector(D, background=B)
        raw = plan.fold_response(G3f.reshape(3 * NPT, M, 3, N)).reshape(NPT, 3, M, C)
        kap = np.array([[sources.mass_fractions(e, normal_ordering=_point("G6", t, True)["normal_ordering"])
                         for e in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))] for t in range(NPT)])
        pure = plan.compose_response(raw, kap)
        plan.close()
        assert pure.shape == raw.shape and np.all(np.isfinite(raw)) and np.all(np.isfinite(pure))
        for a in (raw, pure):
            a.setflags(write=False)
        _STACK[C] = (raw, pure, D, B)
    return _STACK[C]


def _check(got, R3, S, data, T, prior, B, log, what, quiet=False):
    """theta, status and mu equal fit_components_host's bits; nll within the module's bound.  Returns the host's."""
    theta, nll, mu, st = got
    hth, hn, hm, hs = detector.fit_components_host(R3, S, data, T, prior=prior, background=B, log=log)
    assert theta.shape == hth.shape and st.shape == hs.shape and mu.shape == hm.shape and st.dtype == np.int32
    assert np.array_equal(st, hs), (what, np.argwhere(st != hs)[:4], [hex(v) for v in st[st != hs][:4]],
                                    [hex(v) for v in hs[st != hs][:4]])
    assert np.array_equal(theta, hth), (what, np.argwhere(theta != hth)[:4])
    assert np.array_equal(mu, hm), what
    C, J = len(data), R3.shape[1]
    K = 0 if T is None else len(T)
    inf = np.isinf(hn)
    assert np.array_equal(np.isinf(nll), inf) and np.all(nll[inf] > 0), what
    assert np.array_equal(inf, (hs & FIT_INFINITE) != 0), what
    m, w = detector._prior(K, prior)
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.sum(mu + np.where(data > 0, np.abs(data * np.log(np.where(mu > 0, mu, 1.0))), 0.0), axis=-1)
    mag = mag + np.sum(0.5 * w[1:] * (theta[..., J:] - m[1:]) ** 2, axis=-1)
    bound = 2 * (C + 3 + 3 * K) * U * mag
    fin = ~inf
    ratio = float(np.max(np.abs(nll[fin] - hn[fin]) / bound[fin])) if np.any(fin) else 0.0
    steps, halv = hs & FIT_STEPS_MASK, (hs >> FIT_TRIALS_SHIFT) & FIT_TRIALS_MASK
    if not quiet:
        print("%s: %d fits, nll ratio to the bound %.3f; steps %d .. %d (mean %.2f), halvings mean %.2f max %d; %d flat, "
              "%d boundary, %d singular, %d not converged, %d infinite, %d with a component at zero" % (
                  what, hs.size, ratio, steps.min(), steps.max(), steps.mean(), halv.mean(), halv.max(),
                  np.count_nonzero(hs & FIT_FLAT), np.count_nonzero(hs & FIT_BOUNDARY), np.count_nonzero(hs & FIT_SINGULAR),
                  np.count_nonzero(hs & FIT_NOT_CONVERGED), int(inf.sum()), np.count_nonzero(hs & (0x3F * FIT_ZERO))))
    assert ratio <= 1.0, (what, ratio)
    assert np.all(steps <= FIT_ITER_MAX), what
    return hth, hn, hm, hs


def _data(R3, S, T, B, C, seed):
    """Counts around a mixture of table 0's first spectrum's components (200, 100 and 50 events in their fullest bins)
    plus the templates and B; some bins empty."""
    mean = B.copy() if T is None else T.sum(axis=0) + B
    for j in range(R3.shape[1]):
        s = detector.events_host(R3[:, j], S)[0, 0]
        mean = mean + (200.0 / 2 ** j) / s.max() * s
    data = np.floor(mean * (0.5 + np.random.default_rng(seed).random(C)))
    if C > 7:
        data[::5] = 0.0
    if C == 1:
        data[0] += 1.0
    return data


# --- real rows: the G6 tables' mass-resolved response ------------------------------------------------------------------------
@pytest.mark.parametrize("J,K", [(2, 0), (3, 0), (3, 1), (3, 3)])
@pytest.mark.parametrize("C", (1, 3, 5, 17, 64))
@pytest.mark.parametrize("Q", (1, 5, 19))
def test_real_rows_equal_the_host_form(nusi, oracle_mod, Q, C, J, K):  # noqa: F811
    log = _ora_log(oracle_mod)
    raw, pure, D, B = _stacks(nusi, C)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0) if K else None
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    for name, stack in (("mass rows", raw), ("pure flavours", pure)):
        R3 = np.ascontiguousarray(stack[:, :J])
        if np.any(R3 < 0):                          # (a mass-resolved entry may be negative: include/nusi.h, "Sign")
            print("G6 %s C=%d: %d folded entries below zero, the host form does not take them" % (name, C, np.count_nonzero(R3 < 0)))
            assert name == "mass rows"
            continue
        data = _data(R3, S, T, B, C, seed=C + Q)
        if C > 1:
            data[C - 1] = 0.0                       # the bin nothing ever fills
        for kind in ("none", "mixed") if K else ("none",):
            prior = _prior_of(T, kind) if K else None
            plan.set_templates(T, prior=prior)
            assert plan.templates() == K
            got = plan.fit_components(R3, S, data)
            assert got[0].shape == (NPT, Q, J + K)
            _check(got, R3, S, data, T, prior, B, log, "G6 %s C=%d Q=%d J=%d K=%d prior %s" % (name, C, Q, J, K, kind))
            if C > 1:                               # a count where nothing is expected: +inf, the flag, the same theta
                d2 = data.copy()
                d2[C - 1] = 2.0
                got2 = plan.fit_components(R3, S, d2)
                _check(got2, R3, S, d2, T, prior, B, log, "... a count where nothing is expected", quiet=True)
                assert np.all(np.isinf(got2[1])) and np.array_equal(got2[0], got[0])
                assert np.array_equal(got2[3], got[3] | FIT_INFINITE)
    plan.close()


# --- synthetic rows: fits that part ways inside one wave ---------------------------------------------------------------------
N_SING, N_DEAD = 2, 4          # the source bins whose rows make a SINGULAR and a one-dead-component record


def _case(C, J, K, ntab=2, Q=40):
    """(R3, S, data, T, prior, B) of one call, after tests/test_profile_gpu.py's _synthetic: every row of R3 a bump
    somewhere else, scales over decades between tables and spectra, sparse spectra of 1 .. 3 rows, so the components of a
    spectrum have shapes of their own.  Spectra 3, 19, .. are zeros (FLAT); spectra 5, 21, .. take source bin N_SING
    alone, where components 0 and 1 have the SAME row (SINGULAR: identical signals); spectra 7, 23, .. take source bin
    N_DEAD alone, where the last signal component's row is zero (not live, the others are fitted).  The data follow table
    1's median spectrum's components in the shares 1 : 1/2 : 1/4 plus the templates and a background."""
    rng = np.random.default_rng([C, J, K])
    R3 = rng.random((ntab, J, M, C)) * 10.0 ** rng.uniform(-4, 4, (ntab, 1, 1, 1))
    c0, wd = rng.uniform(0, C, (ntab, J, M, 1)), rng.uniform(0.5, C / 3 + 1, (ntab, J, M, 1))
    R3 = R3 * np.exp(-((np.arange(C)[None, None, None, :] - c0) / wd) ** 2)
    S = rng.random((Q, M)) * 10.0 ** rng.uniform(-3, 3, (Q, 1))
    pick = rng.random((Q, M)) < 2.0 / M
    pick[np.arange(Q), rng.integers(1, M, Q)] = True
    S = S * pick
    S[3::16] = 0.0
    for q0, n in ((5, N_SING), (7, N_DEAD)):
        one = np.zeros(M)
        one[n] = 1.0
        S[q0::16] = one[None, :] * 10.0 ** rng.uniform(-3, 3, (len(S[q0::16]), 1))
    R3[:, 1, N_SING] = R3[:, 0, N_SING]
    R3[:, J - 1, N_DEAD] = 0.0
    R3[:, :J - 1, N_DEAD] += 1e-3 * R3[:, :J - 1, N_DEAD].max(axis=-1, keepdims=True)     # (the live ones reach every bin)
    ev = [detector.events_host(R3[:, j], S)[1] for j in range(J)]
    qref = np.argsort(ev[0].sum(axis=-1))[Q // 2]               # table 1's median spectrum: its components 1 : 1/2 : 1/4
    ref = sum(0.5 ** j * ev[j][qref] / ev[j][qref].max() for j in range(J) if ev[j][qref].max() > 0)
    T = _templates(C, K, scale=50.0) if K else None
    if K and C > 1:
        T[:, C - 1] = T[:, 0] * 1e-3                            # (no dead bin here)
    B = 30.0 * (0.5 + rng.random(C))        # (without a background two identical rows are optimal at the equal-share start)
    mean = 1e3 / ref.max() * ref + (T.sum(axis=0) if K else 0.0) + B
    data = rng.poisson(mean).astype(np.float64)
    if C > 4:
        data[1] = 0.0
    prior = None
    if K and C <= J + K:                                        # no more bins than components: priors on the templates
        prior = (np.full(K, 1.0), np.full(K, 0.5))
    return np.ascontiguousarray(R3), np.ascontiguousarray(S), data, T, prior, B


def _parted(hs, per_wave):
    """Do fits that share a wave (per_wave consecutive spectra of a table) differ in steps, halvings and zero bits, and do
    a SINGULAR, a FLAT and a one-dead-component record (spectra 5, 3 and 7 of every 16) each share one with a converged fit?"""
    steps, halv, zero = hs & FIT_STEPS_MASK, (hs >> FIT_TRIALS_SHIFT) & FIT_TRIALS_MASK, (hs >> 16) & 0x3F
    conv = (hs & (FIT_SINGULAR | FIT_FLAT | FIT_NOT_CONVERGED)) == 0
    out = [False] * 6
    for t in range(hs.shape[0]):
        for q0 in range(0, hs.shape[1], per_wave):
            w = slice(q0, q0 + per_wave)
            for i, x in enumerate((steps, halv, zero)):
                out[i] |= len(set(x[t, w].tolist())) > 1
            qs = np.arange(hs.shape[1])[w]
            other = conv[t, w] & (qs % 16 != 7)
            out[3] |= bool(np.any(hs[t, w] & FIT_SINGULAR) and np.any(other))
            out[4] |= bool(np.any(hs[t, w] & FIT_FLAT) and np.any(other))
            out[5] |= bool(np.any(conv[t, w] & (qs % 16 == 7)) and np.any(other))
    return out


@pytest.mark.parametrize("J,K", JK)
@pytest.mark.parametrize("C", (1, 3, 5, 17, 64))
def test_fits_that_part_ways_inside_a_wave(nusi, oracle_mod, C, J, K):  # noqa: F811
    """All eight instances.  What the wave's run masks, the divergent solve and the full-exec butterflies can get wrong
    shows only where neighbours differ, so the host result is asked first: steps, halvings and free sets differ inside a
    wave, and a SINGULAR, a FLAT and a one-dead-component record each share one with a converged fit (C = 64: the four
    waves of a block).  That needs data
    that can determine the components: it is asserted for C >= J (the templates have priors where C < J + K); at C = 1
    two signal components on one bin are never determined and only the equality with the host is left."""
    log = _ora_log(oracle_mod)
    R3, S, data, T, prior, B = _case(C, J, K)
    plan = _plan(nusi, "G6")
    plan.set_detector(_D(C, N), background=B)
    plan.set_templates(T, prior=prior)
    hth, hn, hm, hs = detector.fit_components_host(R3, S, data, T, prior=prior, background=B, log=log)
    lg = int(np.ceil(np.log2(C))) if C > 1 else 0
    per_wave = 64 >> lg if lg < 6 else 4          # (C = 64: the four waves of a block)
    parted = _parted(hs, per_wave)
    sig0 = (hs >> 16) & ((1 << J) - 1)
    dead = hs[:, 7::16]
    if C >= J:
        assert all(parted), (parted, [hex(v) for v in hs[0, :16]])
        assert np.all(hs[:, 5::16] & FIT_SINGULAR) and np.all(hs[:, 3::16] & FIT_FLAT)
        assert np.any(sig0 != 0) and np.any((sig0 == 0) & ((hs & (FIT_SINGULAR | FIT_NOT_CONVERGED)) == 0))
    # one dead component: not live, at zero with its bit, and no FLAT (the others are live)
    assert np.all(dead & (FIT_ZERO << (J - 1))) and not np.any(dead & FIT_FLAT) and np.all(hth[:, 7::16, J - 1] == 0.0)
    got = plan.fit_components(R3, S, data)
    _check(got, R3, S, data, T, prior, B, log, "synthetic C=%d J=%d K=%d" % (C, J, K))
    plan.close()


# --- shapes and outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (1, 2))
def test_many_spectra_on_few_bins(nusi, oracle_mod, C):  # noqa: F811
    """Q = 600 is several blocks (256 fits a block at C = 1, 128 at C = 2) with a partial last one.  The device form
    writes into NaN-filled buffers (status: -1) that are 64 elements longer than [ntab][Q][..]: every entry is written and
    nothing behind the last."""
    log = _ora_log(oracle_mod)
    raw, pure, D, B = _stacks(nusi, C)
    Q, J, K, TAIL = 600, 2, 1, 64
    R3 = np.ascontiguousarray(pure[:, :J])
    S = _spectra(M, Q)
    T = np.array([[4.0, 7.0][:C]])
    prior = (np.array([1.0]), np.array([0.2]))
    data = np.array([9.0, 3.0][:C])
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=prior)
    got = plan.fit_components(R3, S, data)
    _check(got, R3, S, data, T, prior, B, log, "G6 C=%d Q=%d J=%d K=%d" % (C, Q, J, K))
    H = _hip()
    with _Dev(H) as dev:
        dR = dev.alloc(R3.nbytes, R3)
        sizes = [NPT * Q * (J + K), NPT * Q, NPT * Q * C, NPT * Q]
        dT, dN, dM = (dev.alloc(8 * (n + TAIL), np.full(n + TAIL, np.nan)) for n in sizes[:3])
        dS = dev.alloc(4 * (sizes[3] + TAIL), np.full(sizes[3] + TAIL, -1, dtype=np.int32))
        assert plan.fit_components_device(dR, NPT, J, S, data, dT, dN, dM, dS) == Q
        assert H.hipDeviceSynchronize() == 0
        for ptr, n, want in ((dT, sizes[0], got[0]), (dN, sizes[1], got[1]), (dM, sizes[2], got[2])):
            out = dev.fetch(ptr, (n + TAIL,))
            assert np.array_equal(out[:n], want.ravel()) and np.all(np.isnan(out[n:]))
        out = _fetch_int(H, dS, (sizes[3] + TAIL,))
        assert np.array_equal(out[:sizes[3]], got[3].ravel()) and np.all(out[sizes[3]:] == -1)
    plan.close()


def test_tables_alone_and_the_device_forms(nusi):  # noqa: F811
    C, Q, J, K = 17, 19, 3, 2
    raw, pure, D, B = _stacks(nusi, C)
    R3 = np.ascontiguousarray(pure)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0)
    data = _data(R3, S, T, B, C, seed=2)
    data[C - 1] = 0.0
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=_prior_of(T, "mixed"))
    theta, nll, mu, st = plan.fit_components(R3, S, data)
    assert len({theta[t].tobytes() for t in range(NPT)}) == NPT
    for t in range(NPT):                            # a 3-table call against each table alone, and a spectrum alone
        one = plan.fit_components(R3[t:t + 1], S, data)
        for x, y in zip(one, (theta, nll, mu, st)):
            assert np.array_equal(x[0], y[t]), t
    one = plan.fit_components(R3, S[6:7], data)
    for x, y in zip(one, (theta, nll, mu, st)):
        assert np.array_equal(x[:, 0], y[:, 6])
    H = _hip()
    with _Dev(H) as dev:                            # into NaN-filled buffers, each optional output NULL in turn
        dR = dev.alloc(R3.nbytes, R3)
        for skip in (None, "nll", "mu", "status"):
            dT, dN = dev.alloc(theta.nbytes, np.full(theta.shape, np.nan)), dev.alloc(nll.nbytes, np.full(nll.shape, np.nan))
            dM = dev.alloc(mu.nbytes, np.full(mu.shape, np.nan))
            dS = dev.alloc(st.nbytes, np.full(st.shape, -1, dtype=np.int32))
            assert plan.fit_components_device(dR, NPT, J, S, data, dT, None if skip == "nll" else dN,
                                              None if skip == "mu" else dM, None if skip == "status" else dS) == Q
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(dev.fetch(dT, theta.shape), theta), skip
            n2, m2, s2 = dev.fetch(dN, nll.shape), dev.fetch(dM, mu.shape), _fetch_int(H, dS, st.shape)
            assert np.all(np.isnan(n2)) if skip == "nll" else np.array_equal(n2, nll), skip
            assert np.all(np.isnan(m2)) if skip == "mu" else np.array_equal(m2, mu), skip
            assert np.all(s2 == -1) if skip == "status" else np.array_equal(s2, st), skip
    # the fit and the profile are untouched: one component of the stack is an ordinary folded matrix
    th1 = plan.fit(np.ascontiguousarray(R3[:, 0]), S, data)[0]
    assert np.array_equal(th1, detector.fit_host(R3[:, 0], S, data, T, prior=_prior_of(T, "mixed"), background=B)[0])
    plan.close()


# --- refusals, by value only ---------------------------------------------------------------------------------------------------
def test_refusals(nusi):  # noqa: F811
    from nusiprop_amd import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    C, J, K, Q = 5, 3, 2, 2
    raw, pure, D, B = _stacks(nusi, C)
    R3 = np.ascontiguousarray(pure)
    S = _spectra(M, Q)
    data = np.arange(1.0, C + 1.0)
    T = _templates(C, K)
    plan = _plan(nusi, "G6")

    def refused(code, f, *a, **k):
        with pytest.raises(nusi.NusiError) as ei:
            f(*a, **k)
        assert ei.value.code == code, (ei.value.code, str(ei.value))

    Sp, datap = S.ctypes.data_as(dp), data.ctypes.data_as(dp)
    refused(_lib.NUSI_ESTATE, plan.fit_components, R3, S, data)                              # no detector
    plan.set_detector(D, background=B)
    assert plan.templates() == 0
    want0 = plan.fit_components(R3, S, data)                                                 # K = 0 is allowed
    assert want0[0].shape == (NPT, Q, J)
    plan.set_templates(T)
    want = plan.fit_components(R3, S, data)
    assert want[0].shape == (NPT, Q, J + K)
    refused(_lib.NUSI_EPARAM, plan.fit_components, R3, S, None)                              # NULL data
    for bad in (-1.0, np.nan, np.inf):
        db, Sb = data.copy(), np.array(S)
        db[C - 1] = bad
        Sb[1, M - 1] = bad
        refused(_lib.NUSI_EPARAM, plan.fit_components, R3, S, db)
        refused(_lib.NUSI_EPARAM, plan.fit_components, R3, Sb, data)
    with pytest.raises(ValueError):
        plan.fit_components(R3[:, :, :-1], S, data)
    with pytest.raises(ValueError):
        plan.fit_components(R3, S, data[:-1])
    H = _hip()
    with _Dev(H) as dev:
        dR, dT = dev.alloc(R3.nbytes, R3), dev.alloc(NPT * Q * (J + K) * 8)
        ft = L.nusi_plan_response_fit_components
        assert ft(plan._h, dR, NPT, J, Sp, Q, datap, None, None, None, None, None) == _lib.NUSI_EPARAM     # NULL theta
        assert ft(plan._h, dR, NPT, J, Sp, Q, None, dT, None, None, None, None) == _lib.NUSI_EPARAM        # NULL data
        assert ft(plan._h, None, NPT, J, Sp, Q, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM     # NULL rows
        assert ft(plan._h, dR, NPT, J, None, Q, datap, dT, None, None, None, None) == _lib.NUSI_EPARAM     # NULL spectra
    got = plan.fit_components(R3, S, data)          # the refusals changed nothing
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    plan.set_detector(D, background=B)              # a new detector clears the templates: K = 0 runs
    assert plan.templates() == 0
    got0 = plan.fit_components(R3, S, data)
    for x, y in zip(got0, want0):
        assert np.array_equal(x, y)
    plan.close()


# --- the scan over the flavour triangle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (0, 1))
def test_composition_scan(nusi, K):  # noqa: F811
    """G6, C = 17, Q = 5, the ten compositions in steps of a third: the held fits and the free fit carry the host forms'
    bits, q is max(2 lambda, 0) of detector.composition_statistic on them, and at the free fit's own fractions q is
    within tests/test_fit_components.py's ``allowance`` of zero (where both fits converged)."""
    from nusiprop_amd import response
    C, Q = 17, 5
    raw, pure, D, B = _stacks(nusi, C)
    R3 = np.ascontiguousarray(pure)
    S = _spectra(M, Q)
    T = _templates(C, K, scale=20.0) if K else None
    prior = (np.array([1.2]), np.array([0.3])) if K else None
    data = _data(R3, S, T, B, C, seed=3)
    data[C - 1] = 0.0
    phi = triangle(3)
    plan = _plan(nusi, "G6")
    plan.set_detector(D, background=B)
    plan.set_templates(T, prior=prior)
    q, fixed, free, word = plan.composition_scan(R3, S, data, phi, prior=prior)
    assert q.shape == word.shape == (NPT, len(phi), Q) and word.dtype == np.int32
    Rc = response.compose_host(R3, phi).reshape(NPT * len(phi), M, C)
    if K:
        hth, hn, hm, hs = detector.fit_host(Rc, S, data, T, prior=prior, background=B)
    else:
        ha, hn, hm, hs = detector.profile_host(Rc, S, data, background=B)
        hth = ha[..., None]
    assert np.array_equal(fixed[0].reshape(hth.shape), hth) and np.array_equal(fixed[2].reshape(hm.shape), hm)
    assert np.array_equal(fixed[3].reshape(hs.shape), hs)
    fth, fn, fm, fs = detector.fit_components_host(R3, S, data, T, prior=prior, background=B)
    assert np.array_equal(free[0], fth) and np.array_equal(free[2], fm) and np.array_equal(free[3], fs)
    lam, mag = detector.composition_statistic(fixed[2], fixed[0], free[2][:, None], free[0][:, None], data, prior=prior)
    assert np.array_equal(q, np.maximum(2.0 * lam, 0.0), equal_nan=True) and np.all(q[word == 0] >= 0.0)
    bad = FIT_NOT_CONVERGED | FIT_SINGULAR | FIT_INFINITE
    assert np.array_equal(word, (fixed[3] & bad) | (free[3][:, None] & bad))
    print("composition_scan K=%d: %d of %d entries flagged; q from %.3g to %.3g" % (
        K, np.count_nonzero(word), word.size, np.nanmin(q), np.nanmax(q)))
    # the free fit's own fractions, one composition per (table, spectrum): entry [t, q, q]
    total, frac = detector.composition(free[0], 3)
    own = np.where(np.isnan(frac), 1.0 / 3.0, frac)
    q2, fx, fr, w2 = plan.composition_scan(R3, S, data, own, prior=prior)
    lam2, mag2 = detector.composition_statistic(fx[2], fx[0], fr[2][:, None], fr[0][:, None], data, prior=prior)
    sig = [detector.events_host(R3[:, j], S) for j in range(3)]
    checked = 0
    for t in range(NPT):
        for i in range(Q):
            if w2[t, i, i] or not total[t, i] > 0:
                continue
            X = np.vstack([np.stack([s[t, i] for s in sig])] + ([T] if K else []))
            ok = allowance(fx[2][t, i, i], fx[0][t, i, i], fr[2][t, i], fr[0][t, i], own[t, i], X, data, prior, mag2[t, i, i], M)
            assert abs(lam2[t, i, i]) <= ok and q2[t, i, i] <= 2.0 * ok, (t, i, lam2[t, i, i], ok)
            checked += 1
    print("composition_scan K=%d: %d of %d own compositions checked against the allowance" % (K, checked, NPT * Q))
