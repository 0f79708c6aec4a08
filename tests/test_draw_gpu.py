"""nusi_plan_draw_counts (k_poisson_draw) on the GPU: Plan.draw equals detector.draw_host with the oracle's ora_exp and
ora_log, every integer -- the generator is defined operation for operation (include/nusi.h "Drawing counts"), so there is
no tolerance.  Expectations on both sides of the split at 10, zero, the tiny and the huge; every C that changes the
index arithmetic (1, an odd one, one past a tile of 16, the most), P and rows that are not powers of two.
"""
import ctypes

import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from tests.test_detector_gpu import _Dev, _hip
from tests.test_tabulated_source_gpu import _plan

pytestmark = pytest.mark.gpu

MUS = np.array([0.0, 1e-300, 0.3, 9.999999, 10.0, 10.000001, 37.0, 1e3, 1e6, 1e12])
SEEDS = ((0x0123456789ABCDEF, 2), (0xFFFFFFFF00000001, 0xFFFFFFFF))


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


@pytest.fixture(scope="module")
def ora(oracle_mod):
    L = oracle_mod.lib()
    for f in (L.ora_exp, L.ora_log):
        f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
    return L.ora_exp, L.ora_log


def _mu(rows, C):
    """Every expectation of MUS, walking through them along (row, c) with a stride that shows each at several c."""
    return MUS[(3 * np.arange(rows)[:, None] + np.arange(C)[None, :]) % len(MUS)].copy()


@pytest.mark.parametrize("rows", (1, 4))
@pytest.mark.parametrize("P", (1, 3, 37))
@pytest.mark.parametrize("C", (1, 5, 17, 64))
def test_draw_equals_the_host_form(nusi, ora, C, P, rows):
    exp, log = ora
    mu = _mu(rows, C)
    plan = _plan(nusi, "G6")
    try:
        for seed, stream in SEEDS:
            got = plan.draw(mu, P, seed, stream=stream)
            want = detector.draw_host(mu, P, seed, stream=stream, exp=exp, log=log)
            assert got.shape == (rows, P, C)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
            assert not np.signbit(got).any()
        if rows == 1:
            assert np.array_equal(plan.draw(mu[0], P, seed, stream=stream), got[0])       # a vector: (P, C)
    finally:
        plan.close()


def test_every_expectation_at_many_toys(nusi, ora):
    """The ten expectations side by side, 37 toys each from two seeds: also that the counts look like their law."""
    exp, log = ora
    plan = _plan(nusi, "G6")
    try:
        a = plan.draw(MUS, 37, *SEEDS[0][:1], stream=SEEDS[0][1])
        b = plan.draw(MUS, 37, *SEEDS[1][:1], stream=SEEDS[1][1])
    finally:
        plan.close()
    assert np.array_equal(a, detector.draw_host(MUS, 37, SEEDS[0][0], stream=SEEDS[0][1], exp=exp, log=log))
    assert not np.array_equal(a, b)
    assert not a[:, :2].any() and np.array_equal(a, np.floor(a))
    for c in range(2, len(MUS)):
        assert abs(a[:, c].mean() - MUS[c]) <= 5 * np.sqrt(MUS[c] / 37), (c, a[:, c].mean())


def test_device_form_and_refusals(nusi, ora):
    exp, log = ora
    mu = _mu(2, 5)
    H = _hip()
    plan = _plan(nusi, "G6")
    try:
        with _Dev(H) as dev:
            n = 2 * 3 * 5
            buf = np.full(n + 4, np.nan)
            d = dev.alloc(buf.nbytes, buf)
            assert plan.draw_device(mu, 3, 99, d, stream=1) == (2, 5)
            # a second draw at once: it waits for the first before it reuses the plan's copy of mu
            d2 = dev.alloc(8 * 7)
            plan.draw_device([2.0], 7, 5, d2)
            assert H.hipDeviceSynchronize() == 0
            out = dev.fetch(d, (n + 4,))
            assert np.array_equal(out[:n].reshape(2, 3, 5), detector.draw_host(mu, 3, 99, stream=1, exp=exp, log=log))
            assert np.all(np.isnan(out[n:]))                                      # nothing past the end
            assert np.array_equal(dev.fetch(d2, (7, 1)), detector.draw_host([2.0], 7, 5, exp=exp, log=log))
            before = plan.draw(mu, 3, 99, stream=1)
            for bad_mu, P in ((np.array([[1.0, np.nan]]), 2), (np.array([[1.0, -1.0]]), 2), (np.array([[np.inf]]), 2),
                              (np.ones((1, 65)), 2), (np.ones((1, 3)), 0), (np.ones((1, 3)), _lib.DRAW_DATASETS_MAX + 1),
                              # rows P C = 2^39 - 64 and 2^39: past the (2^31 - 1) 256 counts one launch holds
                              (np.ones((161, 64)), 53353631), (np.ones((128, 64)), 1 << 26)):
                with pytest.raises(_lib.NusiError) as e:
                    plan.draw_device(bad_mu, P, 1, d)
                assert e.value.code == _lib.NUSI_EPARAM
            with pytest.raises(_lib.NusiError) as e:
                plan.draw_device(mu, 3, 1, 0)
            assert e.value.code == _lib.NUSI_EPARAM
            assert H.hipDeviceSynchronize() == 0
            assert np.array_equal(dev.fetch(d, (n + 4,))[:n], out[:n])            # a refused call changes nothing
            assert np.array_equal(plan.draw(mu, 3, 99, stream=1), before)
    finally:
        plan.close()
