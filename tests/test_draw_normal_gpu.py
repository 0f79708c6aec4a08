"""The toys' normal generator on the GPU: k_normal_draw (nusi_plan_draw_normals) against detector.draw_normal_host with the
oracle's log, bit for bit.  rows = 3, P = 5, J = 1, 3 and 64 (the counter's 6 bits of j full); centres 0, 0.3, 1 and 50 under
widths 0.05, 1 and inf -- the truncation binding, half binding and far off, and no prior.  Both the _host form and the
device form's output.  Refusals vary values only: every call passes its arrays' own sizes.
"""
import numpy as np
import pytest

from nusiprop_amd import _lib, detector
from tests.test_detector_gpu import _Dev, _hip, _ora_log, _plan, nusi  # noqa: F401  (nusi: the fixture)

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
ROWS, P = 3, 5
CENTRES, WIDTHS = (0.0, 0.3, 1.0, 50.0), (0.05, 1.0, np.inf)


def _inputs(J):
    """center (ROWS, J) and sigma (J,): every (centre, width) pair of the lists where J holds them, cycled with the row."""
    k = np.arange(ROWS)[:, None] + np.arange(J)[None, :]
    center = np.array(CENTRES)[k % len(CENTRES)]
    sigma = np.array(WIDTHS)[(np.arange(J) // len(CENTRES) + np.arange(J)) % len(WIDTHS)]
    return np.ascontiguousarray(center), sigma


@pytest.mark.parametrize("J", (1, 3, 64))
def test_draw_normal_is_the_host_form(nusi, oracle_mod, J):  # noqa: F811
    log = _ora_log(oracle_mod)
    plan = _plan(nusi, "G6")
    H = _hip()
    try:
        center, sigma = _inputs(J)
        if J == 64:
            assert {(c, s) for c in CENTRES for s in WIDTHS} == {(center[r, j], sigma[j]) for r in range(ROWS) for j in range(J)}
        for stream in (0, 3):
            want = detector.draw_normal_host(center, sigma, P, SEED, stream=stream, log=log)
            got = plan.draw_normal(center, sigma, P, SEED, stream=stream)
            assert got.shape == (ROWS, P, J) and np.array_equal(got, want), (J, stream)
            assert np.all(got >= 0) and not np.signbit(got).any()
            nop = np.isinf(sigma)
            assert np.array_equal(got[:, :, nop], np.broadcast_to(center[:, None, nop], got[:, :, nop].shape))
            with _Dev(H) as dev:
                dO = dev.alloc(want.nbytes, np.full(want.shape, np.nan))
                assert plan.draw_normal_device(center, sigma, P, SEED, dO, stream=stream) == (ROWS, J)
                assert H.hipDeviceSynchronize() == 0
                assert np.array_equal(dev.fetch(dO, want.shape), want), (J, stream)
        # a vector is row 0; a number is every component's width
        assert np.array_equal(plan.draw_normal(center[0], sigma, P, SEED), detector.draw_normal_host(center[0], sigma, P, SEED, log=log))
        assert np.array_equal(plan.draw_normal(center, 1.0, P, SEED), detector.draw_normal_host(center, 1.0, P, SEED, log=log))
        # the counts of the same identity do not move: other blocks
        mu = np.full((ROWS, J), 12.0)
        before = plan.draw(mu, P, SEED)
        plan.draw_normal(center, sigma, P, SEED)
        assert np.array_equal(plan.draw(mu, P, SEED), before)
    finally:
        plan.close()


def test_refusals_change_nothing(nusi):  # noqa: F811
    plan = _plan(nusi, "G6")
    H = _hip()
    try:
        center, sigma = _inputs(3)
        with _Dev(H) as dev:
            dO = dev.alloc(8 * ROWS * P * 3, np.full((ROWS, P, 3), np.nan))
            for c, s, p in ((np.where(center == 0.3, -0.3, center), sigma, P), (np.where(center == 0.3, np.nan, center), sigma, P),
                            (np.where(center == 0.3, np.inf, center), sigma, P), (center, [0.05, 0.0, 1.0], P),
                            (center, [0.05, -1.0, 1.0], P), (center, [0.05, np.nan, 1.0], P), (center, sigma, 0),
                            (center, sigma, _lib.DRAW_DATASETS_MAX + 1)):
                with pytest.raises(_lib.NusiError) as e:
                    plan.draw_normal_device(c, s, p, SEED, dO)
                assert e.value.code == _lib.NUSI_EPARAM
            with pytest.raises(_lib.NusiError) as e:
                plan.draw_normal_device(center, sigma, P, SEED, 0)
            assert e.value.code == _lib.NUSI_EPARAM
            assert H.hipDeviceSynchronize() == 0
            assert np.all(np.isnan(dev.fetch(dO, (ROWS, P, 3))))
    finally:
        plan.close()
