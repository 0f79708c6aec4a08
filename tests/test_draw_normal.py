"""The toys' normal generator on the CPU: detector.draw_normal_host, the numpy-only form of nusi_plan_draw_normals
(include/nusi.h "Drawing normals"), and the host build of the device's own code for it (nusi_draw.hpp's normal0 through
tests/hostcheck_normal), which must give draw_normal_host's bits under the oracle's log.

The statistical checks: at the seed, stream and row below, n = 20 000 draws.  At center = 10, sigma = 1 (the truncation
at 0 lies 10 sigma off: a plain normal) the mean within 4 sigma / sqrt(n) of 10 and the share of |z| < 1 within
4 sqrt(p q / n) of p = erf(1 / sqrt 2) = 0.682689.  At center = 0 (a half normal) every value >= 0 and the mean within 4
standard errors of sigma sqrt(2 / pi), the standard error sigma sqrt((1 - 2 / pi) / n).  A fixed seed: nothing here is
random between runs.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from nusiprop_amd import _lib, detector

SEED, STREAM, ROW = 0x0123456789ABCDEF, 2, 5
D, DP, IP = ctypes.c_double, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
N = 20000


@pytest.fixture(scope="module")
def hlib():
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call(["make", "-s", "-C", os.path.join(here, "hostcheck_normal")])
    L = ctypes.CDLL(os.path.join(here, "_build", "libhostcheck_normal.so"))
    L.hc_normal.argtypes = [DP, DP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_uint, DP, IP]
    L.hc_normal_block0.restype = ctypes.c_uint
    return L


@pytest.fixture(scope="module")
def ora_log(oracle_mod):
    f = oracle_mod.lib().ora_log
    f.restype, f.argtypes = D, [D]
    return f


def _sample(center, sigma):
    """N draws at (SEED, STREAM, ROW): 400 toys of 50 components."""
    c = np.zeros((ROW + 1, 50))
    c[ROW] = center
    rounds = []
    x = detector.draw_normal_host(c, sigma, 400, SEED, stream=STREAM, log=math.log, rounds=rounds)
    assert x.shape == (ROW + 1, 400, 50)
    return x[ROW].ravel(), np.array(rounds[-N:])


def test_the_rule_written_out():
    """One draw against the definition, step by step from the Philox block."""
    c, sg, p, j = 0.75, 0.5, 7, 3
    want, r = None, 0
    while want is None:
        b = detector.philox4x32([detector.NORMAL_BLOCK0 + r, p * 64 + j, ROW, STREAM], [SEED & 0xFFFFFFFF, SEED >> 32])
        u0, u1 = detector.uniforms(b)
        u, v = 2.0 * u0 - 1.0, 2.0 * u1 - 1.0
        s = u * u + v * v
        r += 1
        if not s < 1.0 or s == 0.0:
            continue
        x = c + sg * (u * math.sqrt((-2.0 * math.log(s)) / s))
        if x >= 0.0:
            want = x
    rounds = []
    got = detector._normal_one(c, sg, SEED, STREAM, ROW, p, j, math.log, rounds)
    assert got == want and rounds == [r]
    cc = np.zeros((ROW + 1, j + 1))
    cc[ROW, j] = c
    assert detector.draw_normal_host(cc, sg, p + 1, SEED, stream=STREAM, log=math.log)[ROW, p, j] == want


def test_no_prior_draws_nothing():
    rounds = []
    c = np.array([[0.0, 0.3, 50.0], [1.0, 2.0, 3.0]])
    x = detector.draw_normal_host(c, np.inf, 4, SEED, rounds=rounds)
    assert x.shape == (2, 4, 3) and np.array_equal(x, np.broadcast_to(c[:, None, :], x.shape))
    assert rounds == [0] * 24                                        # no block consumed
    # one component without a prior among others with one
    x = detector.draw_normal_host(c, [1.0, np.inf, 1.0], 4, SEED)
    assert np.array_equal(x[:, :, 1], np.broadcast_to(c[:, None, 1], (2, 4))) and not np.array_equal(x[:, :, 0], x[:, :, 2])
    assert detector.draw_normal_host(np.ones(3), 1.0, 2, 1).shape == (2, 3)


def test_refusals():
    for bad in (np.nan, np.inf, -1.0):
        with pytest.raises(ValueError):
            detector.draw_normal_host([1.0, bad], 1.0, 2, 1)
    for bad in (np.nan, 0.0, -1.0):
        with pytest.raises(ValueError):
            detector.draw_normal_host([1.0, 1.0], [1.0, bad], 2, 1)
    with pytest.raises(ValueError):
        detector.draw_normal_host(np.ones(detector.BINS_MAX + 1), 1.0, 2, 1)
    with pytest.raises(ValueError):
        detector.draw_normal_host(np.ones((2, 2, 2)), 1.0, 2, 1)
    with pytest.raises(ValueError):
        detector.draw_normal_host(np.ones(3), 1.0, 0, 1)
    with pytest.raises(ValueError):
        detector.draw_normal_host(np.ones(3), 1.0, 2, 2 ** 64)
    with pytest.raises(ValueError):
        detector.draw_normal_host(np.ones(3), 1.0, 2, 1, stream=-1)
    assert detector.draw_normal_host(np.ones(detector.BINS_MAX), 1.0, 1, 1).shape == (1, detector.BINS_MAX)


def test_a_sub_block_is_a_slice_of_the_whole_draw():
    rng = np.random.default_rng(3)
    c, sg = rng.uniform(0, 3, (3, 7)), rng.uniform(0.1, 2, 7)
    whole = detector.draw_normal_host(c, sg, 6, SEED, stream=4)
    assert whole.shape == (3, 6, 7) and np.all(whole >= 0)
    assert np.array_equal(detector.draw_normal_host(c[:2, :5], sg[:5], 3, SEED, stream=4), whole[:2, :3, :5])
    assert np.array_equal(detector.draw_normal_host(c[0], sg, 6, SEED, stream=4), whole[0])       # a vector is row 0


def test_every_coordinate_of_the_identity_changes_the_draw():
    base = dict(seed=SEED, stream=2, row=5, p=7, j=9)
    seen = {detector._normal_one(1.0, 1.0, log=math.log, **base)}
    for k, v in (("seed", SEED ^ 1), ("seed", SEED ^ (1 << 40)), ("stream", 3), ("row", 6), ("p", 8), ("j", 10)):
        seen.add(detector._normal_one(1.0, 1.0, log=math.log, **dict(base, **{k: v})))
    assert len(seen) == 7
    # the block word separates the normals from the counts of the same identity: none of the counts' 64 blocks
    assert detector.NORMAL_BLOCK0 == 0x80000000 and detector.NORMAL_BLOCK0 > detector.DRAW_PTRS_ROUNDS
    assert detector.NORMAL_BLOCK0 + detector.NORMAL_ROUNDS - 1 < 2 ** 32
    blocks = {detector._uniform2(SEED, 2, 5, 7, 9, b) for b in list(range(64)) + [detector.NORMAL_BLOCK0 + r for r in range(64)]}
    assert len(blocks) == 128
    # the counts do not move when normals are drawn: the generator keeps no state
    mu = np.full((2, 8), 5.0)
    a = detector.draw_host(mu, 4, SEED)
    detector.draw_normal_host(np.ones((2, 8)), 1.0, 4, SEED)
    assert np.array_equal(a, detector.draw_host(mu, 4, SEED))


def test_rounds_consumed():
    """The polar method accepts a round with probability pi / 4; at center = 0 half of the accepted are negative."""
    _, used = _sample(10.0, 1.0)
    assert used.min() == 1 and 1 < used.max() < detector.NORMAL_ROUNDS
    assert abs(used.mean() - 4 / math.pi) < 4 * math.sqrt((1 - math.pi / 4) / (math.pi / 4) ** 2 / N)
    _, used0 = _sample(0.0, 1.0)
    pa = math.pi / 8
    assert abs(used0.mean() - 1 / pa) < 4 * math.sqrt((1 - pa) / pa ** 2 / N)
    # exhaustion -- all 64 rounds rejected -- gives the center: forced here by a log of NaN, which fails x >= 0 in every round
    rounds = []
    x = detector._normal_one(1.0, 1.0, SEED, 0, 0, 0, 0, lambda s: float("nan"), rounds)
    assert x == 1.0 and rounds == [detector.NORMAL_ROUNDS]


def test_distribution_of_a_plain_normal():
    x, _ = _sample(10.0, 1.0)
    assert x.size == N
    print("center 10, sigma 1: mean %.5f, share |z| < 1 %.5f" % (x.mean(), np.mean(np.abs(x - 10.0) < 1.0)))
    assert abs(x.mean() - 10.0) < 4 * 1.0 / math.sqrt(N)
    pin = 0.682689
    assert abs(np.mean(np.abs(x - 10.0) < 1.0) - pin) < 4 * math.sqrt(pin * (1 - pin) / N)


@pytest.mark.parametrize("sigma", (1.0, 0.05))
def test_distribution_at_the_boundary(sigma):
    x, _ = _sample(0.0, sigma)
    assert x.size == N and np.all(x >= 0.0) and not np.signbit(x).any()
    want, se = sigma * math.sqrt(2 / math.pi), sigma * math.sqrt((1 - 2 / math.pi) / N)
    print("center 0, sigma %g: mean %.6f (half normal %.6f, s.e. %.6f)" % (sigma, x.mean(), want, se))
    assert abs(x.mean() - want) < 4 * se


def test_device_code_on_the_host_gives_draw_normal_host(hlib, ora_log):
    """nusi_draw.hpp's normal0 compiled for the CPU against draw_normal_host with the oracle's log: every bit and every
    count of blocks, over centers from 0 up, widths from narrow to wider than the center, and no prior."""
    center = np.array([[0.0, 0.0, 0.3, 0.3, 1.0, 1.0, 50.0, 50.0, 1e-300, 1e6, 0.7],
                       [2.5, 0.0, 7.0, 0.01, 11.0, 15.5, 100.0, 0.01, 3e4, 12.0, 0.0]])
    sigma = np.array([0.05, 1.0, 0.05, 1.0, 1.0, 3.0, 0.05, 100.0, 1.0, 1e-3, np.inf])
    rows, J = center.shape
    assert hlib.hc_normal_rounds() == detector.NORMAL_ROUNDS == _lib.NORMAL_ROUNDS
    assert hlib.hc_normal_block0() == detector.NORMAL_BLOCK0
    for seed, stream in ((SEED, STREAM), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF)):
        P = 37
        out, used = np.full((rows, P, J), np.nan), np.full((rows, P, J), -1, dtype=np.int32)
        hlib.hc_normal(center.ctypes.data_as(DP), sigma.ctypes.data_as(DP), rows, J, P, seed, stream, out.ctypes.data_as(DP),
                       used.ctypes.data_as(IP))
        rounds = []
        want = detector.draw_normal_host(center, sigma, P, seed, stream=stream, log=ora_log, rounds=rounds)
        assert np.array_equal(out, want) and np.all(out >= 0)
        assert np.array_equal(used.ravel(), np.array(rounds))
        assert np.array_equal(out[:, :, J - 1], np.broadcast_to(center[:, None, J - 1], (rows, P))) and not used[:, :, J - 1].any()
        assert used[:, :, :J - 1].min() >= 1
        # without the count of blocks: the same values
        out2 = np.full((rows, P, J), np.nan)
        hlib.hc_normal(center.ctypes.data_as(DP), sigma.ctypes.data_as(DP), rows, J, P, seed, stream, out2.ctypes.data_as(DP), None)
        assert np.array_equal(out, out2)


def test_header_constants_and_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "nusi.h")).read()
    hpp = open(os.path.join(root, "nusiprop_amd", "csrc", "nusi_draw.hpp")).read()
    assert "#define NUSI_NORMAL_ROUNDS %d\n" % detector.NORMAL_ROUNDS in text and _lib.NORMAL_ROUNDS == detector.NORMAL_ROUNDS == 64
    assert "kNormalRounds = %d" % detector.NORMAL_ROUNDS in hpp and "kNormalBlock0 = 0x%Xu" % detector.NORMAL_BLOCK0 in hpp
    assert "0x80000000 + r" in text and "Drawing normals" in text
    for name in ("nusi_plan_draw_normals", "nusi_plan_draw_normals_host"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in text
    for name, val in (("NUSI_OPT_TOY_NUISANCE", _lib.OPT_TOY_NUISANCE), ("NUSI_TOYS_FIXED", _lib.TOYS_FIXED),
                      ("NUSI_TOYS_GLOBAL", _lib.TOYS_GLOBAL), ("NUSI_TOYS_PRIOR", _lib.TOYS_PRIOR)):
        assert "#define %s %d\n" % (name, val) in text
    assert (_lib.OPT_TOY_NUISANCE, _lib.TOYS_FIXED, _lib.TOYS_GLOBAL, _lib.TOYS_PRIOR) == (17, 0, 1, 2)
    assert (detector.TOYS_FIXED, detector.TOYS_GLOBAL, detector.TOYS_PRIOR) == (0, 1, 2)
    L = _lib.load()
    assert L.nusi_plan_draw_normals.argtypes[6] is ctypes.c_ulonglong and L.nusi_plan_draw_normals_host.restype is ctypes.c_int
    # without a plan the calls refuse and say so
    assert L.nusi_plan_draw_normals_host(None, None, None, 1, 1, 1, 0, 0, None) in (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_set_option(None, _lib.OPT_TOY_NUISANCE, _lib.TOYS_GLOBAL) == _lib.NUSI_EPARAM
