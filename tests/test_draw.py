"""The detector layer's generator on the CPU: detector.philox4x32 / uniforms / loggam / draw_host, the numpy-only forms of
nusi_plan_draw_counts (include/nusi.h "Drawing counts"), and the host build of the device's own code for it
(nusi_draw.hpp through tests/hostcheck_draw), which must give draw_host's integers under the oracle's exp and log.

The statistical check: at the seed, stream and row below, 20 000 draws per expectation against the Poisson pmf, chi^2 over
the bins of expectation >= 5 (the rest pooled), |z| = |chi^2 - dof| / sqrt(2 dof) <= 4.  A fixed seed: nothing here is
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
MUS = (0.3, 3.0, 9.99, 10.0, 37.0, 1000.0)
D, DP = ctypes.c_double, ctypes.POINTER(ctypes.c_double)
UP = ctypes.POINTER(ctypes.c_uint)

KAT = (
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
)


@pytest.fixture(scope="module")
def hlib():
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call(["make", "-s", "-C", os.path.join(here, "hostcheck_draw")])
    L = ctypes.CDLL(os.path.join(here, "_build", "libhostcheck_draw.so"))
    L.hc_philox.argtypes = [UP, UP, UP]
    L.hc_loggam.restype, L.hc_loggam.argtypes = D, [D]
    L.hc_draw.argtypes = [DP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_uint, DP]
    return L


@pytest.fixture(scope="module")
def ora(oracle_mod):
    L = oracle_mod.lib()
    for f in (L.ora_exp, L.ora_log):
        f.restype, f.argtypes = D, [D]
    return L.ora_exp, L.ora_log


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert _hex(detector.philox4x32(ctr, key)) == want
        assert _hex(detector._philox(*ctr, *key)) == want
    # arrays broadcast, entry by entry the scalar form
    ctr = np.array([k[0] for k in KAT], dtype=np.uint64)
    key = np.array([k[1] for k in KAT], dtype=np.uint64)
    got = detector.philox4x32(ctr, key)
    assert got.dtype == np.uint32 and [_hex(g) for g in got] == [k[2] for k in KAT]
    with pytest.raises(ValueError):
        detector.philox4x32([0, 0, 0], [0, 0])
    with pytest.raises(ValueError):
        detector.philox4x32([2 ** 32, 0, 0, 0], [0, 0])


def test_philox_device_code_on_the_host(hlib):
    for ctr, key, want in KAT:
        c, k, o = (ctypes.c_uint * 4)(*ctr), (ctypes.c_uint * 2)(*key), (ctypes.c_uint * 4)()
        hlib.hc_philox(c, k, o)
        assert _hex(o) == want


def test_uniforms_range_and_bits():
    u = detector.uniforms([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [1 << 5, 0, 0, 1 << 6], [0x80000000, 0, 0x1F, 0x3F]])
    assert u.shape == (3, 2) and u.dtype == np.float64
    assert u[0, 0] == 0.0 and u[0, 1] == 1.0 - 2.0 ** -53           # the ends: 0 and the largest double below 1
    assert u[1, 0] == 2.0 ** -27 and u[1, 1] == 2.0 ** -53           # the lowest bit of either word that counts
    assert u[2, 0] == 0.5 and u[2, 1] == 0.0                         # the top bit; the dropped low bits
    rng = np.random.default_rng(7)
    x = rng.integers(0, 2 ** 32, (1000, 4), dtype=np.uint64)
    u = detector.uniforms(x)
    assert np.all(u >= 0.0) and np.all(u < 1.0)
    assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))    # 53 bits each
    assert np.array_equal((u[:, 0] * 2.0 ** 53).astype(np.uint64), ((x[:, 0] >> np.uint64(5)) << np.uint64(26)) + (x[:, 1] >> np.uint64(6)))
    # the scalar path of draw_host reads the same uniforms off the same block
    b = detector.philox4x32([3, 7 * 64 + 9, 5, 2], [SEED & 0xFFFFFFFF, SEED >> 32])
    assert tuple(detector.uniforms(b)) == detector._uniform2(SEED, 2, 5, 7, 9, 3)


def test_zero_expectation_draws_nothing():
    rounds = []
    x = detector.draw_host(np.zeros((2, 3)), 4, SEED, rounds=rounds)
    assert x.shape == (2, 4, 3) and not x.any() and not np.signbit(x).any()
    assert rounds == [0] * 24                                        # no block consumed
    assert detector.draw_host(np.zeros(3), 2, 1).shape == (2, 3)


def test_refusals():
    for bad in (np.nan, np.inf, -1.0):
        with pytest.raises(ValueError):
            detector.draw_host([1.0, bad], 2, 1)
    with pytest.raises(ValueError):
        detector.draw_host(np.ones(detector.BINS_MAX + 1), 2, 1)
    with pytest.raises(ValueError):
        detector.draw_host(np.ones(3), 0, 1)
    with pytest.raises(ValueError):
        detector.draw_host(np.ones(3), 2, 2 ** 64)
    with pytest.raises(ValueError):
        detector.draw_host(np.ones(3), 2, 1, stream=-1)
    # a mu that cannot be an input is defined all the same: NaN, no bits
    for bad in (np.nan, np.inf, -1.0):
        assert math.isnan(detector._draw_one(bad, 1, 0, 0, 0, 0, math.exp, math.log))


def test_a_sub_block_is_a_slice_of_the_whole_draw():
    rng = np.random.default_rng(3)
    mu = np.concatenate([rng.uniform(0, 9, (3, 4)), rng.uniform(10, 60, (3, 3))], axis=1)
    whole = detector.draw_host(mu, 6, SEED, stream=4)
    assert whole.shape == (3, 6, 7)
    assert np.array_equal(detector.draw_host(mu[:2, :5], 3, SEED, stream=4), whole[:2, :3, :5])   # rows, toys and bins from 0
    assert np.array_equal(detector.draw_host(mu[0], 6, SEED, stream=4), whole[0])                 # a vector is row 0
    assert np.array_equal(whole, np.floor(whole)) and np.all(whole >= 0)


def test_every_coordinate_of_the_identity_changes_the_block():
    base = dict(seed=SEED, stream=2, row=5, p=7, c=9, block=0)
    seen = {detector._uniform2(**base)}
    for k, v in (("seed", SEED ^ 1), ("seed", SEED ^ (1 << 40)), ("stream", 3), ("row", 6), ("p", 8), ("c", 10), ("block", 1)):
        seen.add(detector._uniform2(**dict(base, **{k: v})))
    assert len(seen) == 8
    # (p, c) and (p + 1, c - 64) would share a counter word: c < 64 keeps them apart
    assert detector.BINS_MAX == 64
    mu = np.full((2, 8), 5.0)
    a, b = detector.draw_host(mu, 16, 1, stream=0), detector.draw_host(mu, 16, 1, stream=1)
    c = detector.draw_host(mu, 16, 2, stream=0)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a[0], a[1])
    assert not np.array_equal(a[0, 0], a[0, 1]) and len(set(a[0, :, 0]) | set(a[0, :, 1])) > 3


def test_both_sides_of_the_threshold():
    below, at = np.nextafter(10.0, 0.0), 10.0
    r_lo, r_hi = [], []
    lo = detector.draw_host(np.full(32, below), 32, SEED, rounds=r_lo)
    hi = detector.draw_host(np.full(32, at), 32, SEED, rounds=r_hi)
    assert set(r_lo) == {1}                                          # inversion: one block, always
    assert min(r_hi) == 1 and max(r_hi) > 1 and max(r_hi) < detector.DRAW_PTRS_ROUNDS   # PTRS: some draws reject a round
    assert not np.array_equal(lo, hi)                                # another algorithm on the same bits
    for x in (lo, hi):
        assert abs(x.mean() - 10.0) < 5 * math.sqrt(10.0 / x.size) and abs(x.var() - 10.0) < 2.5
    # inversion is the inverse CDF of U0: checked against the pmf's partial sums in exact order
    u = detector._uniform2(SEED, 0, 0, 3, 4, 0)[0]
    k, F = 0, math.exp(-below)
    pk = F
    while not u < F:
        k += 1
        pk = (pk * below) / k
        F = F + pk
    assert lo[3, 4] == k


def test_loggam_against_lgamma():
    """detector.loggam against math.lgamma at x = 1 .. 2000.  The method is a truncated Stirling series with no derived
    bound: the largest deviation measured is 3.64e-12 (near x = 2000, where lgamma is 1.3e4 and one ulp is 1.8e-12), and
    the test asserts 4 x that."""
    dev = max(abs(detector.loggam(float(x), math.log) - math.lgamma(x)) for x in range(1, 2001))
    print("loggam: largest deviation from lgamma on 1 .. 2000: %.3e" % dev)
    assert dev <= 4 * 3.64e-12
    assert detector.loggam(1.0) == 0.0 and detector.loggam(2.0) == 0.0
    assert abs(detector.loggam(0.5, math.log) - math.lgamma(0.5)) < 1e-13       # the shift, off the integers
    assert abs(detector.loggam(6.999, math.log) - math.lgamma(6.999)) < 1e-13 and abs(detector.loggam(7.0, math.log) - math.lgamma(7.0)) < 1e-13


@pytest.mark.parametrize("mu", MUS)
def test_chi_square_against_the_pmf(mu):
    m = np.zeros((ROW + 1, 50))
    m[ROW] = mu
    rounds = []
    x = detector.draw_host(m, 400, SEED, stream=STREAM, exp=math.exp, log=math.log, rounds=rounds)
    assert not x[:ROW].any()
    x = x[ROW].ravel()
    n = x.size
    assert n == 20000 and np.array_equal(x, np.floor(x)) and x.min() >= 0
    kmax = int(mu + 20 * math.sqrt(mu) + 30)
    pmf = np.array([math.exp(-mu + k * math.log(mu) - math.lgamma(k + 1)) for k in range(kmax)])
    E, O = n * pmf, np.bincount(x.astype(np.int64), minlength=kmax)[:kmax]
    sel = E >= 5
    Er, Or = np.append(E[sel], n - E[sel].sum()), np.append(O[sel], n - O[sel].sum())    # the rest pooled into one bin
    if Er[-1] < 5:
        Er[-2], Or[-2] = Er[-2] + Er[-1], Or[-2] + Or[-1]
        Er, Or = Er[:-1], Or[:-1]
    dof = len(Er) - 1
    z = (((Or - Er) ** 2 / Er).sum() - dof) / math.sqrt(2 * dof)
    used = np.array(rounds[-n:])
    print("mu = %g: z = %.2f over %d bins, largest count %d, %.3f blocks per draw" % (mu, z, dof + 1, x.max(), used.mean()))
    assert abs(z) <= 4
    assert used.max() < detector.DRAW_PTRS_ROUNDS and (np.all(used == 1) if mu < 10 else 1.0 < used.mean() < 1.5)


def test_device_code_on_the_host_gives_draw_host(hlib, ora):
    """nusi_draw.hpp compiled for the CPU (the functions k_poisson_draw calls) against draw_host with the oracle's exp
    and log: every integer, at expectations on both sides of the split, the tiny, the huge and zero."""
    exp, log = ora
    mu = np.array([[0.0, 1e-300, 0.3, 9.999999, 10.0, 10.000001, 37.0, 1e3, 1e6, 1e12],
                   [2.5, 0.0, 7.0, 9.0, 11.0, 15.5, 100.0, 0.01, 3e4, 12.0]])
    for seed, stream in ((SEED, STREAM), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF)):
        P = 37
        out = np.full((2, P, mu.shape[1]), np.nan)
        hlib.hc_draw(mu.ctypes.data_as(DP), 2, mu.shape[1], P, seed, stream, out.ctypes.data_as(DP))
        want = detector.draw_host(mu, P, seed, stream=stream, exp=exp, log=log)
        assert np.array_equal(out, want)
        assert np.all(np.abs(out[0, :, 9] - 1e12) < 1e7) and not out[:, :, 0][0].any()
    for x in (1.0, 2.0, 3.0, 6.5, 7.0, 50.0, 1e6 + 1, 1e12 + 1):
        assert hlib.hc_loggam(x) == detector.loggam(x, log)


def test_header_constants_and_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "nusi.h")).read()
    assert "#define NUSI_DRAW_DATASETS_MAX %d\n" % detector.DRAW_DATASETS_MAX in text
    assert _lib.DRAW_DATASETS_MAX == detector.DRAW_DATASETS_MAX == 1 << 26
    assert "#define NUSI_DRAW_COUNTS_MAX %d\n" % _lib.DRAW_COUNTS_MAX in text and _lib.DRAW_COUNTS_MAX == (2 ** 31 - 1) * 256
    for name in ("nusi_plan_draw_counts", "nusi_plan_draw_counts_host"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in text
    for word in ("0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85"):
        assert word in text
    assert (detector.PHILOX_M0, detector.PHILOX_M1, detector.PHILOX_W0, detector.PHILOX_W1) == (
        0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85)
    L = _lib.load()
    assert L.nusi_plan_draw_counts.argtypes[5] is ctypes.c_ulonglong and L.nusi_plan_draw_counts_host.restype is ctypes.c_int
    # without a plan the calls refuse and say so
    assert L.nusi_plan_draw_counts_host(None, None, 1, 1, 1, 0, 0, None) in (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
