"""nusi_libm.hpp's atan2 with the first-range vote (atan2_vote_t: atan2_i, atan2_w) on the host, where each vote is the
call's own predicate, so every call takes the path its own operands choose: bit for bit among atan2_i, atan2_w,
atan2_full (fdlibm's branches), atan2 without the new vote (atan2_slow) and the oracle's ora_atan2.

The host library tests/hostcheck_atan2 is built as tests/hostcheck_div is.  atan2_w is compared on the pairs inside
its operand bounds only (finite, moduli in [2^-500, 2^500], x possibly 0).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import atan2_cases as ac

DP = ctypes.POINTER(ctypes.c_double)
IP = ctypes.POINTER(ctypes.c_int)
D = ctypes.c_double


@pytest.fixture(scope="module")
def hlib():
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call(["make", "-s", "-C", os.path.join(here, "hostcheck_atan2")])
    return ctypes.CDLL(os.path.join(here, "_build", "libhostcheck_atan2.so"))


@pytest.fixture(scope="module")
def ora(oracle_mod):
    L = oracle_mod.lib()
    L.ora_atan2.restype = D
    L.ora_atan2.argtypes = [D, D]
    return L.ora_atan2


def _operands():
    rng = np.random.default_rng(20261020)
    ys, xs, kinds = [], [], []

    def add(y, x, k):
        y, x = np.asarray(y, np.float64).ravel(), np.asarray(x, np.float64).ravel()
        assert y.shape == x.shape, k
        ys.append(y); xs.append(x); kinds.append(np.full(y.size, k))

    n = 200000   # seeded pairs over 40 decades, all four sign combinations
    sx, sy = np.tile([1.0, 1.0, -1.0, -1.0], n // 4), np.tile([1.0, -1.0, 1.0, -1.0], n // 4)
    add(sy * 10.0 ** rng.uniform(-20, 20, n), sx * 10.0 ** rng.uniform(-20, 20, n), "seeded")
    n = 40000    # ... and with the quotient within two decades of 1, where the five ranges meet
    x = 10.0 ** rng.uniform(-20, 20, n) * rng.choice([-1.0, 1.0], n)
    add(x * 10.0 ** rng.uniform(-2, 2, n) * rng.choice([-1.0, 1.0], n), x, "near")
    # t at every range boundary and at 2^-29, +-1 ulp, exactly (x a power of two), four signs each
    tb = np.repeat(ac.boundary_ts(), 16)
    y, x = ac.pair(tb, rng, signs=False)
    s = np.tile([1.0, 1.0, -1.0, -1.0], tb.size // 4)
    add(y * np.tile([1.0, -1.0], tb.size // 2), x * s, "boundary")
    # ... the boundary's whole high word and the one below it (the votes and selects compare high words), random low words
    hw = np.repeat(np.array([h - d for h in ac.BOUNDS_HI + [ac.R_TINY] for d in (0, 1)], np.uint64), 1000)
    ts = ((hw << np.uint64(32)) | rng.integers(0, 2 ** 32, hw.size, dtype=np.uint64)).view(np.float64)
    y, x = ac.pair(ts, rng)
    add(y, x, "boundary_word")
    # ... and next to them through a rounded quotient: x with a full mantissa
    x = (1.0 + rng.random(tb.size)) * rng.choice([-1.0, 1.0], tb.size)
    add(tb * x * (1 + rng.integers(-2, 3, tb.size) * 2.0 ** -52), x, "boundary_rounded")
    # exponent differences of +-59, +-60 (and +-58, +-61), mantissas either way round
    for d in (58, 59, 60, 61):
        for sgn in (1, -1):
            m = 64
            e = rng.integers(-200, 200, m)
            add(np.ldexp(1.0 + rng.random(m), e + sgn * d) * rng.choice([-1.0, 1.0], m),
                np.ldexp(1.0 + rng.random(m), e) * rng.choice([-1.0, 1.0], m), "expdiff")
            add(np.ldexp(1.0, e + sgn * d), np.ldexp(np.nextafter(2.0, 1.0), e), "expdiff")
            add(np.ldexp(np.nextafter(2.0, 1.0), e + sgn * d), np.ldexp(1.0, e), "expdiff")
    # x = 1.0 (fdlibm's atan(y) shortcut; outside the common path), y through every range and both signs
    ty = np.concatenate([ac.boundary_ts(), 10.0 ** rng.uniform(-12, 12, 200)])
    add(np.concatenate([ty, -ty]), np.ones(2 * ty.size), "x_one")
    add(np.concatenate([ty, -ty]), -np.ones(2 * ty.size), "x_minus_one")
    # x = 0 (inside atan2_w's bounds, outside its vote)
    add(np.concatenate([ty, -ty]), np.zeros(2 * ty.size), "x_zero")
    # outside atan2_w's bounds: zeros, subnormals, infinities, NaN, the largest doubles
    sp = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, np.inf, -np.inf, np.nan, np.finfo(np.float64).max, 1.0, -3.0,
                   2.0 ** -501, 2.0 ** 501])
    g = np.array(np.meshgrid(sp, sp, indexing="ij")).reshape(2, -1)
    add(g[0], g[1], "special")
    return np.concatenate(ys), np.concatenate(xs), np.concatenate(kinds)


@pytest.fixture(scope="module")
def run(hlib, ora):
    y, x, kind = _operands()
    n = y.size
    ai, aw, af, asel = (np.empty(n) for _ in range(4))
    pi, pw = np.empty(n, np.int32), np.empty(n, np.int32)
    dp = lambda a: a.ctypes.data_as(DP)
    hlib.hc_atan2_n(n, dp(y), dp(x), dp(ai), dp(aw), dp(af), pi.ctypes.data_as(IP), pw.ctypes.data_as(IP))
    hlib.hc_atan2_slow_n(n, dp(y), dp(x), dp(asel))
    o = np.array([ora(float(a), float(b)) for a, b in zip(y, x)])
    r = dict(y=y, x=x, kind=kind, ai=ai, aw=aw, af=af, asel=asel, pi=pi, pw=pw, ora=o, inw=ac.w_bounds(y, x))
    for v in r.values():
        v.setflags(write=False)
    return r


def _report(r, bad, what):
    i = np.flatnonzero(bad)[:3]
    return "%s: %d differ, first %s" % (what, int(bad.sum()), [(str(r["kind"][j]), float.hex(float(r["y"][j])),
                                                                float.hex(float(r["x"][j]))) for j in i])


def test_every_path_is_taken(run):
    """The operands, before anything is compared: the paths the host library reports (flags set inside the bodies that
    ran; 8 added where a flagged call's bits differ from the plain call's) are the numpy model's, per call,
    and each of the three is taken often -- by atan2_i and, inside its bounds, by atan2_w; every range and both sides
    of every boundary occur on the common path."""
    y, x = run["y"], run["x"]
    assert y.size >= 240000
    assert np.array_equal(run["pi"], np.where(ac.plain(y, x), np.where(ac.first_range(y, x), 0, 1), 2))
    inw = run["inw"]
    assert np.array_equal(run["pw"][inw], np.where(ac.w_plain(y, x), np.where(ac.first_range(y, x), 0, 1), 2)[inw])
    for p in (run["pi"], run["pw"][inw]):
        assert [int((p == k).sum()) >= 1000 for k in (0, 1, 2)] == [True] * 3, np.bincount(p)
    with np.errstate(all="ignore"):
        t = np.abs(y / x)
    common = run["pi"] != 2
    for r in (-1, 0, 1, 2, 3):
        assert (ac.range_of(t[common]) == r).sum() >= 500, r
    assert (ac.hi(t[common]) < ac.R_TINY).sum() >= 100
    hb = set(ac.hi(t[common & (run["kind"] == "boundary")]).tolist())
    for h in ac.BOUNDS_HI + [ac.R_TINY]:
        assert h in hb and h - 1 in hb, hex(h)   # the boundary's high word, and the one below it (t - 1 ulp)
    # the common path's edges in the exponent difference: both sides of atan2_plain's k = +-60 occur
    ed = run["kind"] == "expdiff"
    assert (run["pi"][ed] == 2).sum() >= 100 and (run["pi"][ed] != 2).sum() >= 100
    assert (run["pw"][ed] == 2).sum() >= 100 and (run["pw"][ed] != 2).sum() >= 100
    assert (run["pi"][(run["kind"] == "x_one")] == 2).all()


@pytest.mark.parametrize("ref", ["atan2_full", "ora_atan2"])
def test_bit_identical(run, ref):
    """atan2_i on every pair, atan2_w on the pairs inside its bounds, and atan2_slow (no first-range vote),
    against fdlibm's branches in the same header and against the oracle's."""
    want = run["af"] if ref == "atan2_full" else run["ora"]
    bad = ~ac.same_bits(run["ai"], want)
    assert not bad.any(), _report(run, bad, "atan2_i vs " + ref)
    bad = ~ac.same_bits(run["aw"], want) & run["inw"]
    assert not bad.any(), _report(run, bad, "atan2_w vs " + ref)
    bad = ~ac.same_bits(run["asel"], want)
    assert not bad.any(), _report(run, bad, "atan2_slow vs " + ref)


def test_full_is_the_oracles(run):
    bad = ~ac.same_bits(run["af"], run["ora"])
    assert not bad.any(), _report(run, bad, "atan2_full vs ora_atan2")
