"""nusi_libm.hpp's atan2 with the first-range wave vote on the GPU: bit for bit against the oracle's ora_atan2 and the
device's own atan2_full, with the path each wave took asserted.

The test-only kernel k_debug_atan2 (entry nusi_debug_atan2, bound here with ctypes; not in nusi.h) takes element i as
lane i % 64 of wave i / 64 and returns atan2_i, atan2_w and atan2_full of (y, x), and the path of the element's wave
in atan2_i and in atan2_w: 0 the first-range vote's short body, 1 the select path, 2 the rare call (fdlibm's
branches), each flag set inside the body that ran.  One launch serves every test of the module.

Waves (64 lanes each; ~20 000 pairs): uniform in range -1 (t = |y / x| < 0.4375); range -1 with one lane at a random
position in each other range, or exactly on a boundary -- the vote must fail and the select path run; range -1 with
one lane below 2^-29 -- the vote holds, the lane takes the select of t; one lane outside the common path (x = 1, x =
0, exponents 62 apart: both votes; y = 0, an infinity, a NaN: atan2_i's, atan2_w not compared) -- the rare call;
seeded mixed waves; and a partial last wave of 37 lanes, uniform in range -1.
"""
import ctypes

import numpy as np
import pytest

from tests import atan2_cases as ac

pytestmark = pytest.mark.gpu
LAST = 37   # lanes of the partial last wave


def _operands():
    rng = np.random.default_rng(20261021)
    ys, xs, kinds, wok = [], [], [], []

    def add(y, x, k, w_ok=True):
        y, x = np.asarray(y, np.float64).ravel(), np.asarray(x, np.float64).ravel()
        assert y.shape == x.shape and (y.size % 64 == 0 or k == "partial"), k
        ys.append(y); xs.append(x); kinds.append(np.full(y.size, k)); wok.append(np.full(y.size, w_ok))

    def first(nw):   # nw waves uniform in range -1, every sign combination
        return ac.pair(ac.t_in_range(-1, 64 * nw, rng), rng)

    y, x = first(100)
    add(y, x, "first")
    # ... with rounded quotients: x of a full mantissa (t within range -1 by a margin)
    x = np.ldexp(1.0 + rng.random(64 * 40), rng.integers(-40, 40, 64 * 40)) * rng.choice([-1.0, 1.0], 64 * 40)
    add(x * ac.t_in_range(-1, x.size, rng) * 0.99 * rng.choice([-1.0, 1.0], x.size), x, "first")
    # one lane in another range, 63 in range -1
    for r in (0, 1, 2, 3):
        y, x = first(8)
        lanes = 64 * np.arange(8) + rng.integers(0, 64, 8)
        y[lanes], x[lanes] = ac.pair(ac.t_in_range(r, 8, rng), rng)
        add(y, x, "one_in_%d" % r)
    # one lane exactly on a boundary (the first of range 0, 1, 2, 3), or one ulp below 7/16 (still range -1)
    tb = ac.boundary_ts()
    for j, k in ((1, "one_at_0"), (4, "one_at_1"), (7, "one_at_2"), (10, "one_at_3"), (0, "one_below_0")):
        y, x = first(4)
        lanes = 64 * np.arange(4) + rng.integers(0, 64, 4)
        y[lanes], x[lanes] = ac.pair(np.full(4, tb[j]), rng)
        add(y, x, k)
    # one lane below 2^-29 (2^-29 - 1 ulp, and far below), 63 in range -1; and whole waves below it
    y, x = first(8)
    lanes = 64 * np.arange(8) + rng.integers(0, 64, 8)
    y[lanes], x[lanes] = ac.pair(np.concatenate([np.full(4, tb[12]), 2.0 ** rng.uniform(-58, -30, 4)]), rng)
    add(y, x, "one_tiny")
    add(*ac.pair(2.0 ** rng.uniform(-58, -29.01, 128), rng), "tiny")
    # one lane outside the common path: of both atan2_i and atan2_w ...
    y, x = first(6)
    lanes = 64 * np.arange(6) + rng.integers(0, 64, 6)
    x[lanes[0:2]] = 1.0
    x[lanes[2:4]] = 0.0
    y[lanes[4]], x[lanes[4]] = 2.0 ** 40, -(2.0 ** -22)
    y[lanes[5]], x[lanes[5]] = -(2.0 ** -31), 2.0 ** 31
    add(y, x, "one_rare")
    # ... and of atan2_i alone (operands outside atan2_w's bounds: its results are not compared on these waves)
    y, x = first(6)
    lanes = 64 * np.arange(6) + rng.integers(0, 64, 6)
    y[lanes[0]] = 0.0
    y[lanes[1]] = -0.0
    y[lanes[2]] = np.inf
    x[lanes[3]] = -np.inf
    y[lanes[4]] = np.nan
    x[lanes[5]] = 5e-324
    add(y, x, "one_rare_i", w_ok=False)
    # seeded mixed waves: quotients within two decades of 1
    n = 64 * 120
    x = 10.0 ** rng.uniform(-20, 20, n) * rng.choice([-1.0, 1.0], n)
    add(x * 10.0 ** rng.uniform(-2, 2, n) * rng.choice([-1.0, 1.0], n), x, "mixed")
    # the partial last wave
    add(*ac.pair(ac.t_in_range(-1, LAST, rng), rng), "partial")
    return tuple(np.concatenate(v) for v in (ys, xs, kinds, wok))


@pytest.fixture(scope="module")
def run(oracle_mod):
    import nusiprop_amd
    from nusiprop_amd import _lib
    nusiprop_amd.load()
    L = ctypes.CDLL(_lib.LIB_PATH)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    L.nusi_debug_atan2.restype = ctypes.c_int
    L.nusi_debug_atan2.argtypes = [dp, dp, ctypes.c_int, dp, dp, dp, ip, ip]
    y, x, kind, wok = _operands()
    n = y.size
    ai, aw, af = (np.empty(n) for _ in range(3))
    pi, pw = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    rc = L.nusi_debug_atan2(y.ctypes.data_as(dp), x.ctypes.data_as(dp), n, *(v.ctypes.data_as(dp) for v in (ai, aw, af)),
                            pi.ctypes.data_as(ip), pw.ctypes.data_as(ip))
    assert rc == 0, rc
    O = oracle_mod.lib()
    O.ora_atan2.restype = ctypes.c_double
    O.ora_atan2.argtypes = [ctypes.c_double, ctypes.c_double]
    ora = np.array([O.ora_atan2(float(a), float(b)) for a, b in zip(y, x)])
    r = dict(y=y, x=x, kind=kind, wok=wok, ai=ai, aw=aw, af=af, pi=pi, pw=pw, ora=ora)
    for v in r.values():
        v.setflags(write=False)
    return r


def _report(r, bad, what):
    i = np.flatnonzero(bad)[:3]
    return "%s: %d differ, first %s" % (what, int(bad.sum()), [(int(j), str(r["kind"][j]), float.hex(float(r["y"][j])),
                                                                float.hex(float(r["x"][j]))) for j in i])


def test_operands_put_waves_on_every_path(run):
    """From the operands alone (numpy's model of the two votes, per wave of 64): each class of waves takes the path
    it was built for, in atan2_i and in atan2_w."""
    y, x, kind = run["y"], run["x"], run["kind"]
    assert 19000 <= y.size <= 22000 and y.size % 64 == LAST
    assert ac.w_bounds(y, x)[run["wok"]].all()
    for common, name in ((ac.plain(y, x), "atan2_i"), (ac.w_plain(y, x), "atan2_w")):
        p = ac.paths(y, x, common)
        ok = run["wok"] if name == "atan2_w" else np.ones(y.size, bool)
        for k in ("first", "one_below_0", "one_tiny", "tiny", "partial"):
            assert (p[kind == k] == 0).all(), (name, k)
        for k in ["one_in_%d" % r for r in range(4)] + ["one_at_%d" % r for r in range(4)]:
            assert (p[kind == k] == 1).all(), (name, k)
        assert (p[kind == "one_rare"] == 2).all(), name
        assert (ac.paths(y, x, ac.plain(y, x))[kind == "one_rare_i"] == 2).all()
        waves = [int((p[ok] == j).sum()) // 64 for j in (0, 1, 2)]
        assert min(waves) >= 6, (name, waves)
    # exactly one lane off range -1 in the one-lane classes, at t >= 7/16
    with np.errstate(all="ignore"):
        t = np.abs(y / np.where(x == 0, 1.0, x))
    for k in ["one_in_%d" % r for r in range(4)] + ["one_at_%d" % r for r in range(4)]:
        off = (ac.range_of(t[kind == k]) >= 0).reshape(-1, 64).sum(axis=1)
        assert (off == 1).all(), (k, off)
    for r in range(4):
        assert (ac.range_of(t[kind == "one_in_%d" % r]).reshape(-1, 64).max(axis=1) == r).all(), r
    tiny = (ac.hi(t[kind == "one_tiny"]) < ac.R_TINY).reshape(-1, 64).sum(axis=1)
    assert (tiny == 1).all()
    mixed = ac.range_of(t[kind == "mixed"])
    assert [int((mixed == r).sum()) >= 200 for r in (-1, 0, 1, 2, 3)] == [True] * 5


def test_path_flags(run):
    """The path every wave took on the device is the model's: the first-range vote holds exactly when all of the
    wave's (active) lanes are in range -1, and a wave with a lane outside the common path takes the rare call.  The
    flags are written inside the bodies that ran (atan2_vote_t<.., true>, atan2_slow_body), not restated beside the
    calls; the kernel adds 8 where such a flagged call's bits differ from atan2_i's / atan2_w's own, so equality
    with the model (values 0, 1, 2) also holds the flagged instances to the library's."""
    y, x = run["y"], run["x"]
    assert np.array_equal(run["pi"], ac.paths(y, x, ac.plain(y, x)))
    w = run["wok"]
    assert np.array_equal(run["pw"][w], ac.paths(y, x, ac.w_plain(y, x))[w])


@pytest.mark.parametrize("ref", ["ora_atan2", "device atan2_full"])
def test_bit_identical(run, ref):
    want = run["ora"] if ref == "ora_atan2" else run["af"]
    bad = ~ac.same_bits(run["ai"], want)
    assert not bad.any(), _report(run, bad, "atan2_i vs " + ref)
    bad = ~ac.same_bits(run["aw"], want) & run["wok"]
    assert not bad.any(), _report(run, bad, "atan2_w vs " + ref)


def test_device_full_is_the_oracles(run):
    bad = ~ac.same_bits(run["af"], run["ora"])
    assert not bad.any(), _report(run, bad, "device atan2_full vs ora_atan2")
