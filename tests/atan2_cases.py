"""Operands and numpy models shared by tests/test_atan2_range_vote.py (host) and tests/test_atan2_range_vote_gpu.py:
nusi_libm.hpp's atan2 votes restated on arrays, and operand pairs (y, x) with a chosen t = |y / x|.

A pair with a given t is (t * x, x) with x a power of two (never 1.0), so that y / x is t exactly, bit for bit.
"""
import numpy as np

R_FIRST = 0x3fdc0000    # s_atan.c: t < 0.4375, range -1
R_TINY = 0x3e200000     # t < 2^-29
BOUNDS_HI = [0x3fdc0000, 0x3fe60000, 0x3ff30000, 0x40038000]   # 7/16, 11/16, 19/16, 39/16: the starts of ranges 0 .. 3


def hi(x):
    return (np.ascontiguousarray(x, np.float64).view(np.uint64) >> np.uint64(32)).astype(np.int64).astype(np.int32)


def lo(x):
    return (np.ascontiguousarray(x, np.float64).view(np.uint64) & np.uint64(0xffffffff)).astype(np.int64)


def from_hi(h):
    return np.array([np.uint64(h) << np.uint64(32)], np.uint64).view(np.float64)[0]


def plain(y, x):
    """nm::atan2_plain: finite, nonzero, x != 1.0 and the exponent difference k within +-60"""
    hx, hy = hi(x).astype(np.int64), hi(y).astype(np.int64)
    ix, iy = hx & 0x7fffffff, hy & 0x7fffffff
    k = (iy - ix) >> 20
    return ((ix < 0x7ff00000) & (iy < 0x7ff00000) & ((ix | lo(x)) != 0) & ((iy | lo(y)) != 0)
            & ~((hx == 0x3ff00000) & (lo(x) == 0)) & (k <= 60) & (k >= -60))


def w_plain(y, x):
    """nm::atan2_w_plain (the products by 2^59 are exact inside atan2_w's operand bounds)"""
    ax, ay = np.abs(x), np.abs(y)
    with np.errstate(all="ignore"):
        return (ay <= ax * 2.0 ** 59) & (ax <= ay * 2.0 ** 59) & (x != 1.0)


def w_bounds(y, x):
    """atan2_w's operand bounds: finite, at most 2^500; y at least 2^-500; x at least 2^-500, or 0"""
    ax, ay = np.abs(x), np.abs(y)
    return np.isfinite(x) & np.isfinite(y) & (ax <= 2.0 ** 500) & (ay <= 2.0 ** 500) & (ay >= 2.0 ** -500) & \
        ((ax >= 2.0 ** -500) | (ax == 0))


def first_range(y, x):
    with np.errstate(all="ignore"):
        return hi(np.abs(y / x)) < R_FIRST


def range_of(t):
    """s_atan.c's range of t >= 0: -1, 0, 1, 2, 3"""
    h = hi(t)
    return -1 + sum((h >= b).astype(int) for b in BOUNDS_HI)


def paths(y, x, common):
    """per element: 0 the first-range path, 1 the select path, 2 the rare call -- element i is lane i % 64 of wave
    i / 64 (the last wave may be partial), common the per-lane predicate of the common path"""
    n = y.size
    pad = (-n) % 64
    c = np.concatenate([common, np.ones(pad, bool)]).reshape(-1, 64).all(axis=1)
    f = np.concatenate([first_range(y, x), np.ones(pad, bool)]).reshape(-1, 64).all(axis=1)
    return np.repeat(np.where(~c, 2, np.where(f, 0, 1)), 64)[:n].astype(np.int32)


def same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def pair(t, rng, signs=True):
    """(y, x) with |y / x| = t bit for bit: x = +-2^e, e in [-30, 30] without 0, y = +-t 2^e"""
    t = np.asarray(t, np.float64)
    e = rng.integers(1, 31, t.shape) * rng.choice([-1, 1], t.shape)
    x, y = np.ldexp(1.0, e), np.ldexp(t, e)
    if signs:
        x, y = x * rng.choice([-1.0, 1.0], t.shape), y * rng.choice([-1.0, 1.0], t.shape)
    return y, x


def t_in_range(r, n, rng):
    """n values of t inside range r (-1: [2^-29, 7/16)), log-uniform, clear of the ends"""
    ends = [2.0 ** -29, 0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 20]
    a, b = ends[r + 1], ends[r + 2]
    return np.exp(rng.uniform(np.log(a * 1.0001), np.log(b * 0.9999), n))


def boundary_ts():
    """every range boundary and 2^-29: the double whose high word is the boundary, and one ulp either side"""
    out = []
    for h in BOUNDS_HI + [R_TINY]:
        t0 = from_hi(h)
        out += [np.nextafter(t0, 0.0), t0, np.nextafter(t0, 4.0)]
    return np.array(out)
