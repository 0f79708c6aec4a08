"""nusi_div.hpp on the GPU: the division with one refined reciprocal per divisor, bit for bit against the device's own
/ on the same operands and against numpy's division on the host.

The test-only kernel k_debug_div_shared (entry nusi_debug_div_shared, bound here with ctypes; not in nusi.h) takes
element i as lane i % 64 of wave i / 64 and returns div_shared2(a0, a1, b), div_shared(a0, b), the device's a0 / b
and a1 / b, and whether the element's wave voted the pair onto the short sequence (every lane's three operands finite,
nonzero and in [2^-380, 2^380)).  One launch serves every test of the module.

Operands: ~10^5 seeded triples across the window (exponents uniform in it, random mantissas and signs); mantissas of
all ones and 1 + ulp against each other; equal numerator and divisor; exponents at the window's two ends and one
step outside; whole waves inside the window; waves with one lane outside it, at a random lane (a zero, a subnormal,
an infinity, a NaN, 2^380, the double below 2^-380), whose wave must take the plain path; and waves of specials.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LO, HI = -380, 380   # the window [2^LO, 2^HI) of nusi_div.hpp (kDivLo, kDivHi)
ONES = float(np.nextafter(2.0, 1.0))       # mantissa of all ones
ONE_ULP = float(np.nextafter(1.0, 2.0))    # 1 + ulp


def _in_window(x):
    a = np.abs(x)
    return np.isfinite(x) & (a >= 2.0 ** LO) & (a < 2.0 ** HI)


def _operands():
    rng = np.random.default_rng(20261019)
    a0, a1, b, kind = [], [], [], []

    def add(x0, x1, d, k):
        x0, x1, d = (np.asarray(v, np.float64) for v in (x0, x1, d))
        assert x0.shape == x1.shape == d.shape and x0.size % 64 == 0, k   # whole waves per class
        a0.append(x0); a1.append(x1); b.append(d); kind.append(np.full(x0.size, k))

    def rnd(n, elo=LO, ehi=HI - 1):
        m = 1.0 + rng.random(n)
        return np.ldexp(m, rng.integers(elo, ehi + 1, n)) * rng.choice([-1.0, 1.0], n)

    n = 64 * 1600   # 102 400 seeded triples across the window: whole waves inside it
    add(rnd(n), rnd(n), rnd(n), 0)
    # mantissas of all ones and 1 + ulp, both signs, exponents through the window
    e = rng.integers(LO, HI - 1, 64 * 8)
    pat = np.array([ONES, ONE_ULP, 1.0, -ONES, -ONE_ULP, 1.5])
    m0, m1, md = (pat[rng.integers(0, pat.size, e.size)] for _ in range(3))
    add(np.ldexp(m0, e), np.ldexp(m1, rng.permutation(e)), np.ldexp(md, rng.permutation(e)), 1)
    # equal numerator and divisor (a1 its negative)
    x = rnd(64 * 4)
    add(x, -x, x, 2)
    # exponents at the window's ends: the smallest and the largest members, against each other
    ends = np.array([2.0 ** LO, np.nextafter(2.0 ** HI, 0.0), -(2.0 ** LO), -np.nextafter(2.0 ** HI, 0.0),
                     np.ldexp(ONE_ULP, LO), np.ldexp(ONES, HI - 1)])
    g = np.array(np.meshgrid(ends, ends, ends, indexing="ij")).reshape(3, -1)   # 216 triples
    pad = 256 - g.shape[1]
    g = np.concatenate([g, g[:, :pad]], axis=1)
    add(g[0], g[1], g[2], 3)
    # one lane of the wave outside the window, 63 inside: the wave takes the plain path
    outs = np.array([0.0, -0.0, 5e-324, 2.0 ** -1022, np.inf, -np.inf, np.nan, 2.0 ** HI, -(2.0 ** HI),
                     np.nextafter(2.0 ** LO, 0.0), -np.nextafter(2.0 ** LO, 0.0), 2.0 ** (HI + 1), 2.0 ** (LO - 1)])
    w = 3 * outs.size   # each outsider as a0, as a1 and as b
    x0, x1, d = rnd(64 * w), rnd(64 * w), rnd(64 * w)
    lanes = rng.integers(0, 64, w)
    for j in range(w):
        (x0, x1, d)[j % 3][64 * j + lanes[j]] = outs[j // 3]
    add(x0, x1, d, 4)
    # waves of specials and of operands one step and further outside: every combination of these values
    sp = np.array([0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1022, 2.0 ** -1000, 2.0 ** (LO - 1), 2.0 ** HI, 2.0 ** 1000,
                   np.finfo(np.float64).max, np.inf, -np.inf, np.nan, 1.0, -3.0, np.ldexp(ONES, -970)])
    g = np.array(np.meshgrid(sp, sp, sp, indexing="ij")).reshape(3, -1)   # 4096 triples
    add(g[0], g[1], g[2], 5)
    return tuple(np.concatenate(v) for v in (a0, a1, b, kind))


@pytest.fixture(scope="module")
def run():
    import nusiprop_amd
    from nusiprop_amd import _lib
    nusiprop_amd.load()
    L = ctypes.CDLL(_lib.LIB_PATH)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    L.nusi_debug_div_shared.restype = ctypes.c_int
    L.nusi_debug_div_shared.argtypes = [dp, dp, dp, ctypes.c_int] + [dp] * 5 + [ip]
    a0, a1, b, kind = _operands()
    n = a0.size
    outs = [np.empty(n) for _ in range(5)]
    fast = np.empty(n, np.int32)
    rc = L.nusi_debug_div_shared(*(v.ctypes.data_as(dp) for v in (a0, a1, b)), n, *(v.ctypes.data_as(dp) for v in outs),
                                 fast.ctypes.data_as(ip))
    assert rc == 0, rc
    with np.errstate(all="ignore"):
        h0, h1 = a0 / b, a1 / b
    for v in (a0, a1, b, kind, fast, h0, h1, *outs):
        v.setflags(write=False)
    return dict(a0=a0, a1=a1, b=b, kind=kind, q0=outs[0], q1=outs[1], s=outs[2], p0=outs[3], p1=outs[4], fast=fast,
                h0=h0, h1=h1)


def _same_bits(x, y):
    """bit for bit, every NaN equal to every NaN (the payload of a generated NaN is not part of RN(a / b))"""
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


def _report(r, bad, what):
    i = np.flatnonzero(bad)[:3]
    return "%s: %d differ, first %s" % (what, int(bad.sum()), [(int(j), float.hex(float(r["a0"][j])),
                                                              float.hex(float(r["a1"][j])), float.hex(float(r["b"][j]))) for j in i])


def test_vote_is_the_waves_window(run):
    """A wave takes the short sequence exactly when all 64 lanes' operands are in the window: the seeded waves, the
    patterns and the window's ends do, a wave with one lane outside does not, nor does any wave of specials with one."""
    ok = (_in_window(run["a0"]) & _in_window(run["a1"]) & _in_window(run["b"])).reshape(-1, 64)
    want = np.repeat(ok.all(axis=1), 64)
    assert np.array_equal(run["fast"] != 0, want)
    for k in (0, 1, 2, 3):
        assert want[run["kind"] == k].all(), k
    assert not want[run["kind"] == 4].any()
    assert ok[(run["kind"] == 4).reshape(-1, 64)[:, 0]].sum(axis=1).tolist() == [63] * (3 * 13)
    assert want.sum() >= 100000 and (~want).sum() >= 64 * 39


@pytest.mark.parametrize("ref", ["device", "numpy"])
def test_bit_identical_to_division(run, ref):
    """div_shared2's two quotients and div_shared's one against the device's own / (p0, p1) and numpy's (h0, h1), on
    every element -- the short sequence's waves and the plain path's alike."""
    r0, r1 = (run["p0"], run["p1"]) if ref == "device" else (run["h0"], run["h1"])
    for got, want, what in ((run["q0"], r0, "a0 / b of the pair"), (run["q1"], r1, "a1 / b of the pair"),
                            (run["s"], r0, "a0 / b alone")):
        bad = ~_same_bits(got, want)
        assert not bad.any(), _report(run, bad, what + " vs " + ref)


def test_device_division_is_numpys(run):
    """The two references agree with each other (the device's / is correctly rounded on these operands too)."""
    for got, want, what in ((run["p0"], run["h0"], "a0 / b"), (run["p1"], run["h1"], "a1 / b")):
        bad = ~_same_bits(got, want)
        assert not bad.any(), _report(run, bad, what)
