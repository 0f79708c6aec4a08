"""nusi_div.hpp's short sequence without a vote -- div_v(true, ..) and div2_v(true, ..), the forms k_alpha_mcorner's call
chain uses with bounds its callers derive themselves -- on the GPU, bit for bit against the device's own / and numpy's.

tests/test_div_shared_gpu.py drives the self-voting forms, whose window [2^-380, 2^380) excludes zeros and is
narrower than what the call sites rely on.  Here the test-only kernel k_debug_div_forced (entry nusi_debug_div_forced,
ctypes, not in nusi.h) runs the short sequence on every element, whatever its wave holds.  One launch; a class per
reliance (each whole waves, random and all-ones / 1 + ulp mantissas, both signs unless said):

  zero     numerator +0 over a positive divisor in [2^-500, 2^500) -- atan2_sel_t<true>'s num for t = 0.5, 1, 1.5,
           cseries_t's x / r for a reflected 1 - x = +0 -- alone, as either member of a pair, and as both
  cseries  x / r, y / r: numerators in [2^-403, 2), r in [2^-400, 0.98]
  inverse  x / r2, -y / r2: numerators in [2^-201, 2^100], r2 in [1, 2^201]
  smith    Smith's ratio and pair: operands in [2^-150, 2^51]
  hypot    r / (2 h): |r| in [2^-900, 2^150), 2 h in [2^-499, 2^102]
  tx       t_x, t_y: numerators in [2^-700, 8), r^2 in (2^-4, 1)
  atan2q   y / x: operands in [2^-500, 2^500), exponents at most 59 apart
  atan2r   num / den: |num| in [2^-61, 2^59), den in [1, 2^60)
  kmax     18 and 22 over -log r in [0.02, 278]
  edges    the ends of the header's conditions: numerators at 2^-969; exponents 767 apart; the quotient at 2^-1021;
           divisors at 2^1021 and at 2^-1022
"""
import ctypes

import numpy as np
import pytest

from tests.test_div_shared_gpu import ONE_ULP, ONES, _report, _same_bits

pytestmark = pytest.mark.gpu

CLASSES = ["zero", "cseries", "inverse", "smith", "hypot", "tx", "atan2q", "atan2r", "kmax", "edges"]


def _operands():
    rng = np.random.default_rng(1019)
    pat = np.array([ONES, ONE_ULP, 1.0, 1.5])

    def mant(n):
        m = 1.0 + rng.random(n)
        k = rng.random(n) < 0.25
        m[k] = pat[rng.integers(0, pat.size, int(k.sum()))]
        return m

    def rnd(n, elo, ehi, signed=True, ends=True):
        """mantissa 2^e, e uniform in [elo, ehi]; the first elements at the two end exponents"""
        e = rng.integers(elo, ehi + 1, n)
        if ends:
            e[:8] = [elo, elo, ehi, ehi, elo, ehi, elo, ehi]
        v = np.ldexp(mant(n), e)
        if ends:
            v[:2] = [np.ldexp(1.0, elo), np.ldexp(ONES, ehi)]
        return v * rng.choice([-1.0, 1.0], n) if signed else v

    n = 64 * 16
    out = {}
    z = np.zeros(n)
    pos = rnd(n, -500, 499, signed=False)
    out["zero"] = (np.concatenate([z, z, rnd(n, -403, 0), z]), np.concatenate([z, rnd(n, -403, 0), z, rnd(n, -403, 0)]),
                   np.concatenate([pos, rng.permutation(pos), pos, rng.permutation(pos)]))
    r = np.minimum(rnd(n, -400, -1, signed=False), 0.98)
    out["cseries"] = (rnd(n, -403, 0), rng.permutation(rnd(n, -403, 0)), r)
    out["inverse"] = (rnd(n, -201, 99), rng.permutation(rnd(n, -201, 99)), rng.permutation(rnd(n, 0, 200, signed=False)))
    out["smith"] = (rnd(n, -150, 50), rng.permutation(rnd(n, -150, 50)), rng.permutation(rnd(n, -150, 50)))
    out["hypot"] = (rnd(n, -900, 149), rng.permutation(rnd(n, -900, 149)), rng.permutation(rnd(n, -499, 101, signed=False)))
    out["tx"] = (rnd(n, -700, 2), rng.permutation(rnd(n, -700, 2)), rnd(n, -4, -1, signed=False, ends=False))
    x = rnd(n, -440, 439)
    out["atan2q"] = (x * np.ldexp(mant(n), rng.integers(-59, 59, n)), x * np.ldexp(mant(n), rng.integers(-59, 59, n)),
                     x)
    out["atan2r"] = (rnd(n, -61, 58), rng.permutation(rnd(n, -61, 58)), rng.permutation(rnd(n, 0, 59, signed=False)))
    out["kmax"] = (np.full(n, 18.0), np.full(n, 22.0), np.clip(rnd(n, -6, 8, signed=False, ends=False), 0.02, 278.0))
    q = n // 4
    sg = lambda k: rng.choice([-1.0, 1.0], k)   # noqa: E731
    ea0 = np.concatenate([np.ldexp(mant(q), -969) * sg(q),                      # numerator at 2^-969 ...
                          np.ldexp(mant(q), 400) * sg(q),                       # exponents 767 apart
                          np.ldexp(mant(q), rng.integers(300, 1000, q)) * sg(q),   # divisor at 2^1021
                          np.ldexp(mant(q), rng.integers(-969, -256, q)) * sg(q)])  # divisor at 2^-1022
    ea1 = np.concatenate([np.ldexp(mant(q), -969) * sg(q), np.ldexp(mant(q), 400) * sg(q),
                          np.ldexp(mant(q), rng.integers(300, 1000, q)) * sg(q),
                          np.ldexp(mant(q), rng.integers(-969, -256, q)) * sg(q)])
    eb = np.concatenate([np.ldexp(mant(q), rng.choice([-1000, 0, 52], q)) * sg(q),   # ... the quotient down at 2^-1021
                         np.ldexp(mant(q), -367) * sg(q),
                         np.ldexp(mant(q), 1021) * sg(q),
                         np.ldexp(mant(q), -1022) * sg(q)])
    out["edges"] = (ea0, ea1, eb)
    a0, a1, b, kind = [], [], [], []
    for k, name in enumerate(CLASSES):
        x0, x1, d = out[name]
        assert x0.size == x1.size == d.size and x0.size % 64 == 0, name
        a0.append(x0); a1.append(x1); b.append(d); kind.append(np.full(x0.size, k))
    return tuple(np.concatenate(v) for v in (a0, a1, b, kind))


@pytest.fixture(scope="module")
def run():
    import nusiprop_amd
    from nusiprop_amd import _lib
    nusiprop_amd.load()
    L = ctypes.CDLL(_lib.LIB_PATH)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    L.nusi_debug_div_forced.restype = ctypes.c_int
    L.nusi_debug_div_forced.argtypes = [dp, dp, dp, ctypes.c_int] + [dp] * 5 + [ip]
    a0, a1, b, kind = _operands()
    n = a0.size
    outs = [np.empty(n) for _ in range(5)]
    fast = np.zeros(n, np.int32)
    rc = L.nusi_debug_div_forced(*(v.ctypes.data_as(dp) for v in (a0, a1, b)), n, *(v.ctypes.data_as(dp) for v in outs),
                                 fast.ctypes.data_as(ip))
    assert rc == 0, rc
    assert fast.all()   # (the forced kernel ran, not the voting one)
    with np.errstate(all="ignore"):
        h0, h1 = a0 / b, a1 / b
    for v in (a0, a1, b, kind, h0, h1, *outs):
        v.setflags(write=False)
    return dict(a0=a0, a1=a1, b=b, kind=kind, q0=outs[0], q1=outs[1], s=outs[2], p0=outs[3], p1=outs[4], h0=h0, h1=h1)


def test_operands_meet_the_headers_conditions(run):
    """What the short sequence is promised (nusi_div.hpp): divisor finite, nonzero, normal with a normal reciprocal;
    numerator +0 over a positive divisor, or finite, at least 2^-969, its exponent less than 768 above the divisor's
    and the quotient normal."""
    b = run["b"]
    assert np.all(np.isfinite(b) & (np.abs(b) >= 2.0 ** -1022) & (np.abs(b) < 2.0 ** 1022))
    for a, h in ((run["a0"], run["h0"]), (run["a1"], run["h1"])):
        zero = a == 0
        assert np.all(~np.signbit(a[zero]) & (b[zero] > 0))
        ea, eb = np.frexp(a[~zero])[1], np.frexp(b[~zero])[1]
        assert np.all(np.isfinite(a)) and np.all(np.abs(a[~zero]) >= 2.0 ** -969)
        assert np.all(ea - eb < 768) and np.all(np.abs(h[~zero]) >= 2.0 ** -1022) and np.all(np.isfinite(h))
    assert (run["kind"] == CLASSES.index("zero")).sum() >= 4096 and ((run["a0"] == 0) & (run["a1"] == 0)).sum() >= 1024


@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("ref", ["device", "numpy"])
def test_forced_short_sequence_bit_identical(run, name, ref):
    sel = run["kind"] == CLASSES.index(name)
    r0, r1 = (run["p0"], run["p1"]) if ref == "device" else (run["h0"], run["h1"])
    for got, want, what in ((run["q0"], r0, "a0 / b of the pair"), (run["q1"], r1, "a1 / b of the pair"),
                            (run["s"], r0, "a0 / b alone")):
        bad = sel & ~_same_bits(got, want)
        assert not bad.any(), _report(run, bad, "%s: %s vs %s" % (name, what, ref))
    if name == "zero":   # +0, not -0
        z = sel & (run["a0"] == 0)
        assert np.all(run["q0"][z].view(np.uint64) == 0) and np.all(run["s"][z].view(np.uint64) == 0)
        z = sel & (run["a1"] == 0)
        assert np.all(run["q1"][z].view(np.uint64) == 0)
