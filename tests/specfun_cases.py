"""Arguments, numpy branch models, references and wave layouts shared by tests/test_specfun_device.py (the host twin
hc_specfun_n) and tests/test_specfun_device_gpu.py (k_debug_specfun): every function of
nusiprop_amd/csrc/nusi_debug_specfun.hpp.

Per function, vectors(name) holds the mpmath vectors' arguments (tests/golden/specfun_kat*.json), every branch constant
its source compares against with both nextafter neighbours (and both signs where the domain allows), special values, and
seeded arguments over the domain, stratified by branch.  classify(name, ...) restates the source's branch conditions in
numpy; the tests assert that every class is populated before they compare anything.  The window forms (hypot<true>,
gsl_cli2_inl) only get arguments inside their caller contract; cdiv_v and the member chains vote their own window and
also get arguments outside it.

layouts(name) places one fixed probe set of 64 arguments per class into waves (element i is lane i % 64 of wave
i / 64): (a) one class alone, (b) every ordered pair 32 + 32, (c) one lane of A at lane 0, 31 or 63 in a wave of B,
(d) seeded shuffles of all classes, (e) partly active waves.  Nothing here is random between runs.
"""
import ctypes
import json
import os
import re

import numpy as np

from tests import atan2_cases as ac

HERE = os.path.dirname(os.path.abspath(__file__))
KAT = json.load(open(os.path.join(HERE, "golden", "specfun_kat.json")))
KAT.update(json.load(open(os.path.join(HERE, "golden", "specfun_kat_libm.json"))))   # log10, pow, hypot
HEADER = os.path.join(os.path.dirname(HERE), "nusiprop_amd", "csrc", "nusi_debug_specfun.hpp")
SENTINEL = np.uint64(0xffffffffffffffff)   # nusi_debug_specfun fills the outputs with 0xff bytes
D = ctypes.c_double
DP = ctypes.POINTER(D)
SEED = 20261021

# name -> DebugSpecfun number (nusi_debug_specfun.hpp; header_numbers() reads the header's own list)
FN = {n: i for i, n in enumerate(
    ["log", "log_i", "log1p", "exp", "atan", "atanh", "log10", "pow", "sqrt", "clog", "cdiv_real", "cdiv", "cdiv_v",
     "li2", "li3", "cli2", "gsl_li2", "clausen", "hypot", "hypot_w", "gsl_cli2", "gsl_cli2_inl", "member_dc",
     "member_dc_inl"])}
_HEADER_NAMES = {"Log": "log", "LogI": "log_i", "Log1p": "log1p", "Exp": "exp", "Atan": "atan", "Atanh": "atanh",
                 "Log10": "log10", "Pow": "pow", "Sqrt": "sqrt", "Clog": "clog", "CdivReal": "cdiv_real", "Cdiv": "cdiv",
                 "CdivV": "cdiv_v", "Li2": "li2", "Li3": "li3", "Cli2": "cli2", "GslLi2": "gsl_li2", "Clausen": "clausen",
                 "Hypot": "hypot", "HypotW": "hypot_w", "GslCli2": "gsl_cli2", "GslCli2Inl": "gsl_cli2_inl",
                 "MemberDc": "member_dc", "MemberDcInl": "member_dc_inl"}
# the functions with a wave vote or ballot in their call graph: these get the wave layouts
VOTED = ["gsl_cli2", "gsl_cli2_inl", "gsl_li2", "hypot", "hypot_w", "cdiv_v", "member_dc", "member_dc_inl", "li2", "cli2",
         "clog"]


def header_numbers():
    """{name: number} from the enum DebugSpecfun as the header lists it"""
    body = re.search(r"enum DebugSpecfun \{(.*?)\};", open(HEADER).read(), re.S).group(1)
    names = [m for m in re.findall(r"^\s*kDs(\w+)", body, re.M) if m != "Count"]
    return {_HEADER_NAMES[n]: i for i, n in enumerate(names)}


# ------------------------------------------------------------------------------------------------ helpers --
def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """64-bit patterns equal (the sign of zero included); NaN equals NaN"""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def hi(x):
    return ac.hi(x).astype(np.int64)


def from_hi(h):
    return float(ac.from_hi(h))


def around(vals, signs=False, k=1):
    """every value with its k nextafter neighbours on both sides (and the negatives)"""
    out = []
    for v in vals:
        lo = up = float(v)
        out.append(float(v))
        for _ in range(k):
            lo, up = float(np.nextafter(lo, -np.inf)), float(np.nextafter(up, np.inf))
            out += [lo, up]
    out = np.array(out)
    return np.concatenate([out, -out]) if signs else out


SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.0 ** -1040, 2.0 ** -1022,
                    float(np.nextafter(2.0 ** -1022, 0)), 1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0])


def logu(rng, lo, hi_, n):
    """n values log-uniform in [2^lo, 2^hi_)"""
    return np.exp2(rng.uniform(lo, hi_, n))


def sgn(rng, n):
    return rng.choice([-1.0, 1.0], n)


def _rng(name):
    return np.random.default_rng(SEED + FN[name])


def _cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts])


def _grid2(u, v):
    a, b = np.meshgrid(np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64), indexing="ij")
    return a.ravel(), b.ravel()


# ------------------------------------------------------------------------------- Smith's complex division --
def smith(a, c, d, ai=None):
    """(a + ai i) / (c + d i) as oracle/ora_cplx.h zdiv and nusi_math.hpp operator/ form it, elementwise (ai = None: a
    real numerator promoted, imaginary part +0)"""
    with np.errstate(all="ignore"):
        first = np.abs(c) < np.abs(d)
        ai = np.zeros_like(a) if ai is None else ai
        r1 = c / d
        den1 = (c * r1) + d
        re1, im1 = ((a * r1) + ai) / den1, ((ai * r1) - a) / den1
        r2 = d / c
        den2 = (d * r2) + c
        re2, im2 = ((ai * r2) + a) / den2, (ai - (a * r2)) / den2
    return np.where(first, re1, re2), np.where(first, im1, im2)


def member_win(x):
    """alpha_member_win (nusi_physics.hpp): |x| in [2^-50, 2^50)"""
    m = np.abs(x)
    return (m >= 2.0 ** -50) & (m < 2.0 ** 50)


# ---------------------------------------------------------------------------------------------- vectors --
# nusi_libm.hpp log_kernel: z in [0x1.6p-1, 0x1.6p+0) in 2^7 subintervals
_LOG_EDGES = np.array([0x3fe6000000000000 + (j << 45) for j in range(0, 129, 8)], np.uint64).view(np.float64)


def _v_log(name):
    rng = _rng(name)
    x = _cat([v for v, _ in KAT["log"]], SPECIAL, around([1.0, 0.6875, 1.375, 2.0, 0.5, 2.0 ** -1022, 2.0 ** 1023], k=2),
             around(_LOG_EDGES), around(_LOG_EDGES * 2.0 ** 300), 10.0 ** rng.uniform(-307, 308, 1500),
             rng.uniform(0.5, 2.0, 1000), 1.0 + rng.uniform(-1e-6, 1e-6, 500), rng.uniform(0, 1, 200) * 2.0 ** -1040,
             -logu(rng, -100, 100, 20))
    if name == "log10":   # e_log10.c: exact powers of ten, and k < 0 against k >= 0 (i)
        x = _cat(x, [v for v, _ in KAT.get("log10", [])], 10.0 ** np.arange(-300, 301, 25), around([1.0, 10.0, 0.1]))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_log(name, a, b, c):
    h = hi(a)
    cls = np.where(np.isnan(a) | (a == np.inf), "nonfinite", np.where(a == 0, "zero", np.where(
        a < 0, "negative", np.where(h < 0x00100000, "subnormal", "normal"))))
    if name == "log10":
        cls = np.where((cls == "normal") & (a < 1.0), "normal_k_negative", cls)
    return cls


def _v_log1p(name):
    rng = _rng(name)
    x = _cat([v for v, _ in KAT["log1p"]], SPECIAL, around([-1.0, 1.0, 0.0, -0.5, 0.375, -0.3125], k=2),
             around(_LOG_EDGES - 1.0), sgn(rng, 1500) * 10.0 ** rng.uniform(-20, 3, 1500), rng.uniform(-1, 1, 1000),
             rng.uniform(-1e-6, 1e-6, 300), 10.0 ** rng.uniform(3, 308, 300), sgn(rng, 100) * rng.uniform(0, 1, 100) * 2.0 ** -1040)
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_log1p(name, a, b, c):
    return np.where(~(a > -1.0) | (a == np.inf), "special", np.where(a >= 1.0, "ge1", "lt1"))


# e_exp.c's thresholds (nusi_libm.hpp exp_i)
_EXP_O, _EXP_U, _INVLN2 = 7.09782712893383973096e+02, -7.45133219101941108420e+02, 1.44269504088896338700e+00


def _v_exp(name):
    rng = _rng(name)
    ln2 = 0.6931471805599453
    edges = [_EXP_O, -_EXP_U, from_hi(0x40862E42), from_hi(0x3fd62e42), from_hi(0x3fd62e43), from_hi(0x3FF0A2B2),
             from_hi(0x3e300000), 0.5 * ln2, 1.5 * ln2, 2.0 ** -28] + [k * ln2 for k in (1019.5, 1020.5, 1021.5, 1022.5, 1074.5)]
    x = _cat([v for v, _ in KAT["exp"]], SPECIAL, around(edges, signs=True, k=2), rng.uniform(-745.2, 709.8, 2000),
             rng.uniform(-1.1, 1.1, 1000), sgn(rng, 500) * logu(rng, -60, 0, 500), rng.uniform(-745.2, -707.0, 300),
             sgn(rng, 100) * rng.uniform(709.0, 800.0, 100))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_exp(name, a, b, c):
    hx = hi(a) & 0x7fffffff
    with np.errstate(all="ignore"):
        k = np.trunc(_INVLN2 * a + np.where(a < 0, -0.5, 0.5))
    big = hx >= 0x40862E42
    out = np.where(hx >= 0x7ff00000, "nonfinite", np.where(a > _EXP_O, "overflow", np.where(a < _EXP_U, "underflow", "")))
    mid = np.where(hx > 0x3fd62e42, np.where(hx < 0x3FF0A2B2, "one_ln2", np.where(k < -1021, "subnormal_result", "k_ln2")),
                   np.where(hx < 0x3e300000, "tiny", "k_zero"))
    return np.where(big & (out != ""), out, mid)


# s_atan.c's ranges (nusi_libm.hpp atan_i): the high words of 7/16, 11/16, 19/16, 39/16, 2^-29, 2^66
_ATAN_HI = [0x3fdc0000, 0x3fe60000, 0x3ff30000, 0x40038000, 0x3e200000, 0x44100000]


def _v_atan(name):
    rng = _rng(name)
    x = _cat([v for v, _ in KAT["atan"]], SPECIAL, around([from_hi(h) for h in _ATAN_HI] + [7 / 16, 11 / 16, 19 / 16, 39 / 16],
                                                           signs=True, k=2),
             sgn(rng, 2000) * 10.0 ** rng.uniform(-10, 22, 2000), rng.uniform(-3, 3, 1500), sgn(rng, 200) * logu(rng, -40, -25, 200))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_atan(name, a, b, c):
    ix = hi(a) & 0x7fffffff
    r = np.where(ix < 0x3fdc0000, "range_m1", np.where(ix < 0x3fe60000, "range_0", np.where(
        ix < 0x3ff30000, "range_1", np.where(ix < 0x40038000, "range_2", "range_3"))))
    return np.where(ix >= 0x44100000, "huge_or_nan", np.where(ix < 0x3e200000, "tiny", r))


def _v_atanh(name):
    rng = _rng(name)
    x = _cat([v for v, _ in KAT["atanh"]], SPECIAL, around([2.0 ** -28, 0.5, 1.0, from_hi(0x3e300000)], signs=True, k=2),
             rng.uniform(-1, 1, 2000), sgn(rng, 500) * logu(rng, -40, 0, 500), sgn(rng, 300) * (1 - logu(rng, -52, -1, 300)),
             sgn(rng, 20) * rng.uniform(1, 5, 20))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_atanh(name, a, b, c):
    ix, lo = hi(a) & 0x7fffffff, ac.lo(a)
    return np.where((ix > 0x3ff00000) | ((ix == 0x3ff00000) & (lo != 0)), "outside", np.where(
        ix == 0x3ff00000, "one", np.where(ix < 0x3e300000, "tiny", np.where(ix < 0x3fe00000, "lt_half", "ge_half"))))


def _v_pow(name):
    rng = _rng(name)
    # the power-law source: (E / 1e14 (1 + z))^-si, si in [2, 3], lE in [4, 17]; and x > 0 at large
    xs = _cat([v[0] for v in KAT.get("pow", [])], 10.0 ** rng.uniform(4, 17, 1500) / 1e14 * (1 + rng.uniform(0, 5, 1500)),
              10.0 ** rng.uniform(4, 17, 500), 10.0 ** rng.uniform(-30, 30, 500), around([1.0], k=2), np.ones(10))
    ys = _cat([v[1] for v in KAT.get("pow", [])], -rng.uniform(2, 3, 1500), -rng.uniform(2, 3, 500), rng.uniform(-8, 8, 500),
              [2.0, -2.0, 0.0, 1.0, 0.5], [0.0, -0.0, 1.0, -1.0, 2.5, 1e300, -1e300, 5e-324, 3.0, -2.0])
    return xs, ys, np.zeros_like(xs)


def _c_pow(name, a, b, c):
    with np.errstate(all="ignore"):
        p = b * np.log(a)
    return np.where(p < 0, "product_negative", np.where(p > 0, "product_positive", "product_zero"))


def _v_sqrt(name):
    rng = _rng(name)
    x = _cat(SPECIAL, around([1.0, 2.0, 4.0, 2.0 ** -1022, 2.0 ** 1023], k=2), 10.0 ** rng.uniform(-307, 308, 2000),
             rng.uniform(0, 4, 1000), rng.uniform(0, 1, 300) * 2.0 ** -1040, -logu(rng, -10, 10, 10))
    with np.errstate(over="ignore"):
        rest = x[SPECIAL.size + 25:] * 10.0 ** rng.uniform(-3, 3, x.size - SPECIAL.size - 25)
    y = _cat(SPECIAL[::-1], around([0.0, 3.0, 4.0, 2.0 ** 511, 2.0 ** -537], k=2), rest)
    return x, y, np.zeros_like(x)


def _c_sqrt(name, a, b, c):
    return np.where(~np.isfinite(a) | (a < 0), "special", np.where(a == 0, "zero", np.where(a < 2.0 ** -1022, "subnormal", "normal")))


def _v_clog(name):
    rng = _rng(name)
    ys, xs = [np.array([p for p, _, _ in KAT["atan2"]])], [np.array([q for _, q, _ in KAT["atan2"]])]
    mag = 10.0 ** rng.uniform(-20, 20, size=(3000, 2))
    ys.append(mag[:, 0] * sgn(rng, 3000))
    xs.append(mag[:, 1] * sgn(rng, 3000))
    for r in range(-1, 4):   # every s_atan.c range of t = |y / x|, and its boundaries
        y, x = ac.pair(ac.t_in_range(r, 200, rng), rng)
        ys.append(y)
        xs.append(x)
    y, x = ac.pair(np.tile(ac.boundary_ts(), 8), rng)
    ys.append(y)
    xs.append(x)
    sp = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 5e-324, 1e308, 1e-308, 2.0 ** 61, 2.0 ** -61]
    y, x = _grid2(sp, sp)
    ys.append(y)
    xs.append(x)
    x, y = _cat(*xs), _cat(*ys)
    return x, y, np.zeros_like(x)   # clog(a + i b): a = x, b = y


def _c_clog(name, a, b, c):
    plain = ac.plain(b, a)
    return np.where(~plain, "atan2_full", np.where(ac.first_range(b, a), "first_range", "select"))


def _v_cdiv(name):
    rng = _rng(name)
    n = 2500
    a, c, d = (sgn(rng, n) * logu(rng, -50, 50, n) for _ in range(3))
    # Smith's |c| = |d| (the second case), and its neighbours
    e = sgn(rng, 60) * logu(rng, -40, 40, 60)
    eq_c = _cat(e, e, np.nextafter(e, 0), np.nextafter(e, np.inf * e))
    eq_d = _cat(e, -e, e, e)
    eq_a = sgn(rng, 240) * logu(rng, -40, 40, 240)
    # the member window's ends, and operands outside it (zeros, tiny, huge, non-finite)
    ends = around([2.0 ** -50, 2.0 ** 50], signs=True, k=1)
    out = np.array([0.0, -0.0, 2.0 ** -60, 1e-300, 5e-324, 2.0 ** 52, 1e20, 1e300, np.inf, -np.inf, np.nan])
    ea, ec = _grid2(ends, ends)
    ed = np.resize(sgn(rng, 7) * logu(rng, -49, 49, 7), ea.size)
    oa, oc = _grid2(out, _cat(out[:8], [1.0, -3.0]))
    od = np.resize(_cat(out, [0.5, -2.0, 7.0]), oa.size)
    A = _cat(a, eq_a, ea, ed, ec, oa, od, oc)
    Cc = _cat(c, eq_c, ec, ea, ed, oc, oa, od)
    Dd = _cat(d, eq_d, ed, ec, ea, od, oc, oa)
    return A, Cc, Dd


def _c_cdiv(name, a, b, c):
    with np.errstate(all="ignore"):
        case = np.where(np.abs(b) < np.abs(c), "case_1", np.where(np.abs(b) == np.abs(c), "case_2_equal", "case_2"))
    inw = member_win(a) & member_win(b) & member_win(c)
    if name == "cdiv_v":
        return np.where(inw, np.char.add("window_", case), "outside_window")
    return np.where(np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & ((b != 0) | (c != 0)), case, "degenerate")


def _v_li2(name):
    rng = _rng(name)
    x = _cat([v for v, _ in KAT["li2_real"]], around([1.0, 0.5, 0.0, 2.0], signs=True, k=2), [0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e300, 1e300],
             sgn(rng, 1500) * 10.0 ** rng.uniform(-8, 8, 1500), rng.uniform(-1.5, 2.5, 1500), rng.uniform(0.5, 1.0, 300),
             sgn(rng, 300) * logu(rng, -200, -20, 300))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_li2(name, a, b, c):
    with np.errstate(all="ignore"):
        u = np.where(np.abs(a) > 1.0, 1.0 / a, a)
    inv = np.where(a > 1.0, "gt1_", np.where(a < -1.0, "lt_m1_", ""))
    return np.char.add(inv, np.where(u == 1.0, "one", np.where(u > 0.5, "reflect", np.where(u == 0.0, "zero", "series"))))


def _v_li3(name):
    rng = _rng(name)
    x = _cat([v for v, _ in KAT["li3"]], [-1.0, float(np.nextafter(-1.0, 0)), 0.5, float(np.nextafter(0.5, 0)), 0.0, -0.0, 5e-324, -5e-324],
             rng.uniform(-1, 0.5, 2000), -logu(rng, -100, 0, 500), logu(rng, -100, -1, 300))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_li3(name, a, b, c):
    return np.where(a == 0, "zero", np.where(a < 0, "negative", "positive"))


_AXIS_RATIO = 2.5e-3   # nusi_math.hpp kLi2AxisRatio


def _polar(rng, r, lo=-np.pi, hi_=np.pi):
    t = rng.uniform(lo, hi_, np.size(r))
    return r * np.cos(t), r * np.sin(t)


def _v_cli2(name):
    rng = _rng(name)
    kx, ky = (np.array([v[i] for v in KAT["li2_complex"] + KAT["li2_complex_axis"] + KAT["li2_complex_unit"]]) for i in (0, 1))
    x1, y1 = _polar(rng, _cat(rng.uniform(0.0, 3.0, 1500), 1 + rng.uniform(-0.05, 0.05, 500), 10.0 ** rng.uniform(-20, 3, 1000)))
    xr = _cat(around([1.0, 0.5, 0.0, 2.0, -1.0], k=1), rng.uniform(-3, 3, 300))   # the real axis (y == 0)
    # the Taylor path's edge |y| = ratio min(|x|, |1 - x|), both sides; |z|^2 = 1 and Re z = 1/2 with neighbours
    xa = _cat(rng.uniform(-3, 3, 300), 1 + sgn(rng, 100) * 10.0 ** rng.uniform(-6, 0, 100))
    ya = sgn(rng, 400) * _AXIS_RATIO * np.minimum(np.abs(xa), np.abs(1 - xa)) * np.resize([1.0, 1 - 1e-15, 1 + 1e-15, 0.5, 2.0], 400)
    xu = _cat(around([0.6, -0.6, 0.8, 0.28, -0.96], k=2))
    yu = np.sqrt(1 - np.round(xu, 2) ** 2) * np.resize([1.0, -1.0], xu.size)
    xh = around([0.5], k=2)
    xh, yh = _grid2(xh, [0.3, -0.7, 1e-2, 3.0])
    x = _cat(kx, x1, xr, xa, xu, xh)
    y = _cat(ky, y1, np.zeros_like(xr), ya, yu, yh)
    return x, y, np.zeros_like(x)


def _c_cli2(name, a, b, c):
    x, y = a, b
    with np.errstate(all="ignore"):
        axis = np.abs(y) <= _AXIS_RATIO * np.minimum(np.abs(x), np.abs(1.0 - x))
        n2 = x * x + y * y
        zr = np.where(n2 > 1.0, x * (1.0 / n2), x)
    inv = np.where(n2 > 1.0, np.where(x > 0, "inverted_xpos_", "inverted_xneg_"), "")
    return np.where(y == 0, "real_axis", np.where(axis, "taylor_axis", np.char.add(inv, np.where(zr > 0.5, "reflect", "series"))))


def _v_gsl_li2(name):
    rng = _rng(name)
    # dilog_xge0's branch points, the series argument 0.01 of each branch that forms one (x = 0.99: 1 - x; 1 / 0.99: 1 -
    # 1 / x; 100: 1 / x), 2^-100 (1 / x below it: x above 2^100), 2^-400 (series_1's argument; for x < 0 also x^2)
    edges = [0.25, 0.5, 1.0, 1.01, 2.0, 0.99, 1 / 0.99, 100.0, 0.01, 2.0 ** 100, 2.0 ** -400, 2.0 ** -200, 2.0 ** -100]
    x = _cat([v for v, _ in KAT["li2_real"]], around(edges, signs=True, k=3), SPECIAL, rng.uniform(-40, 40, 1000), rng.uniform(-1.5, 2.5, 1500),
             10.0 ** rng.uniform(-20, 0, 600), -(10.0 ** rng.uniform(-20, 3, 400)), logu(rng, -600, -380, 200), -logu(rng, -320, -180, 200),
             logu(rng, 90, 400, 200), rng.uniform(1.0, 1.01, 200), rng.uniform(0.98, 1.0, 100), 1 + logu(rng, -52, -7, 100))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_gsl_xge0(x):
    return np.where((x > 1.0) & (x <= 1.01), "near_one", np.where(x == 1.0, "one", np.where(
        ~(x > 0.25), np.where(x > 0.0, np.where(x < 2.0 ** -400, "series_1_exact", "series_1"), "zero_or_nan"),
        np.where(x > 2.0, np.where(x > 2.0 ** 100, "gt2_exact", "gt2"), np.where(x > 1.01, "le2", np.where(x > 0.5, "lt1", "le_half"))))))


def _c_gsl_li2(name, a, b, c):
    return np.where(a < 0, "negative", _c_gsl_xge0(a))


_X_CUT = 3.14159265358979323846 * 1.4901161193847656e-08   # clausen: kPiD kSqrtEps


def _angle_restrict_pos(theta):
    """nusi_gsl.hpp angle_restrict_pos, the same operations"""
    P1, P2, P3 = 4 * 7.85398125648498535156e-01, 4 * 3.77489470793079817668e-08, 4 * 2.69515142907905952645e-15
    TwoPi = 2 * (P1 + P2 + P3)
    with np.errstate(all="ignore"):
        y = 2 * np.floor(theta / TwoPi)
        r = ((theta - y * P1) - y * P2) - y * P3
        return np.where(r > TwoPi, ((r - 2 * P1) - 2 * P2) - 2 * P3, np.where(r < 0, ((r + 2 * P1) + 2 * P2) + 2 * P3, r))


def _v_clausen(name):
    rng = _rng(name)
    pi = np.pi
    x = _cat([v for v, _ in KAT["clausen"]], [0.0, -0.0, 5e-324, 1e-300], around([_X_CUT, pi, 2 * pi, 4 * pi, 6 * pi, 20 * pi, 3 * pi], signs=True, k=3),
             rng.uniform(-7, 7, 1500), rng.uniform(-100, 100, 1000), sgn(rng, 500) * logu(rng, -60, 0, 500),
             2 * pi * rng.integers(1, 50, 200) + sgn(rng, 200) * logu(rng, -40, -20, 200), sgn(rng, 100) * 10.0 ** rng.uniform(2, 8, 100))
    return x, np.zeros_like(x), np.zeros_like(x)


def _c_clausen(name, a, b, c):
    x = _angle_restrict_pos(np.abs(a))
    refl = x > np.pi
    x = np.where(refl, (6.28125 - x) + 0.19353071795864769253e-02, x)
    return np.char.add(np.where(refl, "upper_", "lower_"), np.where(x == 0, "zero", np.where(x < _X_CUT, "small", "chebyshev")))


def _v_hypot(name):
    rng = _rng(name)
    n = 2500
    a, b = (rng.normal(size=n) * 10.0 ** rng.uniform(-200, 200, n) for _ in range(2))
    b[:1500] = a[:1500] * 10.0 ** rng.uniform(-3, 3, 1500)
    e = around([2.0 ** 500, 2.0 ** -500], signs=True, k=1)
    ea, eb = _grid2(e, _cat(e, [1.0, 3.0, 2.0 ** -600, 2.0 ** 600]))
    sa, sb = _grid2(SPECIAL, _cat(SPECIAL, [3.0, 1e200]))
    za = sgn(rng, 100) * logu(rng, -1070, 1020, 100)   # b == 0
    A = _cat([v[0] for v in KAT.get("hypot", [])], a, ea, eb, sa, sb, za, np.zeros(100), [3.0, 5.0, 1e-320, 1e300, 1e-300])
    B = _cat([v[1] for v in KAT.get("hypot", [])], b, eb, ea, sb, sa, np.zeros(100), za, [4.0, 12.0, 1e-320, 1e300, 1e-300])
    return A, B, np.zeros_like(A)


def _c_hypot(name, a, b, c):
    x, y = np.abs(a), np.abs(b)
    with np.errstate(all="ignore"):
        big, small = np.fmax(x, y), np.fmin(x, y)
        swap_nan = np.isnan(x) | np.isnan(y)
    return np.where(swap_nan | np.isinf(big), "nonfinite", np.where(small == 0, "b_zero", np.where(
        (small >= 2.0 ** -500) & (big <= 2.0 ** 500), "common", np.where(big > 2.0 ** 500, "scaled_down", "scaled_up"))))


def _v_hypot_w(name):
    """inside hypot<true>'s caller bounds: 2^-500 <= |x|, |y| <= 2^100, or the smaller one 0"""
    rng = _rng(name)
    n = 2000
    a = sgn(rng, n) * logu(rng, -500, 100, n)
    b = sgn(rng, n) * np.clip(np.abs(a) * logu(rng, -60, 60, n), 2.0 ** -500, 2.0 ** 100)
    t = sgn(rng, 400) * logu(rng, -500, -451, 400)   # both so small that the residual is below 2^-900 (its vote fails)
    tb = sgn(rng, 400) * np.clip(np.abs(t) * rng.uniform(0.01, 1, 400), 2.0 ** -500, None)
    e = np.array([2.0 ** -500, float(np.nextafter(2.0 ** -500, 1)), 2.0 ** 100, float(np.nextafter(2.0 ** 100, 0)), 1.0, 2.0 ** -450, 2.0 ** -449])
    ea, eb = _grid2(_cat(e, -e), e)
    za = sgn(rng, 100) * logu(rng, -500, 100, 100)
    A = _cat(a, t, ea, za, np.zeros(100), [2.0 ** -500, 2.0 ** 100, 3.0, 5.0])
    B = _cat(b, tb, eb, np.zeros(100), za, [0.0, 0.0, 4.0, 12.0])
    ok = lambda v: ((np.abs(v) >= 2.0 ** -500) & (np.abs(v) <= 2.0 ** 100))
    assert ((ok(A) & ok(B)) | (ok(A) & (B == 0)) | (ok(B) & (A == 0))).all()
    return A, B, np.zeros_like(A)


def _c_hypot_w(name, a, b, c):
    big, small = np.maximum(np.abs(a), np.abs(b)), np.minimum(np.abs(a), np.abs(b))
    # |residual| <= 2^-51 h^2: below 2^-900, or 0, for h <= 2^-449 -- the lane's vote for the short division fails
    return np.where(small == 0, "b_zero", np.where(big <= 2.0 ** -450, "residual_below_vote", "generic"))


def _gsl_cli2_edges():
    """GSL's branch points of the complex dilogarithm, with neighbours: both edges of |r^2 - 1| < eps, r = 0.25, r = 0.98,
    x = 0.732, r^2 = 1 (the modulus of (x, tiny) is |x| exactly)"""
    xs, ys = [], []
    y0 = 1e-3
    for k in range(-6, 7):   # r^2 = 1 + k eps / 2 to a rounding
        xs.append(np.sqrt(1 - y0 * y0 + k * 2.0 ** -53))
        ys.append(y0)
    for x0 in (0.25, 0.98, 1.0, 1 / 0.98, 4.0, 0.732):
        for v in around([x0], k=2):
            for y in (1e-10, -1e-10, 2.0 ** -60):
                xs += [-v, v]
                ys += [y, y]
    for v in around([0.732], k=2):
        for y in (0.1, -0.3, 0.6, 1e-5):
            xs.append(v)
            ys.append(y)
    xs += [0.6, -0.6, 0.8, -0.8, 0.28, 0.96]
    ys += [0.8, 0.8, -0.6, 0.6, 0.96, -0.28]
    return np.array(xs), np.array(ys)


def _gsl_cli2_classes(rng, n):
    """n seeded arguments in each of the complex dilogarithm's classes, by construction (classify() must agree)"""
    th = lambda m: rng.uniform(0.8, 2 * np.pi - 0.8, m)   # Re z <= |z| cos 0.8 < 0.732
    out = {}
    t = th(n)
    r = rng.uniform(0.01, 0.24, n)
    out["series_1"] = (r * np.cos(t), r * np.sin(t))
    r = 1e-15 * rng.uniform(0.5, 2, n)
    out["series_1_fast"] = _polar(rng, r)
    r, t = rng.uniform(0.3, 0.9, n), th(n)
    out["series_2"] = (r * np.cos(t), r * np.sin(t))
    r, t = rng.uniform(0.975, 0.9799, n), th(n)
    out["series_2_slow"] = (r * np.cos(t), r * np.sin(t))
    r, t = rng.uniform(0.981, 0.999, n), th(n)
    out["series_3"] = (r * np.cos(t), r * np.sin(t))
    out["reflected"] = (rng.uniform(0.74, 0.95, n), sgn(rng, n) * 10.0 ** rng.uniform(-6, np.log10(0.25), n))
    out["inverted"] = _polar(rng, 10.0 ** rng.uniform(0.05, 6, n))
    t = rng.uniform(-np.pi, np.pi, 40 * n)
    x, y = np.cos(t), np.sin(t)
    on = np.abs((x * x + y * y) - 1.0) < 2.2204460492503131e-16
    out["unit_circle"] = (x[on][:n], y[on][:n])
    return out


def _v_gsl_cli2(name):
    rng = _rng(name)
    inl = name == "gsl_cli2_inl"
    kx, ky = (np.array([v[i] for v in KAT["li2_complex"] + KAT["li2_complex_axis"] + KAT["li2_complex_unit"]]) for i in (0, 1))
    ex, ey = _gsl_cli2_edges()
    xs, ys = [kx, ex], [ky, ey]
    for x, y in _gsl_cli2_classes(rng, 250).values():
        xs.append(x)
        ys.append(y)
    x1, y1 = _polar(rng, _cat(rng.uniform(0.0, 3.0, 800), 1 + rng.uniform(-0.05, 0.05, 400), 10.0 ** rng.uniform(-20, 3, 600)))
    xs.append(x1)
    ys.append(y1)
    if inl:   # the member window's corners and edges: |x|, |y| in [2^-201, 2^100]
        w = np.array([2.0 ** -201, float(np.nextafter(2.0 ** -201, 1)), 2.0 ** 100, float(np.nextafter(2.0 ** 100, 0)), 2.0 ** -100, 1.0, 0.5])
        wx, wy = _grid2(_cat(w, -w), _cat(w, -w))
        x2 = sgn(rng, 500) * logu(rng, -201, 100, 500)
        y2 = sgn(rng, 500) * logu(rng, -201, 100, 500)
        xs += [wx, x2]
        ys += [wy, y2]
    else:   # the real axis, r < 2^-400 (the exact-division instance; hypot's scaled branch below 2^-500), r = 2^-400
        xr = _cat(around([0.25, 0.5, 1.0, 1.01, 2.0, 0.0], signs=True, k=1), rng.uniform(-3, 3, 200), 10.0 ** rng.uniform(-5, 5, 100))
        tx, ty = _polar(rng, logu(rng, -900, -400, 300))
        hx = around([2.0 ** -400], signs=True, k=2)
        xs += [xr, tx, hx, hx * 2.0 ** -60]
        ys += [np.zeros_like(xr), ty, hx * 2.0 ** -60, hx]
    x, y = _cat(*xs), _cat(*ys)
    if inl:
        ok = lambda v: (np.abs(v) >= 2.0 ** -201) & (np.abs(v) <= 2.0 ** 100)
        keep = ok(x) & ok(y)
        x, y = x[keep], y[keep]
    return x, y, np.zeros_like(x)


def _c_gsl_cli2(name, a, b, c):
    """gsl_cli2_t / unitdisk / fundamental_body / cseries (nusi_gsl.hpp), the conditions in their order.  The moduli are
    numpy's hypot: within an ulp of the device's, which only matters to an argument placed on an edge"""
    x, y = a, b
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
        unit = np.abs(r2 - 1.0) < 2.2204460492503131e-16
        inv = ~(r2 < 1.0)
        ux, uy = np.where(inv, x / r2, x), np.where(inv, -y / r2, y)
        refl = ux > 0.732
        fx, fy = np.where(refl, 1.0 - ux, ux), np.where(refl, -uy, uy)
        rf = np.hypot(fx, fy)
    ser = np.where(rf > 0.98, "series_3", np.where(rf > 0.25, np.where(rf > 0.97, "series_2_slow", "series_2"), np.where(
        rf < 2.0 ** -400, "series_exact", np.where(rf < 1e-12, "series_1_fast", "series_1"))))
    return np.where(y == 0, "real_axis", np.where(unit, "unit_circle", np.where(inv, "inverted", np.where(refl, "reflected", ser))))


def _v_member(name):
    """(S, t, gr) of alpha_member_ref_dc(_inl): a = 1 + S + t, c = 2 + t, d = -gr"""
    rng = _rng(name)
    n = 1500
    S, t, gr = 10.0 ** rng.uniform(-3, 3, n), -(10.0 ** rng.uniform(-3, 3, n)), 10.0 ** rng.uniform(-9, -1, n)
    # Smith's first case inside the window: |2 + t| < gr
    g1 = 10.0 ** rng.uniform(-6, -1, 300)
    t1 = -2.0 + sgn(rng, 300) * g1 * rng.uniform(0.01, 0.9, 300)
    S1 = 10.0 ** rng.uniform(-2, 2, 300)
    # |z| on both sides of 1: a ~ |c|
    t2 = -(10.0 ** rng.uniform(-2, 0.2, 300))
    S2 = (2 + t2) * rng.uniform(0.5, 2.0, 300) - 1 - t2
    g2 = 10.0 ** rng.uniform(-8, -2, 300)
    # outside the window: a (0, a rounding error of 0, above 2^50), c (0, below 2^-50), gr (below 2^-50), singly and together
    xs = np.array([0.5, 1.0, 3.0, 1e-3, 2.0 ** 52, 1e20])
    ts = np.array([-2.0, -1.5, -2.0 - 2.0 ** -51, -2.0 + 2.0 ** -52, -1e-3, -1e18, -3.0])
    gs = np.array([2.0 ** -51, 2.0 ** -60, 1e-300, 2e-8, 0.02])
    Sx, tx, gx = (v.ravel() for v in np.meshgrid(xs, ts, gs, indexing="ij"))
    # the window's ends on each operand
    ends = around([2.0 ** -50, 2.0 ** 50], k=1)
    Se, ge = _grid2(ends, _cat(ends[:3], [1e-4]))
    te = np.resize([-0.5, -1.0, -1.75], Se.size)
    ce = around([2.0 ** -50], signs=True, k=1) - 2.0   # c = 2 + t at the lower end (t's spacing is 2^-52: c is 2^-50 +- 2^-52)
    return (_cat(S, S1, S2, Sx, -1.0 - ts, Se - 1 - te, np.full(ce.size, 0.75)), _cat(t, t1, t2, tx, ts, te, ce),
            _cat(gr, g1, g2, gx, np.full(ts.size, 2e-8), ge, np.full(ce.size, 1e-3)))


def _c_member(name, a, b, c):
    S, t, gr = a, b, c
    A, Cc = 1 + S + t, 2 + t
    zr, zi = smith(A, Cc, -gr)
    with np.errstate(all="ignore"):
        inv = ~((zr * zr + zi * zi) < 1.0)
        first = np.abs(Cc) < np.abs(gr)
    inside = np.where(first, "window_case_1", np.where(inv, "window_case_2_inverted", "window_case_2"))
    return np.where(~member_win(A), "outside_a", np.where(~member_win(Cc), "outside_c", np.where(~member_win(gr), "outside_gr", inside)))


_TABLE = {
    "log": (_v_log, _c_log), "log_i": (_v_log, _c_log), "log10": (_v_log, _c_log), "log1p": (_v_log1p, _c_log1p),
    "exp": (_v_exp, _c_exp), "atan": (_v_atan, _c_atan), "atanh": (_v_atanh, _c_atanh), "pow": (_v_pow, _c_pow),
    "sqrt": (_v_sqrt, _c_sqrt), "clog": (_v_clog, _c_clog), "cdiv_real": (_v_cdiv, _c_cdiv), "cdiv": (_v_cdiv, _c_cdiv),
    "cdiv_v": (_v_cdiv, _c_cdiv), "li2": (_v_li2, _c_li2), "li3": (_v_li3, _c_li3), "cli2": (_v_cli2, _c_cli2),
    "gsl_li2": (_v_gsl_li2, _c_gsl_li2), "clausen": (_v_clausen, _c_clausen), "hypot": (_v_hypot, _c_hypot),
    "hypot_w": (_v_hypot_w, _c_hypot_w), "gsl_cli2": (_v_gsl_cli2, _c_gsl_cli2), "gsl_cli2_inl": (_v_gsl_cli2, _c_gsl_cli2),
    "member_dc": (_v_member, _c_member), "member_dc_inl": (_v_member, _c_member),
}
# every class classify() can return for the function: all of them must be populated
CLASSES = {
    "log": ["nonfinite", "zero", "negative", "subnormal", "normal"],
    "log_i": ["nonfinite", "zero", "negative", "subnormal", "normal"],
    "log10": ["nonfinite", "zero", "negative", "subnormal", "normal", "normal_k_negative"],
    "log1p": ["special", "ge1", "lt1"],
    "exp": ["nonfinite", "overflow", "underflow", "one_ln2", "k_ln2", "subnormal_result", "tiny", "k_zero"],
    "atan": ["huge_or_nan", "tiny", "range_m1", "range_0", "range_1", "range_2", "range_3"],
    "atanh": ["outside", "one", "tiny", "lt_half", "ge_half"],
    "pow": ["product_negative", "product_positive", "product_zero"],
    "sqrt": ["special", "zero", "subnormal", "normal"],
    "clog": ["atan2_full", "first_range", "select"],
    "cdiv_real": ["case_1", "case_2", "case_2_equal", "degenerate"],
    "cdiv": ["case_1", "case_2", "case_2_equal", "degenerate"],
    "cdiv_v": ["window_case_1", "window_case_2", "window_case_2_equal", "outside_window"],
    "li2": ["gt1_reflect", "gt1_series", "lt_m1_series", "one", "reflect", "zero", "series"],
    "li3": ["zero", "negative", "positive"],
    "cli2": ["real_axis", "taylor_axis", "inverted_xpos_reflect", "inverted_xpos_series", "inverted_xneg_series", "reflect", "series"],
    "gsl_li2": ["negative", "near_one", "one", "series_1_exact", "series_1", "zero_or_nan", "gt2_exact", "gt2", "le2", "lt1", "le_half"],
    "clausen": ["lower_zero", "lower_small", "lower_chebyshev", "upper_small", "upper_chebyshev"],
    "hypot": ["nonfinite", "b_zero", "common", "scaled_down", "scaled_up"],
    "hypot_w": ["b_zero", "residual_below_vote", "generic"],
    "gsl_cli2": ["real_axis", "unit_circle", "inverted", "reflected", "series_3", "series_2_slow", "series_2", "series_exact",
                 "series_1_fast", "series_1"],
    "gsl_cli2_inl": ["unit_circle", "inverted", "reflected", "series_3", "series_2_slow", "series_2", "series_1_fast", "series_1"],
    "member_dc": ["outside_a", "outside_c", "outside_gr", "window_case_1", "window_case_2_inverted", "window_case_2"],
    "member_dc_inl": ["outside_a", "outside_c", "outside_gr", "window_case_1", "window_case_2_inverted", "window_case_2"],
}

_cache = {}


def vectors(name):
    """(a, b, c): the function's arguments, float64 arrays of one length (unused arguments 0)"""
    if name not in _cache:
        a, b, c = (np.ascontiguousarray(v, dtype=np.float64) for v in _TABLE[name][0](name))
        assert a.size == b.size == c.size and a.size <= 65536
        for v in (a, b, c):
            v.setflags(write=False)
        _cache[name] = (a, b, c)
    return _cache[name]


def classify(name, a, b, c):
    """the branch each argument takes, from the source's conditions: an array of class names"""
    return np.asarray(_TABLE[name][1](name, a, b, c)).astype(str)


def class_counts(name):
    cls = classify(name, *vectors(name))
    return {k: int((cls == k).sum()) for k in CLASSES[name]}, sorted(set(cls) - set(CLASSES[name]))


# -------------------------------------------------------------------------------------------- references --
def bind_oracle(L):
    for f in ("ora_log", "ora_log1p", "ora_exp", "ora_atan", "ora_atanh", "ora_log10", "ora_li2", "ora_li3", "ora_gsl_dilog",
              "ora_gsl_clausen"):
        getattr(L, f).restype = D
        getattr(L, f).argtypes = [D]
    for f in ("ora_atan2", "ora_pow", "ora_hypot"):
        getattr(L, f).restype = D
        getattr(L, f).argtypes = [D, D]
    for f in ("ora_complex_dilog_xy", "ora_gsl_complex_dilog_xy"):
        getattr(L, f).restype = None
        getattr(L, f).argtypes = [D, D, DP, DP]
    return L


def _map1(f, a):
    return np.array([f(float(v)) for v in a], dtype=np.float64)


def _map2(f, a, b):
    return np.array([f(float(u), float(v)) for u, v in zip(a, b)], dtype=np.float64)


def _mapc(f, x, y):
    re, im = D(), D()
    out = np.empty((2, x.size))
    for i in range(x.size):
        f(float(x[i]), float(y[i]), ctypes.byref(re), ctypes.byref(im))
        out[0, i], out[1, i] = re.value, im.value
    return out[0], out[1]


def reference(name, L, a, b, c):
    """(o0, o1) of debug_specfun<name> by the oracle (L: its library, bind_oracle'd) -- and for the operations the oracle
    takes from the C compiler (sqrt, Smith's division: oracle/ora_cplx.h zdiv) by the same IEEE operations in numpy"""
    z = np.zeros_like(a)
    one = {"log": "ora_log", "log_i": "ora_log", "log1p": "ora_log1p", "exp": "ora_exp", "atan": "ora_atan", "atanh": "ora_atanh",
           "log10": "ora_log10", "li2": "ora_li2", "li3": "ora_li3", "gsl_li2": "ora_gsl_dilog", "clausen": "ora_gsl_clausen"}
    with np.errstate(all="ignore"):
        if name in one:
            return _map1(getattr(L, one[name]), a), z
        if name == "pow":
            return _map2(L.ora_pow, a, b), z
        if name in ("hypot", "hypot_w"):
            return _map2(L.ora_hypot, a, b), z
        if name == "sqrt":
            return np.sqrt(a), np.sqrt(a * a + b * b)
        if name == "clog":
            return 0.5 * _map1(L.ora_log, a * a + b * b), _map2(L.ora_atan2, b, a)
        if name in ("cdiv_real", "cdiv_v"):
            return smith(a, b, c)
        if name == "cdiv":
            return smith(a, b, c, ai=-c)
        if name == "cli2":
            return _mapc(L.ora_complex_dilog_xy, a, b)
        if name in ("gsl_cli2", "gsl_cli2_inl"):
            return _mapc(L.ora_gsl_complex_dilog_xy, a, b)
        if name in ("member_dc", "member_dc_inl"):
            zr, zi = smith(1 + a + b, 2 + b, -c)
            return _mapc(L.ora_gsl_complex_dilog_xy, zr, zi)
    raise KeyError(name)


# ----------------------------------------------------------------------------------------------- layouts --
# the classes whose probe sets are mixed in waves (the voted functions'), as classify() names them
LAYOUT_CLASSES = {k: CLASSES[k] for k in VOTED}


def probes(name):
    """{class: 64 indices into vectors(name)}, fixed: seeded picks among the class's arguments (repeated if it has fewer)"""
    rng = np.random.default_rng(SEED + 1000 + FN[name])
    cls = classify(name, *vectors(name))
    out = {}
    for k in LAYOUT_CLASSES[name]:
        idx = np.flatnonzero(cls == k)
        assert idx.size > 0, (name, k)
        out[k] = rng.choice(idx, 64, replace=idx.size < 64)
    return out


PARTIAL = {"lane_0": np.arange(64) == 0, "lane_63": np.arange(64) == 63, "even_lanes": np.arange(64) % 2 == 0,
           "odd_lanes": np.arange(64) % 2 == 1}


def layouts(name):
    """[(label, idx[64], active[64])]: one wave each, idx into vectors(name)"""
    rng = np.random.default_rng(SEED + 2000 + FN[name])
    P = probes(name)
    keys = list(P)
    full = np.ones(64, bool)
    out = [("a:%s" % k, P[k], full) for k in keys]
    for A in keys:
        for B in keys:
            if A == B:
                continue
            out.append(("b:%s|%s" % (A, B), np.concatenate([P[A][:32], P[B][32:]]), full))
            for lane in (0, 31, 63):
                w = P[B].copy()
                w[lane] = P[A][lane]
                out.append(("c:%s@%d in %s" % (A, lane, B), w, full))
    pool = np.concatenate([P[k] for k in keys])
    shuffles = []
    for s in range(2):
        perm = rng.permutation(pool)
        for j in range(0, perm.size, 64):
            shuffles.append(perm[j:j + 64])
            out.append(("d:shuffle %d.%d" % (s, j // 64), perm[j:j + 64], full))
    for pname, mask in PARTIAL.items():
        for k in keys:
            out.append(("e:%s of %s" % (pname, k), P[k], mask))
        for j, w in enumerate(shuffles[:2]):
            out.append(("e:%s of shuffle %d" % (pname, j), w, mask))
    return out


def layout_arrays(name, tail=0):
    """the layouts as one launch: (idx, active, wave labels); tail: a last wave of that many elements (a shuffle's first)"""
    L = layouts(name)
    idx = np.concatenate([w for _, w, _ in L])
    act = np.concatenate([m for _, _, m in L])
    labels = [l for l, _, _ in L]
    if tail:
        w = next(w for l, w, _ in L if l.startswith("d:"))
        idx, act = np.concatenate([idx, w[:tail]]), np.concatenate([act, np.ones(tail, bool)])
        labels.append("e:last wave of %d" % tail)
    assert idx.size <= 65536
    return idx, act, labels
