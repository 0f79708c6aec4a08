"""The profiled statistic on the CPU: detector.profile_host (the yardstick of nusi_plan_response_profile and the user's
host path) and the ABI's new entry points.

profile_host's result is checked in exact arithmetic (fractions.Fraction on the doubles themselves): with
g(a) = S1 - S2(a), S1 = sum_c s_c, S2(a) = sum over active c of data_c s_c / (a s_c + B_c), g'(a) = sum data_c s_c^2 /
(a s_c + B_c)^2, a converged ahat > 0 satisfies

    |g(ahat)| <= K u (S1 + S2(ahat)),   K = 2 ceil(log2 C) + 18,  u = 2^-53

("The profiled statistic", derives K from the rounding count of S1, S2 and the step), i.e. ahat is
within K u (S1 + S2) / g' of the root in Newton's measure.  Signals come as R[t][1][c] = s_c on a two-bin source axis with
S = [., 1.0], so the accumulator is s_c itself (0.0 + s_c * 1.0) and the table axis numbers the cases.
"""
import ctypes
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from nusiprop_amd import detector
from nusiprop_amd.detector import FIT_BOUNDARY, FIT_FLAT, FIT_INFINITE, FIT_ITER_MAX, FIT_NOT_CONVERGED, FIT_STEPS_MASK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nusi.h")
NEW = ["nusi_plan_response_profile", "nusi_plan_response_profile_host"]
U = Fraction(1, 2 ** 53)
CS = (1, 2, 3, 5, 17, 64)
KINDS = ("zero_bg", "tiny_bg", "bg_dominated", "decades", "downward")
NCASE = 24


def bound_constant(C):
    """K of the module docstring."""
    return 2 * int(math.ceil(math.log2(C))) + 18 if C > 1 else 18


def make_cases(C, kind, asimov, seed, n=NCASE):
    """n seeded cases of one class: (s [n][C], B [n][C], data [n][C], a0 [n]).  Poisson data of the expectation
    a0 s + B, or (asimov) the non-integer expectation itself, rounded as the doubles round it."""
    rng = np.random.default_rng([seed, C, KINDS.index(kind), int(asimov)])
    if kind == "decades":
        s = 10.0 ** rng.uniform(-15, 15, (n, C))                 # 30 decades inside one case
    else:
        s = 10.0 ** rng.uniform(-1, 1, (n, C)) * 10.0 ** rng.uniform(-6, 6, (n, 1))
    a0 = 10.0 ** rng.uniform(0, 9, n) / s.max(axis=1)            # the largest bin expects up to 1e9 events
    if kind in ("zero_bg", "decades"):
        B = np.zeros((n, C))
    elif kind == "tiny_bg":
        B = 1e-300 * rng.uniform(0.5, 2.0, (n, C))
    elif kind == "bg_dominated":
        B = 1e6 * (a0[:, None] * s)
    else:                                                        # downward: the data fall short of the background
        B = rng.uniform(5.0, 50.0, (n, C))
        a0 = 0.05 * B.min(axis=1) / s.max(axis=1)
    mean = a0[:, None] * s + B
    if asimov:
        data = mean
    elif kind == "downward":
        data = rng.poisson(0.7 * B).astype(np.float64)
    else:
        data = rng.poisson(mean).astype(np.float64)
    return s, B, data, a0


def run_case(s, B, data, log=np.log):
    """profile_host of one case: s [C] through a two-bin source axis."""
    C = len(s)
    R = np.zeros((1, 2, C))
    R[0, 1] = s
    a, nll, mu, st = detector.profile_host(R, np.array([[7.0, 1.0]]), data, background=B, log=log)
    return float(a[0, 0]), float(nll[0, 0]), mu[0, 0], int(st[0, 0])


def exact_g(a, s, B, data):
    """(S1, S2, g') at a, exact."""
    a = Fraction(a)
    S1 = sum((Fraction(float(x)) for x in s), Fraction(0))
    S2 = gp = Fraction(0)
    for sc, bc, dc in zip(s, B, data):
        if dc > 0 and sc > 0:
            sc, bc, dc = Fraction(float(sc)), Fraction(float(bc)), Fraction(float(dc))
            den = a * sc + bc
            S2 += dc * sc / den
            gp += dc * sc * sc / (den * den)
    return S1, S2, gp


# --- the defined order: profile_host against a scalar loop on Python floats -----------------------------------------------
def _tree(x):
    P = 1
    while P < len(x):
        P *= 2
    v = list(x) + [0.0] * (P - len(x))
    while len(v) > 1:
        v = [v[i] + v[i + 1] for i in range(0, len(v), 2)]
    return v[0]


def scalar_profile(s, B, data):
    """include/nusi.h's iteration, one operation per line, on Python floats."""
    C = len(s)
    s, B, data = [float(x) for x in s], [float(x) for x in B], [float(x) for x in data]
    act = [data[c] > 0 and s[c] > 0 for c in range(C)]
    S1 = _tree(s)
    steps = flags = 0
    a = 0.0
    if S1 == 0 or not any(act):
        flags |= FIT_FLAT
    else:
        for c in range(C):
            if act[c]:
                x = data[c] / S1 - B[c] / s[c]
                a = x if x > a else a
        while True:
            r, h = [0.0] * C, [0.0] * C
            for c in range(C):
                if act[c]:
                    den = a * s[c]
                    den = den + B[c]
                    u = s[c] / den
                    r[c] = data[c] * u
                    h[c] = r[c] * u
            S2, S3 = _tree(r), _tree(h)
            steps += 1
            g = S1 - S2
            if g >= 0:
                if a == 0:
                    flags |= FIT_BOUNDARY
                break
            an = a + (S2 - S1) / S3
            if an <= a:
                break
            a = an
            if steps == FIT_ITER_MAX:
                flags |= FIT_NOT_CONVERGED
                break
    mu = []
    for c in range(C):
        m = a * s[c]
        mu.append(m + B[c])
    if any(data[c] > 0 and mu[c] == 0 for c in range(C)):
        flags |= FIT_INFINITE
    return a, mu, steps | flags


@pytest.mark.parametrize("C", CS)
def test_profile_host_is_the_scalar_loop(C):
    for kind in KINDS:
        s, B, data, _ = make_cases(C, kind, False, seed=1, n=6)
        if C > 2:
            s[0, 1] = 0.0                           # a bin without signal
            data[1, C - 1] = 0.0                    # a bin without data
        R = np.zeros((len(s), 2, C))
        R[:, 1] = s
        for t in range(len(s)):                     # (one background per call)
            a, nll, mu, st = detector.profile_host(R[t], np.array([3.0, 1.0]), data[t], background=B[t], log=math.log)
            wa, wmu, wst = scalar_profile(s[t], B[t], data[t])
            assert a.shape == () and mu.shape == (C,) and st.dtype == np.int32
            assert float(a) == wa and int(st) == wst and list(mu) == wmu, (kind, t)
            assert float(nll) == float(detector.poisson_host(mu, data[t], log=math.log))


def test_tree_is_the_sum_of_adjacent_pairs():
    x = np.random.default_rng(2).random((3, 4, 11))
    got = detector.tree(x)
    assert got.shape == (3, 4)
    for i in range(3):
        for j in range(4):
            assert got[i, j] == _tree([float(v) for v in x[i, j]])
    assert detector.tree(np.array([1.5])) == 1.5
    # not the serial sum: 1 + 2^-53 + 2^-53 + 0 is 1 serially and 1 + 2^-52 pairwise
    assert detector.tree(np.array([1.0, 0.0, 2.0 ** -53, 2.0 ** -53])) == 1.0 + 2.0 ** -52


# --- optimality in exact arithmetic -------------------------------------------------------------------------------------
# (the downward class is defined by its Poisson shortfall: it has no Asimov form)
@pytest.mark.parametrize("kind,asimov", [(k, a) for k in KINDS for a in (False, True) if not (a and k == "downward")])
@pytest.mark.parametrize("C", CS)
def test_ahat_is_optimal_in_exact_arithmetic(C, kind, asimov):
    s, B, data, a0 = make_cases(C, kind, asimov, seed=3)
    K = bound_constant(C)
    worst = worst_a0 = 0.0
    seen = {"interior": 0, "boundary": 0, "flat": 0}
    for t in range(len(s)):
        a, nll, mu, st = run_case(s[t], B[t], data[t])
        steps = st & FIT_STEPS_MASK
        assert not st & FIT_NOT_CONVERGED and steps <= FIT_ITER_MAX, (t, st)
        assert not st & FIT_INFINITE and math.isfinite(nll)
        act = (data[t] > 0) & (s[t] > 0)
        if st & FIT_FLAT:
            assert a == 0.0 and steps == 0 and (float(np.sum(s[t])) == 0.0 or not act.any())
            seen["flat"] += 1
            continue
        assert steps >= 1
        S1, S2, gp = exact_g(a, s[t], B[t], data[t])
        if st & FIT_BOUNDARY:
            assert a == 0.0 and S1 - S2 >= 0, (t, float(S1 - S2))
            seen["boundary"] += 1
            continue
        assert a > 0.0
        seen["interior"] += 1
        unit = U * (S1 + S2)
        ratio = abs(S1 - S2) / (K * unit)
        worst = max(worst, float(ratio))
        assert ratio <= 1, (C, kind, t, float(ratio))
        if asimov:                                  # the root of the rounded data is within 2 u S1 / g' of a0
            r0 = abs(Fraction(a) - Fraction(float(a0[t]))) * gp / (K * unit)
            worst_a0 = max(worst_a0, float(r0))
            assert r0 <= 1, (C, kind, t, float(r0))
    print("C=%d %s %s: worst |g(ahat)| / (K u (S1 + S2)) = %.3f (K = %d)%s, %s" % (
        C, kind, "asimov" if asimov else "poisson", worst, K,
        ", worst |ahat - a0| g' / (K u (S1 + S2)) = %.3f" % worst_a0 if asimov else "", seen))
    if kind == "downward":
        assert seen["boundary"] > 0                 # the class exists to reach a = 0
    else:
        assert seen["interior"] > 0


def test_flat_cases():
    s = np.array([2.0, 3.0, 0.0])
    B = np.array([1.0, 1.0, 1.0])
    for sig, data in ((np.zeros(3), np.array([1.0, 2.0, 3.0])),          # S1 == 0
                      (s, np.zeros(3)),                                   # no data at all
                      (s, np.array([0.0, 0.0, 4.0]))):                    # data only where there is no signal
        a, nll, mu, st = run_case(sig, B, data)
        assert a == 0.0 and st == FIT_FLAT and list(mu) == list(B)
        assert nll == float(detector.poisson_host(B, data))


def test_bin_with_data_and_nothing_expected():
    """data_c > 0 = s_c = B_c: nll = +inf and NUSI_FIT_INFINITE; the bin does not enter the iteration, so ahat is that
    of the problem without it (x + 0.0 = x in every tree sum)."""
    rng = np.random.default_rng(5)
    for C in (2, 5, 17):
        s = rng.uniform(1.0, 10.0, C + 1)
        B = rng.uniform(0.1, 1.0, C + 1)
        data = rng.poisson(30.0 * s + B).astype(np.float64)
        s[C], B[C], data[C] = 0.0, 0.0, 3.0
        a, nll, mu, st = run_case(s, B, data)
        a1, nll1, mu1, st1 = run_case(s[:C], B[:C], data[:C])
        assert nll == math.inf and st & FIT_INFINITE and mu[C] == 0.0
        assert a == a1 and a > 0 and st == st1 | FIT_INFINITE and math.isfinite(nll1)
        assert np.array_equal(mu[:C], mu1)
    # ... also where nothing else is active: flat and infinite
    a, nll, mu, st = run_case(np.array([0.0, 0.0]), np.array([1.0, 0.0]), np.array([0.0, 2.0]))
    assert a == 0.0 and nll == math.inf and st == FIT_FLAT | FIT_INFINITE


@pytest.mark.parametrize("C", (1, 5, 17))
def test_nll_is_smallest_at_ahat(C):
    """Well-conditioned cases (hundreds of counts per bin, so a 1e-3 change of a moves nll by about 1e-6 of the counts,
    far above its rounding): nll(ahat) <= nll at ahat (1 +- 1e-3) and at 0, with poisson_host."""
    rng = np.random.default_rng(6 + C)
    for t in range(8):
        s = rng.uniform(1.0, 10.0, C)
        B = rng.uniform(0.1, 1.0, C)
        data = rng.poisson(rng.uniform(20.0, 200.0) * s + B).astype(np.float64)
        a, nll, mu, st = run_case(s, B, data, log=math.log)
        assert a > 0 and not st & ~FIT_STEPS_MASK
        for other in (a * (1 + 1e-3), a * (1 - 1e-3), 0.0):
            assert nll < float(detector.poisson_host(other * s + B, data, log=math.log)), (t, other)
    # at the boundary: nll(0) <= nll at small positive a
    s, B, data = np.full(C, 2.0), np.full(C, 50.0), np.full(C, 30.0)
    a, nll, mu, st = run_case(s, B, data, log=math.log)
    assert a == 0.0 and st == 1 | FIT_BOUNDARY
    assert nll < float(detector.poisson_host(0.01 * s + B, data, log=math.log))


def test_shapes_and_arguments():
    rng = np.random.default_rng(7)
    ntab, M, C, Q = 2, 9, 3, 4
    R, S = rng.random((ntab, M, C)), rng.random((Q, M))
    data, B = np.array([3.0, 0.0, 5.0]), np.array([0.5, 0.25, 0.0])
    a, nll, mu, st = detector.profile_host(R, S, data, background=B)
    assert a.shape == nll.shape == st.shape == (ntab, Q) and mu.shape == (ntab, Q, C) and st.dtype == np.int32
    # mu is the events' mu at the fitted scale, nll its statistic; the squeezed forms
    assert np.array_equal(mu[1], detector.events_host(R[1], S, scale=a[1], background=B))
    assert np.array_equal(nll, detector.poisson_host(mu, data))
    a1, nll1, mu1, st1 = detector.profile_host(R[1], S[2], data, background=B)
    assert a1.shape == () and mu1.shape == (C,) and a1 == a[1, 2] and st1 == st[1, 2] and np.array_equal(mu1, mu[1, 2])
    assert detector.profile_host(R, S, data)[0].shape == (ntab, Q)          # no background
    for bad in (data[:-1], data[None], np.array([1.0, -1.0, 0.0]), np.array([1.0, np.nan, 0.0]),
                np.array([1.0, np.inf, 0.0])):
        with pytest.raises(ValueError):
            detector.profile_host(R, S, bad)
    with pytest.raises(ValueError):
        detector.profile_host(R, S[:, :-1], data)
    with pytest.raises(ValueError):
        detector.profile_host(R, S, data, background=np.zeros(C + 1))


# --- the C ABI's new entry points --------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    from nusiprop_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "nusiprop_amd", "csrc")])
    return _lib


def test_header_declares_and_binding_lists_the_entry_points(lib):
    declared = set(re.findall(r"\b(nusi_[a-z_0-9A-Z]+)\s*\(", _header_text()))
    for f in NEW:
        assert f in declared and f in lib.EXPORTS, f
    defines = {k: int(v, 0) for k, v in re.findall(r"#define\s+NUSI_FIT_(\w+)\s+(\w+)", _header_text())}
    assert defines == {"ITER_MAX": 64, "STEPS_MASK": 0xFF, "FLAT": 0x100, "BOUNDARY": 0x200, "NOT_CONVERGED": 0x400,
                       "INFINITE": 0x800}
    for k, v in defines.items():
        assert getattr(lib, "FIT_" + k) == v == getattr(detector, "FIT_" + k), k


def test_library_exports_and_binds_the_entry_points(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = lib.load()
    dp, ip, vp, i = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int
    want = {"nusi_plan_response_profile": [vp, vp, i, dp, i, dp, vp, vp, vp, vp, vp],
            "nusi_plan_response_profile_host": [vp, dp, i, dp, i, dp, dp, dp, dp, ip]}
    for f in NEW:
        assert f in exported, f
        fn = getattr(L, f)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[f], f
    assert "k_detector_profile" in subprocess.check_output(["nm", "-D", lib.LIB_PATH], text=True)


def test_profile_without_a_gpu_fails_loudly(lib):
    """No plan without a GPU, and no CPU fallback behind the plan's call: NUSI_EHIP."""
    L = lib.load()
    if L.nusi_device_count() > 0:
        pytest.skip("a GPU is present")
    dp = ctypes.POINTER(ctypes.c_double)
    x, out = np.ones(8), np.zeros(8)
    xp, op = x.ctypes.data_as(dp), out.ctypes.data_as(dp)
    assert L.nusi_plan_response_profile_host(None, xp, 1, xp, 1, xp, op, None, None, None) == lib.NUSI_EHIP
    assert L.nusi_plan_response_profile(None, None, 1, xp, 1, xp, None, None, None, None, None) == lib.NUSI_EHIP
    assert not out.any()
