"""The detector on the CPU: detector.fold_host / events_host / poisson_host / matrix (the yardsticks of the plan's
detector calls) and the ABI's new entry points -- header, binding list and library agree (tests/test_response.py's
approach).
"""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from nusiprop_amd import detector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nusi.h")
NEW = ["nusi_plan_set_detector", "nusi_plan_detector_bins", "nusi_plan_fold_flux", "nusi_plan_fold_flux_host",
       "nusi_plan_response_fold", "nusi_plan_response_fold_host", "nusi_plan_response_events",
       "nusi_plan_response_events_host"]


def test_fold_host_against_einsum():
    """Random non-negative data: two summation orders of K = 3 N non-negative products are each within gamma_K of the
    exact sum, so they differ by at most 2 gamma_K exact; `want` stands in for the exact sum and may itself lie gamma_K
    under it, hence want / (1 - gamma_K) (a factor 1 + 1e-14; the GPU tests use the issue's plain 2 gamma_K host)."""
    rng = np.random.default_rng(3)
    N, C = 37, 5
    D = rng.random((C, 3, N))
    G = rng.random((2, 9, 3, N))
    want = np.einsum("tnfb,cfb->tnc", G, D)
    got = detector.fold_host(G, D)
    assert got.shape == (2, 9, C)
    assert np.all(np.abs(got - want) <= 2 * detector.gamma(3 * N) * want / (1 - detector.gamma(3 * N)))
    flux = rng.random((4, 3, N))
    got = detector.fold_host(flux, D)
    want = np.einsum("pfb,cfb->pc", flux, D)
    assert got.shape == (4, C)
    assert np.all(np.abs(got - want) <= 2 * detector.gamma(3 * N) * want / (1 - detector.gamma(3 * N)))
    one = detector.fold_host(flux[1], D)                                # one row: (C,), another order again
    assert one.shape == (C,) and np.all(np.abs(one - want[1]) <= 2 * detector.gamma(3 * N) * want[1] / (1 - detector.gamma(3 * N)))
    assert not detector.fold_host(np.zeros((3, N)), D).any()
    with pytest.raises(ValueError):
        detector.fold_host(flux[:, :, :-1], D)
    assert detector.gamma(111) == 111 * 2.0 ** -53 / (1 - 111 * 2.0 ** -53)


def test_events_host_is_the_scalar_loop():
    """Bit for bit the defined sum: acc = 0.0; for n = 1 .. M-1 ascending acc = acc + R[n] * S[n] (Python floats), then
    scale * acc, then + background.  Bin 0 of the source axis is never read."""
    rng = np.random.default_rng(4)
    ntab, M, C, Q = 2, 9, 3, 4
    R, S = rng.random((ntab, M, C)), rng.random((Q, M))
    sc, bg = rng.random(Q) + 0.5, rng.random(C)
    S[1, 3] = 0.0
    got = detector.events_host(R, S, scale=sc, background=bg)
    plain = detector.events_host(R, S)
    assert got.shape == plain.shape == (ntab, Q, C)
    for t in range(ntab):
        for q in range(Q):
            for c in range(C):
                acc = 0.0
                for n in range(1, M):
                    acc = acc + float(R[t, n, c]) * float(S[q, n])
                assert plain[t, q, c] == acc
                assert got[t, q, c] == float(sc[q]) * acc + float(bg[c])
    S2 = S.copy()
    S2[:, 0] = 1e300
    assert np.array_equal(detector.events_host(R, S2), plain)
    # the squeezed forms
    assert np.array_equal(detector.events_host(R[1], S[2]), plain[1, 2])
    assert np.array_equal(detector.events_host(R, S[2], scale=3.0), 3.0 * plain[:, 2])
    with pytest.raises(ValueError):
        detector.events_host(R, S[:, :-1])


def test_poisson_host_is_the_scalar_loop():
    rng = np.random.default_rng(5)
    mu = rng.random((2, 3, 6)) * 10
    data = np.array([3.0, 0.0, 7.0, 1.0, 0.0, 12.0])
    got = detector.poisson_host(mu, data, log=math.log)
    assert got.shape == (2, 3)
    for t in range(2):
        for q in range(3):
            s = 0.0
            for c in range(6):
                m, d = float(mu[t, q, c]), float(data[c])
                s = s + (m if d == 0.0 else m - d * math.log(m))
            assert got[t, q] == s
    # data_c == 0: the log is not evaluated (mu_c = 0 there is fine); mu_c == 0 < data_c: +inf
    mu0 = mu.copy()
    mu0[0, 0, 1] = 0.0
    assert np.isfinite(detector.poisson_host(mu0, data, log=math.log)).all()
    mu0[1, 2, 0] = 0.0
    out = detector.poisson_host(mu0, data, log=math.log)
    assert out[1, 2] == np.inf and np.isfinite(np.delete(out.ravel(), 5)).all()
    assert detector.poisson_host(mu[0, 0], data).shape == ()
    with pytest.raises(ValueError):
        detector.poisson_host(mu, data[:-1])


def test_matrix_hand_computed_and_cap():
    lo, hi = np.array([1.0, 2.0]), np.array([2.0, 4.0])
    aeff = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]])
    mig = np.array([[0.5, 0.25], [0.5, 0.75], [0.0, 0.0]])
    D = detector.matrix(lo, hi, aeff, mig, exposure=4.0)
    assert D.shape == (3, 3, 2)
    # D[c][f][b] = exposure (hi_b - lo_b) aeff[f][b] mig[c][b]: widths 1 and 2 (every factor a small dyadic: exact)
    want = np.array([[[4 * 1 * a[0] * m[0], 4 * 2 * a[1] * m[1]] for a in aeff] for m in mig])
    assert np.array_equal(D, want)
    assert D[0, 1, 1] == 8.0 and D[1, 2, 0] == 10.0 and not D[2].any()
    # a callable of (f, E) at the geometric bin centres; one effective area for all flavours; the identity migration
    Dc = detector.matrix(lo, hi, lambda f, E: (f + 1) * E * E)
    assert Dc.shape == (2, 3, 2)
    assert Dc[0, 2, 0] == pytest.approx(3 * 2.0) and Dc[1, 0, 1] == pytest.approx(2 * 8.0) and Dc[0, 0, 1] == 0.0
    assert np.array_equal(detector.matrix(lo, hi, [1.0, 2.0], mig)[:, 0], detector.matrix(lo, hi, [1.0, 2.0], mig)[:, 2])
    # the cap: the identity migration of a 65-bin axis gives C = 65
    e = np.arange(66.0) + 1
    assert detector.matrix(e[:64], e[1:65], 1.0).shape == (64, 3, 64)
    with pytest.raises(ValueError):
        detector.matrix(e[:-1], e[1:], 1.0)
    with pytest.raises(ValueError):
        detector.matrix(lo, hi, -aeff, mig)


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
        assert f in declared, f
        assert f in lib.EXPORTS, f
    m = re.search(r"#define\s+NUSI_DETECTOR_BINS_MAX\s+(\d+)", _header_text())
    assert m and int(m.group(1)) == lib.DETECTOR_BINS_MAX == detector.BINS_MAX == 64


def test_library_exports_and_binds_the_entry_points(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = lib.load()
    dp, vp, i = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_int
    want = {"nusi_plan_set_detector": [vp, i, dp, dp], "nusi_plan_detector_bins": [vp],
            "nusi_plan_fold_flux": [vp, vp, i, vp, vp], "nusi_plan_fold_flux_host": [vp, dp, i, dp],
            "nusi_plan_response_fold": [vp, vp, i, vp, vp], "nusi_plan_response_fold_host": [vp, dp, i, dp],
            "nusi_plan_response_events": [vp, vp, i, dp, i, dp, dp, vp, vp, vp],
            "nusi_plan_response_events_host": [vp, dp, i, dp, i, dp, dp, dp, dp]}
    for f in NEW:
        assert f in exported, f
        fn = getattr(L, f)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[f], f
    # the kernels' translation unit is linked in
    syms = subprocess.check_output(["nm", "-D", lib.LIB_PATH], text=True)
    assert "k_detector_fold" in syms and "k_detector_events" in syms


def test_detector_without_a_gpu_fails_loudly(lib):
    """Without a GPU there is no plan to hand in, and every detector call refuses with NUSI_EHIP -- no CPU fallback."""
    L = lib.load()
    if L.nusi_device_count() > 0:                   # (the library's own count: the runtime it links)
        pytest.skip("a GPU is present")
    h = ctypes.c_void_p()
    assert L.nusi_plan_create(0, 20, 12.0, 17.0, 5.0, 1, ctypes.byref(h)) == lib.NUSI_EHIP and not h.value
    dp = ctypes.POINTER(ctypes.c_double)
    D, out = np.ones(60), np.zeros(8)
    Dp, op = D.ctypes.data_as(dp), out.ctypes.data_as(dp)
    assert L.nusi_plan_detector_bins(h) == 0
    assert L.nusi_plan_set_detector(h, 1, Dp, None) == lib.NUSI_EHIP
    assert b"HIP" in L.nusi_last_error() or b"device" in L.nusi_last_error()
    assert L.nusi_plan_fold_flux_host(h, Dp, 1, op) == lib.NUSI_EHIP
    assert L.nusi_plan_response_fold_host(h, Dp, 1, op) == lib.NUSI_EHIP
    assert L.nusi_plan_response_events_host(h, Dp, 1, Dp, 1, None, None, op, None) == lib.NUSI_EHIP
    assert L.nusi_plan_fold_flux(h, None, 1, None, None) == lib.NUSI_EHIP
    assert L.nusi_plan_response_fold(h, None, 1, None, None) == lib.NUSI_EHIP
    assert L.nusi_plan_response_events(h, None, 1, Dp, 1, None, None, None, None, None) == lib.NUSI_EHIP
    assert not out.any()
