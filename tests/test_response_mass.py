"""The mass-resolved response's surface and host definitions without a GPU (include/nusi.h "Mass-resolved response
matrices"): the new symbols, the pure functions nusi_mixing, nusi_mass_fractions and nusi_response_mass_shape, and
response.compose_host / cascade_host on inputs whose results are known exactly.  The GPU side is
tests/test_response_mass_gpu.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from nusiprop_amd import _lib, response, sources
from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"nusi_mixing": 2, "nusi_mass_fractions": 3, "nusi_response_mass_shape": 4, "nusi_plan_step_constants": 3,
         "nusi_plan_response_mass": 7, "nusi_plan_response_mass_host": 6, "nusi_plan_response_compose": 8,
         "nusi_plan_response_compose_host": 7, "nusi_response_mass": 4}
# flavour composition -> the issue's table of kappa for normal ordering (three decimals)
TABLE = {(1, 1, 1): (0.333, 0.333, 0.333), (1, 2, 0): (0.276, 0.345, 0.379), (0, 1, 0): (0.074, 0.369, 0.557),
         (1, 0, 0): (0.681, 0.297, 0.022)}
dp = ctypes.POINTER(ctypes.c_double)


def test_symbols_and_prototypes():
    text = open(os.path.join(ROOT, "include", "nusi.h")).read()
    L = _lib.load()
    for name, nargs in NAMES.items():
        assert name in _lib.EXPORTS and re.search(r"\bint %s\s*\(" % name, text), name
        assert len(getattr(L, name).argtypes) == nargs, name
    hpp = open(os.path.join(ROOT, "include", "nuSIprop.hpp")).read()
    assert "void response_mass(" in hpp and "nusi_response_mass(h_" in hpp
    import nusiprop_amd
    for who, names in ((nusiprop_amd.Plan, ("response_mass", "response_mass_device", "compose_response",
                                            "compose_response_device", "step_constants")),
                       (nusiprop_amd.pyprop, ("response_mass",)), (nusiprop_amd, ("mixing",)),
                       (sources, ("mass_fractions", "mixing")),
                       (response, ("cascade_host", "response_mass_host", "compose_host"))):
        for n in names:
            assert callable(getattr(who, n)), (who, n)


def test_without_a_plan_the_calls_refuse():
    L = _lib.load()
    one = np.ones(9)
    p = one.ctypes.data_as(dp)
    refused = (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_response_mass(None, None, 1, None, None, None, None) in refused
    assert L.nusi_plan_response_mass_host(None, None, 1, None, p, p) in refused
    assert L.nusi_plan_response_compose(None, None, 1, 3, p, 1, None, None) in refused
    assert L.nusi_plan_response_compose_host(None, p, 1, 3, p, 1, p) in refused
    assert L.nusi_plan_step_constants(None, p, p) == _lib.NUSI_EPARAM
    assert L.nusi_response_mass(None, None, p, p) == _lib.NUSI_EPARAM
    assert L.nusi_mixing(1, None) == _lib.NUSI_EPARAM


@pytest.mark.parametrize("normal", [True, False], ids=["normal", "inverted"])
def test_mixing_is_the_oracles(oracle_mod, normal):
    import nusiprop_amd
    kw = dict(mphi=1e7, g=0.1, mntot=0.1, si=2.0, norm=1.0, majorana=True, non_resonant=True, normal_ordering=normal,
              N_bins_E=20, lEmin=12.0, lEmax=17.0, zmax=5.0, flav=2, phiphi=False, source_model=1)
    want = oracle_mod.Oracle(**cases.oracle_kwargs(kw)).mixing()
    got = nusiprop_amd.mixing(normal)
    assert got.shape == (3, 3) and np.array_equal(got, want)
    assert np.array_equal(sources.mixing(normal_ordering=normal), want)
    assert np.allclose(got.sum(axis=0), 1.0, atol=1e-15) and np.allclose(got.sum(axis=1), 1.0, atol=1e-15)


def test_mass_fractions():
    rng = np.random.default_rng(5)
    comps = [np.array(c, dtype=np.float64) for c in TABLE] + [rng.random(3) * 10.0 ** rng.integers(-3, 4) for _ in range(20)]
    comps += [np.array([0.0, 0.0, 2.5]), np.array([1e-300, 0.0, 0.0]), np.array([3e200, 1e200, 0.0])]
    for normal in (True, False):
        U2 = sources.mixing(normal)
        for phi in comps:
            want = np.array([((phi[0] * U2[0, k] + phi[1] * U2[1, k]) + phi[2] * U2[2, k]) / ((phi[0] + phi[1]) + phi[2])
                             for k in range(3)])
            got = sources.mass_fractions(phi, normal_ordering=normal)
            assert np.array_equal(got, want), (normal, phi)
            assert np.all(got >= 0.0) and abs(got.sum() - 1.0) < 1e-14
    for comp, row in TABLE.items():
        assert np.all(np.abs(sources.mass_fractions(comp) - np.array(row)) <= 5.01e-4), comp
    # the interacting share sum_k kappa_k u_k for the tau coupling: 0.333, 0.376, 0.275
    u = sources.mixing(True)[2]
    for comp, share in (((1, 1, 1), 0.333), ((0, 1, 0), 0.376), ((1, 0, 0), 0.275)):
        assert abs(float(sources.mass_fractions(comp) @ u) - share) <= 5.01e-4, comp
    for bad in ((-1.0, 1.0, 1.0), (np.nan, 1.0, 1.0), (1.0, np.inf, 0.0), (0.0, 0.0, 0.0), (-0.0, 0.0, 0.0)):
        with pytest.raises(_lib.NusiError) as ei:
            sources.mass_fractions(bad)
        assert ei.value.code == _lib.NUSI_EPARAM, bad
    L = _lib.load()
    assert L.nusi_mass_fractions(1, None, np.zeros(3).ctypes.data_as(dp)) == _lib.NUSI_EPARAM


def _shape(N, Nz, n):
    d = ctypes.c_longlong(-1)
    return _lib.load().nusi_response_mass_shape(N, Nz, n, ctypes.byref(d)), d.value


@pytest.mark.parametrize("N,Nz", ((300, 48), (37, 7), (1, 2), (60, 64)))
def test_the_size_limit(N, Nz):
    M = N + Nz - 1
    first = -(-(1 << 31) // (3 * M))                               # the first table count with n 3 M >= 2^31
    assert first * 3 * M >= 1 << 31 > (first - 1) * 3 * M
    assert _shape(N, Nz, first)[0] == _lib.NUSI_EPARAM and "2^31" in _lib.last_error()
    code, doubles = _shape(N, Nz, first - 1)
    assert code == _lib.NUSI_OK and doubles == (first - 1) * 3 * M * 3 * N
    assert _lib.load().nusi_response_mass_shape(N, Nz, first - 1, None) == _lib.NUSI_OK       # doubles may be NULL
    for bad in ((0, Nz, 1), (N, 1, 1), (N, Nz, 0), (N, Nz, -3)):
        assert _shape(*bad)[0] == _lib.NUSI_EPARAM, bad


def test_compose_host():
    rng = np.random.default_rng(11)
    ntab, Qc, shape = 3, 4, (5, 3, 7)
    A = rng.standard_normal((ntab, 3) + shape) * 10.0 ** rng.integers(-20, 5, size=(ntab, 3) + shape)
    A[:, :, 0] = 0.0                                                # the zero column
    kap = rng.random((ntab, Qc, 3))
    kap[1, 2, 0] = 0.0
    got = response.compose_host(A, kap)
    want = np.zeros((ntab, Qc) + shape)
    for t in range(ntab):                                           # the scalar loop: products and sums rounded separately
        for c in range(Qc):
            for x in np.ndindex(*shape):
                p0, p1, p2 = kap[t, c, 0] * A[(t, 0) + x], kap[t, c, 1] * A[(t, 1) + x], kap[t, c, 2] * A[(t, 2) + x]
                want[(t, c) + x] = (p0 + p1) + p2
    assert got.shape == want.shape and np.array_equal(got, want)
    z = got[:, :, 0]
    assert np.all(z == 0.0) and not np.any(np.signbit(z))           # +0.0 stays +0.0
    # against einsum on non-negative rows (no cancellation): a few ulp
    Ap = np.abs(A)
    ein = np.einsum("tck,tk...->tc...", kap, Ap)
    gp = response.compose_host(Ap, kap)
    nz = ein != 0
    worst = float(np.max(np.abs(gp[nz] - ein[nz]) / ein[nz]))
    print("compose_host vs einsum: worst %.2e" % worst)
    assert worst <= 4 * np.finfo(float).eps
    # the broadcast forms
    assert np.array_equal(response.compose_host(A, kap[0]), response.compose_host(A, np.broadcast_to(kap[0], (ntab, Qc, 3))))
    one = response.compose_host(A, kap[0, 1])
    assert one.shape == (ntab,) + shape and np.array_equal(one, response.compose_host(A, kap[0])[:, 1])
    for bad in (np.array([0.3, -1e-300, 0.3]), np.array([0.3, np.nan, 0.3]), np.ones((2, 2, 3)), np.ones(4)):
        with pytest.raises(ValueError):
            response.compose_host(A, bad)


@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
def test_cascade_host_routes_each_mass_state(nonres):
    """All-zero tables: nothing interacts, so bin b of state k ends as the sum of its own source terms over the steps,
    and the flavour flux is the |U|^2 expression of those -- the routing per mass state and the finalise.  Bin widths
    are powers of two and the sources small integers, so every operation is exact."""
    N, Nz = 6, 5
    T = N + Nz - 2
    Emin = 2.0 ** np.arange(3, 3 + N)
    Emax = 2.0 * Emin                                               # dE_b = 2^(3 + b)
    rng = np.random.default_rng(3)
    src = rng.integers(0, 64, size=(2, 3, Nz, N)).astype(np.float64)
    src[:, 1] *= 4.0
    src[:, 2, :, ::2] = 0.0
    src[..., 0, :] = 0.0                                            # no source at step 0
    U2 = sources.mixing(False)
    u = U2[1]
    zeros = (np.zeros(T), np.zeros(T), np.zeros(T * (T - 1) // 2))
    flux, fla = response.cascade_host(*zeros, Emin, Emax, np.full(Nz, 0.5), np.full(Nz, 3.0), u, U2, nonres, src)
    assert flux.shape == fla.shape == (2, 3, N)
    dE = Emax - Emin
    assert np.array_equal(flux * dE, src.sum(axis=-2))
    f = flux
    want = np.stack([U2[q, 0] * f[:, 0] + U2[q, 1] * f[:, 1] + U2[q, 2] * f[:, 2] for q in range(3)], axis=1)
    assert np.array_equal(fla, want)
    # a source in one state only leaves the other two exactly zero
    only = np.zeros_like(src)
    only[:, 1] = src[:, 1]
    f1, _ = response.cascade_host(*zeros, Emin, Emax, np.full(Nz, 0.5), np.full(Nz, 3.0), u, U2, nonres, only)
    assert np.array_equal(f1[:, 1], flux[:, 1]) and not np.any(f1[:, 0]) and not np.any(f1[:, 2])


def test_impulse_sources_and_tabulated_src_host():
    N, Nz = 4, 3
    M = N + Nz - 1
    sc, w, z = np.array([0.0, 0.7, 1.3]), np.array([9.0, 2.0, 5.0]), np.array([0.0, 0.1, 0.21])
    src = response.impulse_sources(sc, w, z, N)
    assert src.shape == (3, M, 3, Nz, N)
    for j in range(3):
        for n in range(M):
            for k in range(3):
                for i in range(Nz):
                    for b in range(N):
                        want = sc[i] * (w[i] / (1 + z[i])) if (k == j and b + i == n and i >= 1) else 0.0
                        assert src[j, n, k, i, b] == want
    # the whole unit source: tabulated_src at norm = 3 on a unit vector, the same bits
    e = np.zeros(M)
    e[3] = 1.0
    assert np.array_equal(response.tabulated_src_host(sc, 3.0, w, z, e, N), src[1, 3, 1])
