"""Response matrices on the GPU (nusi_plan_response: k_cascade_bs_impulse; nusi_plan_response_apply: k_response_apply).

G[p][n][k][b] is the flux nusi_plan_evolve gives a point whose tabulated slot holds the unit vector e_n (norm = 1), so
the existing API is the first yardstick, column by column; the oracle's power-law run (the construction of
tests/test_tabulated_source_gpu.py, whose grids, points and oracle cache are used here) is the second, and
response.apply_host (numpy, the defined summation order) is the apply kernel's.

Grids (the smallest with a partial group of source bins, a partial step pass and more than one FIFO hand-off):
  G6   N_E = 37, 6 steps,  M = 43:   one pass, three groups (the last of 10 columns)
  G47  N_E = 45, 47 steps, M = 92:   eight passes, the last of 5 steps; six groups, the last of 11 columns
  G63  N_E = 60, 63 steps, M = 123:  eleven passes
Tolerance: cases.FLUX_RTOL, the project's bound for summation-order differences; cases.rel_err demands exact zeros
where the reference has zeros.
"""
import ctypes

import numpy as np
import pytest

from tests import cases
from tests.test_tabulated_source_gpu import GRIDS, PHYS, _plan, _pt, _S, _sfr, oracle_pl   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

RGRIDS = ("G6", "G47", "G63")
MAXIS = {"G6": 43, "G47": 92, "G63": 123}


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


_RESP = {}


def _response(nusi, grid, nonres):
    """(G, G_fla) of both PHYS points on the default (MFMA) path, computed once per (grid, mode) and left unchanged."""
    key = (grid, nonres)
    if key not in _RESP:
        plan = _plan(nusi, grid, max_points=2, mode="auto")
        G, Gf = plan.response([_pt(grid, k, nonres) for k in range(len(PHYS))])
        assert plan.kernels()[1] == "k_cascade_bs_impulse", plan.kernels()
        plan.close()
        assert G.shape == Gf.shape == (2, MAXIS[grid], 3, GRIDS[grid][0])
        G.setflags(write=False)
        Gf.setflags(write=False)
        _RESP[key] = (G, Gf)
    return _RESP[key]


def _err(a, af, b, bf):
    return max(cases.rel_err(a, b), cases.rel_err(af, bf))


# --- 1. columns against the existing API ---------------------------------------------------------------------------
def _columns_by_evolve(nusi, grid, nonres, mode):
    """Column n of both points by plan.evolve: a point on a slot holding e_n, norm = 1."""
    from nusiprop_amd import sources
    M = MAXIS[grid]
    plan = _plan(nusi, grid, max_points=2 * M, mode=mode)
    for n in range(M):
        e = np.zeros(M)
        e[n] = 1.0
        plan.set_source(n, e)
    pts = [_pt(grid, k, nonres, si=7.5, norm=1.0, source_model=sources.tabulated(n)) for k in range(len(PHYS)) for n in range(M)]
    f, fl = plan.evolve(pts)
    plan.close()
    N = GRIDS[grid][0]
    return f.reshape(2, M, 3, N), fl.reshape(2, M, 3, N)


@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid,mode", [(g, "auto") for g in RGRIDS] + [("G47", "one")])
def test_columns_against_evolve(nusi, grid, mode, nonres):
    G, Gf = _response(nusi, grid, nonres)
    R, Rf = _columns_by_evolve(nusi, grid, nonres, mode)
    M, N = MAXIS[grid], GRIDS[grid][0]
    below = np.arange(N)[None, :] < np.arange(M)[:, None]          # [n, b]: b < n
    for k in range(len(PHYS)):
        # the condition of the comparison: no entry with b < n of the reference lies under rel_err's floor
        for ref in (R[k], Rf[k]):
            assert np.all(np.abs(ref[below[:, None, :].repeat(3, axis=1)]) > 1e-280 * np.max(np.abs(ref))), (grid, k)
        e = _err(G[k], Gf[k], R[k], Rf[k])
        same = np.array_equal(G[k], R[k]) and np.array_equal(Gf[k], Rf[k])
        print("%s %s nonres=%d point %d: response vs evolve of e_n, worst %.2e, bits equal: %s" % (grid, mode, nonres, k, e, same))
        assert e <= cases.FLUX_RTOL, (grid, mode, nonres, k, e)


# --- 2. structure ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", RGRIDS)
def test_structure(nusi, grid, nonres):
    M, N = MAXIS[grid], GRIDS[grid][0]
    at_or_above = (np.arange(N)[None, :] >= np.arange(M)[:, None])[None, :, None, :].repeat(2, axis=0).repeat(3, axis=2)
    for A in _response(nusi, grid, nonres):
        assert np.all(np.isfinite(A)) and np.all(A >= 0.0)
        assert np.all(A[:, 0] == 0.0)
        z = A[at_or_above]
        assert np.all(z == 0.0) and not np.any(np.signbit(z))      # +0.0 for b >= n
        assert not np.any(np.signbit(A[:, 0]))
        assert np.all(np.max(A[:, 1:], axis=(2, 3)) > 0.0)          # every column n >= 1 has a positive entry


# --- 3. against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", RGRIDS)
def test_power_law_against_the_oracle(nusi, oracle_pl, grid, nonres):
    from nusiprop_amd import response
    G, Gf = _response(nusi, grid, nonres)
    plan = _plan(nusi, grid, max_points=1)
    worst = 0.0
    for si in (2.0, 3.0):
        S = _S(plan, si)
        for k in range(len(PHYS)):
            f, fl, fs = oracle_pl(grid, k, nonres, si)
            e = _err(response.apply_host(G[k], S) / fs, response.apply_host(Gf[k], S) / fs, f, fl)
            print("%s nonres=%d point %d gamma %.1f: G . S / fs vs the oracle's power law %.2e" % (grid, nonres, k, si, e))
            worst = max(worst, e)
    plan.close()
    assert worst <= cases.FLUX_RTOL, worst


# --- 4. redshift weights ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_redshift_weights(nusi, grid):
    G, Gf = _response(nusi, grid, True)
    plan = _plan(nusi, grid, max_points=2, mode="auto")
    pts = [_pt(grid, k, True) for k in range(len(PHYS))]
    _, _, z = plan.source_axis()
    sfr = _sfr(z)
    G1, Gf1 = plan.response(pts, z_weight=sfr)                      # the star-formation rate passed explicitly
    assert np.array_equal(G1, G) and np.array_equal(Gf1, Gf)
    G2, Gf2 = plan.response(pts, z_weight=lambda v: 2.0 * _sfr([v])[0])
    e = _err(G2, Gf2, 2.0 * G, 2.0 * Gf)
    print("%s: w = 2 SFR vs twice G %.2e, bits equal: %s" % (grid, e, np.array_equal(G2, 2.0 * G) and np.array_equal(Gf2, 2.0 * Gf)))
    assert e <= cases.FLUX_RTOL, e
    # one step only: the source of bin n enters at b = n - i0, and every push goes to lower bins
    N, Nz, M = plan.N, plan.Nz, MAXIS[grid]
    i0 = Nz // 2
    w = np.zeros(Nz)
    w[i0] = sfr[i0]
    above = (np.arange(N)[None, :] > np.arange(M)[:, None] - i0)[None, :, None, :].repeat(2, axis=0).repeat(3, axis=2)
    for nonres in (True, False):
        G3, Gf3 = plan.response([dict(p, non_resonant=nonres) for p in pts], z_weight=w)
        for A in (G3, Gf3):
            assert np.all(A[above] == 0.0) and np.all(np.isfinite(A)) and np.all(A >= 0.0)
        n = i0 + N // 2
        assert np.all(G3[:, n, :, :n - i0 + 1] > 0.0)
    plan.close()


# --- 5. scan shape and chunking ----------------------------------------------------------------------------------------
def test_scan_and_chunks_bit_identical(nusi):
    from nusiprop_amd import _lib
    grid = "G47"
    pts = [_pt(grid, 0, True, mphi=float(m), g=float(g)) for m in np.logspace(6.0, 7.5, 4) for g in np.logspace(-2.0, -0.3, 5)]
    plan = _plan(nusi, grid, max_points=len(pts), mode="auto")
    G, Gf = plan.response(pts)
    assert "k_alpha_batch" in plan.kernels()[0] and plan.kernels()[1] == "k_cascade_bs_impulse", plan.kernels()
    assert "k_ga_dilogs_batch" in plan.ga_kernel(), plan.ga_kernel()
    assert len(plan.warnings(len(pts))) == len(pts)
    Ga, Ata, Aa = plan.tables(7)
    # the FIFO budget of one table: 16 columns x 3 N doubles per group of source bins
    per_kb = (-(-plan.T // 16) * 3 * plan.N * 16 * 8 + 1023) // 1024
    plan.set_option(_lib.OPT_RESPONSE_FIFO_KB, per_kb)
    Gc, Gfc = plan.response(pts)
    assert np.array_equal(Gc, G) and np.array_equal(Gfc, Gf)
    plan.set_option(_lib.OPT_RESPONSE_FIFO_KB, 0)
    one = _plan(nusi, grid, max_points=1, mode="auto")
    for j, p in enumerate(pts):
        g1, gf1 = one.response([p])
        assert np.array_equal(g1[0], G[j]) and np.array_equal(gf1[0], Gf[j]), j
        if j == 7:                                                   # ... and the call's tables are the response's
            t1 = one.tables(0)
            assert np.array_equal(t1[0], Ga) and np.array_equal(t1[1], Ata) and np.array_equal(t1[2], Aa)
    one.close()
    assert len(plan.stage_ms()) == 3
    plan.close()
    assert np.all(np.max(G[:, 1:], axis=(2, 3)) > 0.0)
    assert not np.array_equal(G[0], G[1])


# --- 6. the scalar fallback ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_scalar_fallback(nusi, grid):
    for nonres in (True, False):
        G, Gf = _response(nusi, grid, nonres)
        plan = _plan(nusi, grid, max_points=2, mode="scalar")
        Gs, Gfs = plan.response([_pt(grid, k, nonres) for k in range(len(PHYS))])
        assert plan.kernels()[1] == "k_cascade", plan.kernels()
        plan.close()
        e = _err(Gs, Gfs, G, Gf)
        print("%s nonres=%d: scalar k_cascade vs the impulse cascade %.2e" % (grid, nonres, e))
        assert e <= cases.FLUX_RTOL, e
        assert not np.any(np.signbit(Gs)) and not np.any(np.signbit(Gfs))


# --- 7. apply ---------------------------------------------------------------------------------------------------------
def _spectra(plan, Q):
    S = np.array([_S(plan, 1.8 + 0.1 * q) * (1.0 + 0.25 * q) for q in range(Q)])
    S[Q // 2, 40:] = 0.0                                             # a spectrum that ends
    S[-1, :10] = 0.0
    return S


@pytest.mark.parametrize("Q", [1, 5, 19])
def test_apply_is_apply_host(nusi, Q):
    from nusiprop_amd import response
    grid = "G47"
    G, Gf = _response(nusi, grid, True)
    plan = _plan(nusi, grid, max_points=2)
    S = _spectra(plan, Q)
    scale = np.array([0.3 + 1.7 * q for q in range(Q)])
    for A in (G, Gf):
        assert np.array_equal(plan.apply_response(A, S), response.apply_host(A, S))
        got = plan.apply_response(A, S, scale=scale)
        assert np.array_equal(got, response.apply_host(A, S, scale=scale))
        assert got.shape == (2, Q, 3, plan.N) and np.all(np.max(got, axis=(2, 3)) > 0.0)
    plan.close()


def test_apply_spectra_forms_and_errors(nusi):
    from nusiprop_amd import _lib, response, sources
    grid = "G47"
    G, _ = _response(nusi, grid, True)
    plan = _plan(nusi, grid, max_points=2)
    lo, hi, _z = plan.source_axis()
    fn = sources.broken_power_law(2.0, 3.0, 3e12)
    want = response.apply_host(G, np.array([sources.bin_integrals(fn, lo, hi), _S(plan, 2.5)]), scale=2.0)
    assert np.array_equal(plan.apply_response(G, [fn, _S(plan, 2.5)], scale=2.0), want)      # callables and vectors
    assert np.array_equal(plan.apply_response(G, fn, scale=2.0), want[:, :1])
    for k, bad in ((1, np.nan), (91, -1e-300), (5, np.inf)):
        Sb = _S(plan, 2.5)
        Sb[k] = bad
        with pytest.raises(nusi.NusiError) as ei:
            plan.apply_response(G, [_S(plan, 2.0), Sb])
        assert ei.value.code == _lib.NUSI_EPARAM, (k, ei.value.code)
    assert np.array_equal(plan.apply_response(G, [fn, _S(plan, 2.5)], scale=2.0), want)      # the plan stays usable
    plan.close()


# --- 8. surfaces --------------------------------------------------------------------------------------------------------
def test_object_api_and_pyprop(nusi):
    from nusiprop_amd import _lib
    grid = "G6"
    N, M = GRIDS[grid][0], MAXIS[grid]
    G, Gf = _response(nusi, grid, True)
    kw = _pt(grid, 0, True, si=2.5, norm=2.0)
    okw = {k: v for k, v in kw.items() if k != "source_model"}
    obj = nusi.pyprop(**okw, source_model=_lib.SOURCE_POWER_LAW)
    g, gf = obj.response()
    assert g.shape == (M, 3, N) and np.array_equal(g, G[0]) and np.array_equal(gf, Gf[0])
    assert not obj.evolved
    out = np.zeros((M, 3, N))
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(_lib.load().nusi_response(obj._h, None, None, out.ctypes.data_as(dp)))        # G NULL, G_fla only
    assert np.array_equal(out, Gf[0])
    _, _, z = obj.source_axis()
    g2, _ = obj.response(z_weight=_sfr(z))
    assert np.array_equal(g2, G[0])


def test_response_and_evolve_share_a_plan(nusi):
    from nusiprop_amd import _lib
    grid = "G47"
    G, Gf = _response(nusi, grid, True)
    pts = [_pt(grid, k, True, si=2.5) for k in range(len(PHYS))]
    ref = _plan(nusi, grid, max_points=2, mode="auto")
    f0, fl0 = ref.evolve(pts)
    ref.close()
    plan = _plan(nusi, grid, max_points=2, mode="auto")
    g, gf = plan.response(pts)
    f1, fl1 = plan.evolve(pts)                                       # a response, then an ordinary evolve
    assert np.array_equal(f1, f0) and np.array_equal(fl1, fl0) and plan.kernels()[1] != "k_cascade_bs_impulse"
    g2, gf2 = plan.response(pts)                                     # ... and the other order
    for a in (g, g2):
        assert np.array_equal(a, G)
    for a in (gf, gf2):
        assert np.array_equal(a, Gf)
    with pytest.raises(nusi.NusiError) as ei:
        plan.response(pts + pts[:1])                                 # n > max_points
    assert ei.value.code == _lib.NUSI_EPARAM
    bad = np.ones(plan.Nz)
    bad[3] = -1.0
    with pytest.raises(nusi.NusiError) as ei:
        plan.response(pts, z_weight=bad)
    assert ei.value.code == _lib.NUSI_EPARAM
    assert np.array_equal(plan.evolve(pts)[0], f0)
    plan.close()


def test_device_entry_points(nusi):
    """response_device and apply_response_device on caller-owned device buffers, G_fla left out (NULL)."""
    from nusiprop_amd import response
    # the HIP runtime libnusi.so itself links (tests/test_tabulated_source_gpu.py's approach)
    H = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so.7")
    vp = ctypes.c_void_p
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    grid = "G47"
    G, _ = _response(nusi, grid, True)
    plan = _plan(nusi, grid, max_points=2, mode="auto")
    arr = plan.params_array([_pt(grid, k, True) for k in range(len(PHYS))])
    S = _spectra(plan, 3)
    dG, dO = vp(), vp()
    assert H.hipMalloc(ctypes.byref(dG), G.nbytes) == 0
    out = np.zeros((2, 3, 3, plan.N))
    assert H.hipMalloc(ctypes.byref(dO), out.nbytes) == 0
    try:
        plan.response_device(arr, dG.value, None)
        assert plan.apply_response_device(dG.value, 2, S, dO.value) == 3
        assert H.hipDeviceSynchronize() == 0
        g = np.zeros_like(G)
        assert H.hipMemcpy(g.ctypes.data, dG, G.nbytes, 2) == 0
        assert H.hipMemcpy(out.ctypes.data, dO, out.nbytes, 2) == 0
    finally:
        H.hipFree(dG)
        H.hipFree(dO)
    plan.close()
    assert np.array_equal(g, G)
    assert np.array_equal(out, response.apply_host(G, S))
