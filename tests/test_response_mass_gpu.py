"""Mass-resolved response matrices on the GPU (nusi_plan_response_mass: k_cascade_mass_impulse, k_cascade_mass;
nusi_plan_response_compose: k_response_compose).

G3[p][j][n][k][b] is the response to a unit source emitted wholly into mass state j (include/nusi.h).  No existing
call takes a source per mass state, so the yardstick is the definition itself on the host, response.cascade_host --
k_cascade's loop nest in numpy -- and it is validated first, against plan.evolve on the scalar kernel (test 1).
Grids, points and the oracle cache are those of tests/test_tabulated_source_gpu.py; one point is added with the
inverted ordering, the mu coupling and Dirac neutrinos.  Tolerance: cases.FLUX_RTOL, the project's bound for
summation-order differences; bit claims use np.array_equal.  Every test prints its worst measured error.
"""
import ctypes

import numpy as np
import pytest

from tests import cases
from tests.test_tabulated_source_gpu import GRIDS, PHYS, _plan, _pt, _S, _sfr, oracle_pl   # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

RGRIDS = ("G6", "G47", "G63")
MAXIS = {"G6": 43, "G47": 92, "G63": 123}
INV = dict(normal_ordering=False, flav=1, majorana=False)     # the added point (on PHYS[0]'s mediator)
NPT = len(PHYS) + 1
THIRDS = (1.0 / 3.0, 1.0 / 3.0, 1.0 / 3.0)
FLAVOURS = ((1.0, 2.0, 0.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0))   # pion decay, muon-damped, neutron decay


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


def _point(grid, k, nonres, **over):
    return _pt(grid, 0, nonres, **dict(INV, **over)) if k == len(PHYS) else _pt(grid, k, nonres, **over)


def _u_U2(nusi, p):
    U2 = nusi.mixing(p["normal_ordering"])
    return U2[p["flav"]].copy(), U2


_MASS, _HOST = {}, {}


def _mass(nusi, grid, nonres):
    """(G3, G3_fla, tables, grid constants) of the three points on the default path, once per (grid, mode), read-only."""
    key = (grid, nonres)
    if key not in _MASS:
        plan = _plan(nusi, grid, max_points=NPT, mode="auto")
        G3, G3f = plan.response_mass([_point(grid, k, nonres) for k in range(NPT)])
        assert plan.kernels()[1] == "k_cascade_mass_impulse", plan.kernels()
        tabs = [plan.tables(k) for k in range(NPT)]
        lo, hi, z = plan.source_axis()
        const = (lo[:plan.N].copy(), hi[:plan.N].copy(), z) + plan.step_constants()
        plan.close()
        assert G3.shape == G3f.shape == (NPT, 3, MAXIS[grid], 3, GRIDS[grid][0])
        G3.setflags(write=False)
        G3f.setflags(write=False)
        _MASS[key] = (G3, G3f, tabs, const)
    return _MASS[key]


def _host(nusi, grid, nonres, k, w=None):
    """The host definition's (G3, G3_fla) of point k on the tables of the device call, once per case, read-only."""
    from nusiprop_amd import response
    key = (grid, nonres, k)
    if w is not None or key not in _HOST:
        _, _, tabs, (Emin, Emax, z, sc, ss) = _mass(nusi, grid, nonres)
        u, U2 = _u_U2(nusi, _point(grid, k, nonres))
        H = response.response_mass_host(*tabs[k], Emin, Emax, sc, ss, z, _sfr(z) if w is None else w, u, U2, nonres)
        if w is not None:
            return H
        for a in H:
            a.setflags(write=False)
        _HOST[key] = H
    return _HOST[key]


def _err(a, af, b, bf):
    return max(cases.rel_err(a, b), cases.rel_err(af, bf))


def _below(M, N):
    return np.arange(N)[None, :] < np.arange(M)[:, None]          # [n, b]: b < n


# --- 1. the yardstick itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", RGRIDS)
def test_cascade_host_is_the_scalar_cascade(nusi, grid, nonres):
    """cascade_host on the plan's own tables and the equal-thirds tabulated source term of a power-law slot against
    plan.evolve of that slot on the scalar kernel k_cascade."""
    from nusiprop_amd import response, sources
    plan = _plan(nusi, grid, max_points=NPT, mode="scalar")
    lo, hi, z = plan.source_axis()
    w = _sfr(z)
    S = _S(plan, 2.0)
    plan.set_source(0, S, z_weight=w)
    pts = [_point(grid, k, nonres, norm=1.5, source_model=sources.tabulated(0)) for k in range(NPT)]
    f, fl = plan.evolve(pts)
    assert plan.kernels()[1] == "k_cascade", plan.kernels()
    sc, ss = plan.step_constants()
    N = plan.N
    src = response.tabulated_src_host(sc, 1.5, w, z, S, N)
    worst = 0.0
    for k in range(NPT):
        u, U2 = _u_U2(nusi, pts[k])
        hf, hfl = response.cascade_host(*plan.tables(k), lo[:N], hi[:N], sc, ss, u, U2, nonres, np.stack([src] * 3))
        e = _err(hf, hfl, f[k], fl[k])
        print("%s nonres=%d point %d: cascade_host vs k_cascade %.2e, bits equal: %s"
              % (grid, nonres, k, e, np.array_equal(hf, f[k]) and np.array_equal(hfl, fl[k])))
        assert np.all(f[k] > 0.0)
        worst = max(worst, e)
    plan.close()
    assert worst <= cases.FLUX_RTOL, worst


# --- 2. the kernel against the definition ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", RGRIDS)
def test_against_the_host_definition(nusi, grid, nonres):
    G3, G3f, _, _ = _mass(nusi, grid, nonres)
    M, N = MAXIS[grid], GRIDS[grid][0]
    worst = 0.0
    for k in range(NPT):
        H, Hf = _host(nusi, grid, nonres, k)
        # the comparison's condition: no non-zero entry of the reference lies under rel_err's floor
        for ref in (H, Hf):
            nzr = ref[ref != 0.0]
            assert np.all(np.abs(nzr) > 1e-280 * np.max(np.abs(ref))), (grid, k)
        e = _err(G3[k], G3f[k], H, Hf)
        sign = np.array_equal(np.sign(G3[k]), np.sign(H)) and np.array_equal(np.sign(G3f[k]), np.sign(Hf))
        print("%s nonres=%d point %d: k_cascade_mass_impulse vs response_mass_host %.2e, signs equal: %s, bits equal: %s"
              % (grid, nonres, k, e, sign, np.array_equal(G3[k], H) and np.array_equal(G3f[k], Hf)))
        worst = max(worst, e)
        assert sign, (grid, nonres, k)
    assert worst <= cases.FLUX_RTOL, worst


# --- 3. structure -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", RGRIDS)
def test_structure(nusi, grid, nonres):
    G3, G3f, _, _ = _mass(nusi, grid, nonres)
    M, N = MAXIS[grid], GRIDS[grid][0]
    above = ~_below(M, N)
    for A in (G3, G3f):
        assert np.all(np.isfinite(A))
        assert np.all(A[:, :, 0] == 0.0) and not np.any(np.signbit(A[:, :, 0]))
        z = A[:, :, above[:, None, :].repeat(3, axis=1)]
        assert np.all(z == 0.0) and not np.any(np.signbit(z))      # +0.0 for b >= n
    for j in range(3):
        blk = G3[:, j, :, j]                                        # the block k = j, [p][n][b]
        assert np.all(blk >= 0.0) and np.all(np.max(blk[:, 1:], axis=2) > 0.0), j
    nneg, rel = 0, 0.0
    for k in range(NPT):
        H, Hf = _host(nusi, grid, nonres, k)
        for A, R in ((G3[k], H), (G3f[k], Hf)):
            assert np.array_equal(A < 0.0, R < 0.0), (grid, nonres, k)     # negative only where the definition is
        neg = G3[k] < 0.0
        nneg += int(neg.sum())
        # where they are: the column's topmost populated bin b = min(n, N) - 1 (the one zero right-hand side that no
        # later step's inflow covers), so at most one per (j, k != j, n)
        top = np.arange(N)[None, :] == (np.minimum(np.arange(M), N) - 1)[:, None]
        assert not np.any(neg & ~top[None, :, None, :]), (grid, nonres, k)
        for j in range(3):
            for kk in range(3):
                m = neg[j, :, kk]
                if m.any():
                    assert kk != j
                    rel = max(rel, float(np.max(-G3[k, j, :, kk][m] / G3[k, j, :, j][m])))
    print("%s nonres=%d: %d negative entries of G3 (k != j), largest |G3[j,n,k,b]| / G3[j,n,j,b] = %.3e" % (grid, nonres, nneg, rel))


# --- 4. equal thirds are the plain response -------------------------------------------------------------------------------
@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", RGRIDS)
def test_thirds(nusi, oracle_pl, grid, nonres):
    from nusiprop_amd import response
    G3, G3f, _, _ = _mass(nusi, grid, nonres)
    plan = _plan(nusi, grid, max_points=NPT, mode="auto")
    G, Gf = plan.response([_point(grid, k, nonres) for k in range(NPT)])
    C, Cf = response.compose_host(G3, THIRDS), response.compose_host(G3f, THIRDS)
    e = _err(C, Cf, G, Gf)
    print("%s nonres=%d: compose_host(G3, thirds) vs Plan.response %.2e" % (grid, nonres, e))
    assert np.all(G >= 0.0) and np.any(G > 0.0)
    worst = e
    for si in (2.0, 3.0):
        S = _S(plan, si)
        for k in range(len(PHYS)):
            f, fl, fs = oracle_pl(grid, k, nonres, si)
            eo = _err(response.apply_host(C[k], S) / fs, response.apply_host(Cf[k], S) / fs, f, fl)
            print("%s nonres=%d point %d gamma %.1f: thirds . S / fs vs the oracle's power law %.2e" % (grid, nonres, k, si, eo))
            worst = max(worst, eo)
    plan.close()
    assert worst <= cases.FLUX_RTOL, worst


# --- 5. physical compositions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", RGRIDS)
def test_physical_compositions_are_non_negative(nusi, grid, nonres):
    from nusiprop_amd import response, sources
    G3, G3f, _, _ = _mass(nusi, grid, nonres)
    low = np.inf
    for phi in FLAVOURS:
        for k in range(NPT):
            kap = sources.mass_fractions(phi, normal_ordering=_point(grid, k, nonres)["normal_ordering"])
            assert np.all(kap > 0.0) and abs(kap.sum() - 1.0) < 1e-14
            H, Hf = _host(nusi, grid, nonres, k)
            for R in (H, Hf):                                      # the condition, on the host reference
                c = response.compose_host(R[None], kap)
                assert np.all(c >= 0.0), (phi, k)
            for A in (G3[k], G3f[k]):                              # ... then the device result
                c = response.compose_host(A[None], kap)
                assert np.all(c >= 0.0) and not np.any(np.signbit(c)), (phi, k)
                low = min(low, float(np.min(c[c > 0.0])))
    print("%s nonres=%d: composed G, G_fla >= 0 for 1:2:0, 0:1:0, 1:0:0; smallest positive entry %.3e" % (grid, nonres, low))


# --- 6. the compose kernel ------------------------------------------------------------------------------------------------
def _D(C, N):
    D = (0.5 + 1.5 * np.random.default_rng(7 + 100 * C).random((C, 3, N))) * 1e3
    D[0, 1] = 0.0
    return D


def _kappas(nusi, grid, Qc):
    """(NPT, Qc, 3): per table its ordering's fractions (the inverted point's differ), then thirds and one with a zero."""
    from nusiprop_amd import sources
    rows = list(FLAVOURS) + [(1.0, 1.0, 1.0)]
    k = np.array([[sources.mass_fractions(rows[c], normal_ordering=_point(grid, t, True)["normal_ordering"])
                   for c in range(Qc)] for t in range(NPT)])
    if Qc > 1:
        k[1, 1] = (0.0, 2.5, 0.25)                                  # need not sum to 1; a zero share
    return k


@pytest.mark.parametrize("Qc", [1, 4])
def test_compose_is_compose_host(nusi, Qc):
    from nusiprop_amd import response
    grid = "G47"
    G3, G3f, _, _ = _mass(nusi, grid, True)
    M, N, C = MAXIS[grid], GRIDS[grid][0], 5
    plan = _plan(nusi, grid, max_points=NPT)
    plan.set_detector(_D(C, N))
    R3 = plan.fold_response(G3f.reshape(3 * NPT, M, 3, N)).reshape(NPT, 3, M, C)
    kap = _kappas(nusi, grid, Qc)
    assert not np.array_equal(kap[0], kap[2])                       # mixed orderings
    for A in (G3, G3f, R3):                                         # X = M 3 N twice, then X = M C
        got = plan.compose_response(A, kap)
        want = response.compose_host(A, kap)
        assert got.shape == (NPT, Qc) + A.shape[2:]
        same = np.array_equal(got, want)
        print("compose Qc=%d X=%d per table: bits equal %s" % (Qc, int(np.prod(A.shape[2:])), same))
        assert same
        zero = np.broadcast_to((A == 0.0).all(axis=1)[:, None], got.shape)
        assert np.all(got[zero] == 0.0) and not np.any(np.signbit(got[zero]))          # +0.0 is kept
        for kb in (kap[0], kap[0, 0]):                              # broadcast forms: (Qc, 3) and (3,)
            assert np.array_equal(plan.compose_response(A, kb), response.compose_host(A, kb))
    assert plan.compose_response(G3, kap[0, 0]).shape == (NPT, M, 3, N)
    plan.close()


# --- 7. the stack in the existing calls -----------------------------------------------------------------------------------
def test_stack_in_apply_and_fold(nusi):
    grid = "G47"
    G3, G3f, _, _ = _mass(nusi, grid, True)
    M, N, C = MAXIS[grid], GRIDS[grid][0], 5
    plan = _plan(nusi, grid, max_points=NPT)
    S = np.array([_S(plan, 2.0), 1.5 * _S(plan, 2.7)])
    kap = _kappas(nusi, grid, 1)[:, 0]                              # (NPT, 3): pion decay per table's ordering
    stack = np.ascontiguousarray(G3f.reshape(3 * NPT, M, 3, N))
    lhs = plan.apply_response(plan.compose_response(G3f, kap[:, None, :])[:, 0], S)
    parts = plan.apply_response(stack, S).reshape(NPT, 3, len(S), 3, N)
    rhs = sum(kap[:, j, None, None, None] * parts[:, j] for j in range(3))
    e = cases.rel_err(lhs, rhs)
    print("apply(compose(G3_fla)) vs sum_j kappa_j apply(G3_fla[:, j]): %.2e" % e)
    assert e <= cases.FLUX_RTOL, e
    plan.set_detector(_D(C, N))
    R3 = plan.fold_response(stack).reshape(NPT, 3, M, C)
    Rc = plan.compose_response(R3, kap[:, None, :])[:, 0]
    Rd = plan.fold_response(plan.compose_response(G3f, kap[:, None, :])[:, 0])
    e2 = cases.rel_err(Rc, Rd)
    print("compose(fold(stack)) vs fold(compose(G3_fla)): %.2e" % e2)
    assert e2 <= cases.FLUX_RTOL, e2
    plan.close()


# --- 8. scans and budgets ---------------------------------------------------------------------------------------------------
def test_scan_and_budgets_bit_identical(nusi):
    from nusiprop_amd import _lib
    grid = "G47"
    pts = [_pt(grid, 0, True, mphi=float(m), g=0.3) for m in np.logspace(6.0, 7.5, 3)]
    pts += [_pt(grid, 1, True, **INV), _pt(grid, 0, True, g=0.07, **INV)]
    plan = _plan(nusi, grid, max_points=len(pts), mode="auto")
    G3, G3f = plan.response_mass(pts)
    assert plan.kernels()[1] == "k_cascade_mass_impulse", plan.kernels()
    assert len(plan.warnings(len(pts))) == len(pts) and len(plan.stage_ms()) == 3
    # the smallest budget: one table's FIFO (three source states x groups x 16 columns x 3 N doubles) per launch
    per_kb = (3 * -(-plan.T // 16) * 3 * plan.N * 16 * 8 + 1023) // 1024
    plan.set_option(_lib.OPT_RESPONSE_FIFO_KB, per_kb)
    Gc, Gfc = plan.response_mass(pts)
    assert np.array_equal(Gc, G3) and np.array_equal(Gfc, G3f)
    plan.set_option(_lib.OPT_RESPONSE_FIFO_KB, 1)                   # below one table: still one table per launch
    Gc, Gfc = plan.response_mass(pts)
    assert np.array_equal(Gc, G3) and np.array_equal(Gfc, G3f)
    plan.close()
    one = _plan(nusi, grid, max_points=1, mode="auto")
    for j, p in enumerate(pts):
        g1, gf1 = one.response_mass([p])
        assert np.array_equal(g1[0], G3[j]) and np.array_equal(gf1[0], G3f[j]), j
    one.close()
    assert not np.array_equal(G3[0], G3[1])
    print("five-table scan: each table alone and the smallest FIFO budgets give equal bits")


# --- 9. the scalar fallback ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_scalar_fallback(nusi, grid):
    for nonres in (True, False):
        G3, G3f, _, _ = _mass(nusi, grid, nonres)
        plan = _plan(nusi, grid, max_points=NPT, mode="scalar")
        Gs, Gfs = plan.response_mass([_point(grid, k, nonres) for k in range(NPT)])
        assert plan.kernels()[1] == "k_cascade_mass", plan.kernels()
        plan.close()
        e = _err(Gs, Gfs, G3, G3f)
        eh, bits = 0.0, True
        for k in range(NPT):
            H, Hf = _host(nusi, grid, nonres, k)
            eh = max(eh, _err(Gs[k], Gfs[k], H, Hf))
            bits = bits and np.array_equal(Gs[k], H) and np.array_equal(Gfs[k], Hf)
        print("%s nonres=%d: k_cascade_mass vs k_cascade_mass_impulse %.2e, vs response_mass_host %.2e (bits equal: %s)"
              % (grid, nonres, e, eh, bits))
        assert e <= cases.FLUX_RTOL and eh <= cases.FLUX_RTOL, (e, eh)


# --- 10. redshift weights -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_redshift_weights(nusi, grid):
    G3, G3f, _, _ = _mass(nusi, grid, True)
    plan = _plan(nusi, grid, max_points=NPT, mode="auto")
    pts = [_point(grid, k, True) for k in range(NPT)]
    _, _, z = plan.source_axis()
    sfr = _sfr(z)
    G1, Gf1 = plan.response_mass(pts, z_weight=sfr)                 # the star-formation rate passed explicitly
    assert np.array_equal(G1, G3) and np.array_equal(Gf1, G3f)
    # one step only: the source of bin n enters at b = n - i0, and every push goes to lower bins
    N, Nz, M = plan.N, plan.Nz, MAXIS[grid]
    i0 = Nz // 2
    w = np.zeros(Nz)
    w[i0] = sfr[i0]
    above = (np.arange(N)[None, :] > np.arange(M)[:, None] - i0)
    for nonres in (True, False):
        Gw, Gfw = plan.response_mass([dict(p, non_resonant=nonres) for p in pts], z_weight=w)
        for A in (Gw, Gfw):
            assert np.all(np.isfinite(A)) and np.all(A[:, :, above[:, None, :].repeat(3, axis=1)] == 0.0)
        n = i0 + N // 2
        for j in range(3):
            assert np.all(Gw[:, j, n, j, :n - i0 + 1] > 0.0)
    plan.close()
    print("%s: explicit SFR equal bits; a single-step weight's support is b <= n - i0" % grid)


# --- 11. surfaces -----------------------------------------------------------------------------------------------------------------
def test_object_pyprop_and_facade(nusi):
    from nusiprop_amd import _lib, response, sources
    grid = "G6"
    N, M = GRIDS[grid][0], MAXIS[grid]
    G3, G3f, _, _ = _mass(nusi, grid, True)
    kw = _pt(grid, 0, True, si=2.5, norm=2.0)
    okw = {k: v for k, v in kw.items() if k != "source_model"}
    obj = nusi.pyprop(**okw, source_model=_lib.SOURCE_POWER_LAW)
    g, gf = obj.response_mass()
    assert g.shape == (3, M, 3, N) and np.array_equal(g, G3[0]) and np.array_equal(gf, G3f[0])
    assert not obj.evolved
    out = np.zeros((3, M, 3, N))
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(_lib.load().nusi_response_mass(obj._h, None, None, out.ctypes.data_as(dp)))   # G3 NULL, G3_fla only
    assert np.array_equal(out, G3f[0])
    assert np.array_equal(nusi.mixing(), sources.mixing(True)) and nusi.mixing(False).shape == (3, 3)
    kap = sources.mass_fractions((1, 2, 0))
    assert np.array_equal(response.compose_host(g[None], kap)[0], response.compose_host(G3[:1], kap)[0])
    print("object, pyprop and facade forms: equal bits with Plan.response_mass (worst error 0)")


def test_refusals(nusi):
    from nusiprop_amd import _lib
    grid = "G6"
    G3, G3f, _, _ = _mass(nusi, grid, True)
    plan = _plan(nusi, grid, max_points=NPT, mode="auto")
    pts = [_point(grid, k, True) for k in range(NPT)]
    for bad in (np.nan, -1.0, np.inf):
        w = np.ones(plan.Nz)
        w[2] = bad
        with pytest.raises(nusi.NusiError) as ei:
            plan.response_mass(pts, z_weight=w)
        assert ei.value.code == _lib.NUSI_EPARAM
    with pytest.raises(nusi.NusiError) as ei:
        plan.response_mass([])                                      # no points
    assert ei.value.code == _lib.NUSI_EPARAM
    for bad in (-1e-300, np.nan, np.inf):
        with pytest.raises(nusi.NusiError) as ei:
            plan.compose_response(G3, (0.3, bad, 0.3))
        assert ei.value.code == _lib.NUSI_EPARAM
    g, gf = plan.response_mass(pts)                                 # the plan stays usable
    assert np.array_equal(g, G3) and np.array_equal(gf, G3f)
    plan.close()
    print("refusals: NUSI_EPARAM for a bad weight, no points and a bad kappa; the plan's next call has equal bits")


def test_device_entry_points(nusi):
    """response_mass_device and compose_response_device on caller-owned device buffers, G3 left out (NULL)."""
    from nusiprop_amd import response
    H = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so.7")   # the HIP runtime libnusi.so itself links
    vp = ctypes.c_void_p
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    grid = "G47"
    _, G3f, _, _ = _mass(nusi, grid, True)
    plan = _plan(nusi, grid, max_points=NPT, mode="auto")
    arr = plan.params_array([_point(grid, k, True) for k in range(NPT)])
    kap = _kappas(nusi, grid, 4)
    X = int(np.prod(G3f.shape[2:]))
    out = np.zeros((NPT, 4) + G3f.shape[2:])
    dG, dO = vp(), vp()
    assert H.hipMalloc(ctypes.byref(dG), G3f.nbytes) == 0
    assert H.hipMalloc(ctypes.byref(dO), out.nbytes) == 0
    try:
        plan.response_mass_device(arr, None, dG.value)
        assert plan.compose_response_device(dG.value, G3f.shape[0], X, kap, dO.value) == 4
        assert H.hipDeviceSynchronize() == 0
        g = np.zeros_like(G3f)
        assert H.hipMemcpy(g.ctypes.data, dG, G3f.nbytes, 2) == 0
        assert H.hipMemcpy(out.ctypes.data, dO, out.nbytes, 2) == 0
    finally:
        H.hipFree(dG)
        H.hipFree(dO)
    plan.close()
    assert np.array_equal(g, G3f)
    assert np.array_equal(out, response.compose_host(G3f, kap))
    print("device forms: equal bits with the host forms (worst error 0)")
