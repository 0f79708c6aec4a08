"""User-tabulated sources (NUSI_SOURCE_TABULATED + slot; nusi_plan_set_source, k_source_tab) on the GPU.

Every yardstick is the oracle's own power-law run (reference_order(1), the library default): a power law put through
the table is the power-law source again, and the flux is linear in the source, so sums of power laws have known
fluxes.  Oracle.prepare() returns norm_total = norm / flux_FS_E0(gamma), so fs(gamma) = 1 / norm_total at norm = 1
comes from the oracle itself; a tabulated point's norm is absolute, so S = power_law_integrals(gamma) with
norm = 1 / fs(gamma) is the power law of norm 1.

Tolerance: cases.FLUX_RTOL (the project's bound for summation-order differences).  The source terms formed from
power_law_integrals on the source axis differ from the direct power-law expression by <= 4.0e-13 relative (the
cancellation on a 4 % bin; numpy, grids up to N_E = 300, gamma in {2, 2.5, 3}), and the flux is a non-negative
combination of those terms.

The points are strongly interacting (fluxes between 1e-6 and 8 % of free streaming in some bin), so equivalence is
not vacuous.  The grids are the smallest that reach each cascade instance:
  G6   N_E = 37, lE 12 -> 17:     6 steps   k_cascade_bs<16, ...>, the source table read a block ahead
  G32  N_E = 200, lE 12 -> 17:    32 steps  <32, ...>
  G47  N_E = 45, lE 12 -> 12.75:  47 steps  <48, ...>, the gamma batch's 6-step passes
  G63  N_E = 60, lE 12 -> 12.75:  63 steps  two 48-step passes; with OPT_STEP_PASSES = 1 the 16-step instance
"""
import ctypes

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

GRIDS = {"G6": (37, 12.0, 17.0), "G32": (200, 12.0, 17.0), "G47": (45, 12.0, 12.75), "G63": (60, 12.0, 12.75)}
STEPS = {"G6": 6, "G32": 32, "G47": 47, "G63": 63}
PHYS = [(1e7, 0.5), (10 ** 6.5, 0.178)]
GAMMAS = (2.0, 3.0)


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


def _pt(grid, k, nonres, **over):
    N, lo, hi = GRIDS[grid]
    m, g = PHYS[k]
    p = dict(mphi=m, g=g, mntot=0.1, si=2.0, norm=1.0, majorana=True, non_resonant=nonres, normal_ordering=True,
             N_bins_E=N, lEmin=lo, lEmax=hi, zmax=5.0, flav=2, phiphi=False, source_model=1)
    p.update(over)
    return p


_ORACLE = {}


@pytest.fixture(scope="module")
def oracle_pl(oracle_mod):
    """(flux, flux_fla, fs) of the oracle's power-law run at norm = 1, computed once per (grid, point, mode, gamma)."""
    def get(grid, k, nonres, si, **over):
        key = (grid, k, nonres, si, tuple(sorted(over.items())))
        if key not in _ORACLE:
            with oracle_mod.reference_order(1):
                o = oracle_mod.Oracle(**cases.oracle_kwargs(_pt(grid, k, nonres, si=si, **over)))
                _, nt = o.prepare()
                f, fl = o.evolve()
            assert np.all(np.isfinite(f)) and np.all(f >= 0) and np.any(f > 0)
            f.setflags(write=False)
            fl.setflags(write=False)
            _ORACLE[key] = (f, fl, 1.0 / nt)
        return _ORACLE[key]
    return get


def _plan(nusi, grid, max_points=16, mode="one"):
    from nusiprop_amd import _lib
    N, lo, hi = GRIDS[grid]
    plan = nusi.Plan(N, lo, hi, 5.0, max_points=max_points)
    assert plan.Nz - 1 == STEPS[grid]
    if mode == "one":          # one point per MFMA-cascade workgroup: the instance the grid is chosen for
        plan.set_option(_lib.OPT_CASCADE_RHS, 1)
    elif mode == "scalar":
        plan.set_cascade(_lib.CASCADE_WAVEFRONT)
    elif mode == "passes":
        plan.set_option(_lib.OPT_STEP_PASSES, 1)
    else:
        assert mode == "auto"  # the points of a table in one workgroup (the gamma batch, pairs)
    return plan


def _S(plan, si):
    from nusiprop_amd import sources
    lo, hi, _ = plan.source_axis()
    return sources.power_law_integrals(lo, hi, si)


def _sfr(z):
    """get_SFR (nuSIprop.hpp:591-605) restated with the host libm's pow (Python floats), on the plan's z."""
    return np.array([((1 + v) ** (-3.4 * 10) + ((1 + v) / 5161) ** (0.3 * 10) + ((1 + v) / 9.06) ** (3.5 * 10)) ** (-1. / 10.)
                     for v in map(float, z)])


def _err(flux, fla, ref_flux, ref_fla):
    return max(cases.rel_err(flux, ref_flux), cases.rel_err(fla, ref_fla))


def test_source_axis(nusi):
    plan = _plan(nusi, "G6")
    lo, hi, z = plan.source_axis()
    N, Nz = plan.N, plan.Nz
    assert len(lo) == len(hi) == N + Nz - 1 and len(z) == Nz and z[0] == 0.0
    e = np.array([10.0 ** (12.0 + 5.0 * (i * 1.0) / N) for i in range(N + 1)])   # (Python floats: the host libm's pow)
    assert np.array_equal(lo[:N], e[:-1]) and np.array_equal(hi[:N], e[1:])
    assert np.allclose(np.sqrt(lo[:N] * hi[:N]), plan.energies, rtol=1e-14)
    for j in range(1, Nz):
        assert lo[N - 1 + j] == lo[N - 1] * (1 + z[j]) and hi[N - 1 + j] == hi[N - 1] * (1 + z[j])
    plan.close()


# --- 1. a power law through the table ---------------------------------------------------------------------------
CASES_1 = [(g, m) for g in GRIDS for m in ("one", "auto", "scalar")] + [("G63", "passes")]


@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid,mode", CASES_1)
def test_power_law_through_table(nusi, oracle_pl, grid, mode, nonres):
    from nusiprop_amd import sources
    plan = _plan(nusi, grid, mode=mode)
    for s, si in enumerate(GAMMAS):
        plan.set_source(s, _S(plan, si))
    pts, refs = [], []
    for k in range(len(PHYS)):
        for s, si in enumerate(GAMMAS):
            f, fl, fs = oracle_pl(grid, k, nonres, si)
            pts.append(_pt(grid, k, nonres, si=7.5, norm=1.0 / fs, source_model=sources.tabulated(s)))   # (si is ignored)
            pts.append(_pt(grid, k, nonres, si=si))
            refs.append((f, fl))
    flux, fla = plan.evolve(pts)
    name = plan.kernels()[1]
    assert name == {"one": "k_cascade_bs", "passes": "k_cascade_bs", "auto": "k_cascade_bs_gamma",
                    "scalar": "k_cascade"}[mode], name
    worst = 0.0
    for j, (f, fl) in enumerate(refs):
        e_or = _err(flux[2 * j], fla[2 * j], f, fl)                     # the tabulated point vs the oracle's power law
        e_pl = _err(flux[2 * j], fla[2 * j], flux[2 * j + 1], fla[2 * j + 1])   # ... vs the plan's own power-law point
        print("%s %s nonres=%d point %d: vs oracle %.2e, vs source_model=1 %.2e" % (grid, mode, nonres, j, e_or, e_pl))
        worst = max(worst, e_or, e_pl)
    plan.close()
    assert worst <= cases.FLUX_RTOL, worst


# --- 2. a spectrum that is not a power law -------------------------------------------------------------------------
def _mix_expected(oracle_pl, grid, k, nonres):
    f2, fl2, fs2 = oracle_pl(grid, k, nonres, 2.0)
    f3, fl3, fs3 = oracle_pl(grid, k, nonres, 3.0)
    return 1.0 * fs2 * f2 + 0.5 * fs3 * f3, 1.0 * fs2 * fl2 + 0.5 * fs3 * fl3


@pytest.mark.parametrize("nonres", [True, False], ids=["nonres", "resonant"])
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_sum_of_power_laws(nusi, oracle_pl, grid, nonres):
    from nusiprop_amd import sources
    plan = _plan(nusi, grid)
    plan.set_source(0, 1.0 * _S(plan, 2.0) + 0.5 * _S(plan, 3.0))
    flux, fla = plan.evolve([_pt(grid, k, nonres, source_model=sources.tabulated(0)) for k in range(len(PHYS))])
    plan.close()
    worst = 0.0
    for k in range(len(PHYS)):
        ef, efl = _mix_expected(oracle_pl, grid, k, nonres)
        e = _err(flux[k], fla[k], ef, efl)
        print("%s nonres=%d point %d: S2 + 0.5 S3 vs the oracle's combination %.2e" % (grid, nonres, k, e))
        worst = max(worst, e)
    assert worst <= cases.FLUX_RTOL, worst


# --- 3. redshift weights -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_redshift_weights(nusi, oracle_pl, grid):
    from nusiprop_amd import sources
    plan = _plan(nusi, grid)
    _, _, z = plan.source_axis()
    S, sfr = _S(plan, 2.0), _sfr(z)
    f, fl, fs = oracle_pl(grid, 0, True, 2.0)
    pt = [_pt(grid, 0, True, norm=1.0 / fs, source_model=sources.tabulated(0))]
    plan.set_source(0, S)
    f0, fl0 = plan.evolve(pt)
    plan.set_source(0, S, sfr)                      # the star-formation rate passed explicitly: the same bits
    f1, fl1 = plan.evolve(pt)
    assert np.array_equal(f0, f1) and np.array_equal(fl0, fl1)
    plan.set_source(0, S, lambda v: 2.0 * _sfr([v])[0])   # twice the weight (a callable): twice the power law's flux
    f2, fl2 = plan.evolve(pt)
    e = _err(f2[0], fl2[0], 2.0 * f, 2.0 * fl)
    print("%s: w = 2 SFR vs twice the oracle's power law %.2e" % (grid, e))
    assert e <= cases.FLUX_RTOL, e
    # one step only, and a spectrum that ends at source-axis bin n_top: step i0 feeds the bins b <= n_top - i0
    N, Nz = plan.N, plan.Nz
    i0, n_top = Nz // 2, N // 2 + Nz // 2
    w = np.zeros(Nz)
    w[i0] = sfr[i0]
    St = np.where(np.arange(len(S)) <= n_top, S, 0.0)
    plan.set_source(0, St, w)
    for nonres in (True, False):
        f3, fl3 = plan.evolve([dict(pt[0], non_resonant=nonres)])
        b_top = n_top - i0
        assert np.all(f3[0][:, b_top + 1:] == 0.0) and np.all(fl3[0][:, b_top + 1:] == 0.0)
        assert np.all(f3[0][:, :b_top + 1] > 0.0) and np.all(np.isfinite(f3[0]))
    plan.close()


# --- 4. mixed groups sharing one table -----------------------------------------------------------------------------
def test_mixed_groups_share_one_table(nusi, oracle_pl):
    from nusiprop_amd import _lib, sources
    grid = "G47"
    plan = _plan(nusi, grid, mode="auto")
    plan.set_source(0, 1.0 * _S(plan, 2.0) + 0.5 * _S(plan, 3.0))
    plan.set_source(1, _S(plan, 2.5), lambda v: (1.0 + v) ** 1.5)
    pts = [_pt(grid, 0, True, si=2.5),                                              # power law
           _pt(grid, 0, True, source_model=0),                                      # DSNB
           _pt(grid, 0, True, norm=3.0, source_model=sources.tabulated(0)),         # two points on one slot ...
           _pt(grid, 0, True, norm=0.25, flav=0, source_model=sources.tabulated(0)),   # (another flavour: its own table)
           _pt(grid, 0, True, source_model=sources.tabulated(1))]                   # ... and one on a second slot
    flux, fla = plan.evolve(pts)
    assert "k_cascade_bs_gamma" in plan.kernels()[1], plan.kernels()
    f2, fl2 = plan.evolve(pts[1:3])                                                  # a pair: DSNB + tabulated
    assert "k_cascade_bs_pairs" in plan.kernels()[1], plan.kernels()
    plan.set_option(_lib.OPT_CASCADE_RHS, 1)
    alone = [plan.evolve([p]) for p in pts]
    assert plan.kernels()[1] == "k_cascade_bs"
    plan.close()
    for j, (fa, fla_a) in enumerate(alone):
        e = _err(flux[j], fla[j], fa[0], fla_a[0])
        print("mixed call, point %d vs alone: %.2e" % (j, e))
        assert e <= 1e-13, (j, e)            # DESIGN sec. 2 "Batching and rounding"
    for j in (1, 2):
        e = _err(f2[j - 1], fl2[j - 1], alone[j][0][0], alone[j][1][0])
        print("pair, point %d vs alone: %.2e" % (j, e))
        assert e <= 1e-13, (j, e)
    assert np.any(alone[2][0] > 0) and np.any(alone[4][0] > 0)
    f, fl, _ = oracle_pl(grid, 0, True, 2.5)
    e = _err(flux[0], fla[0], f, fl)
    print("mixed call, the power-law point vs the oracle: %.2e" % e)
    assert e <= cases.FLUX_RTOL, e


# --- 5. scalar vs MFMA ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["G6", "G47"])
def test_scalar_and_mfma_agree(nusi, grid):
    from nusiprop_amd import sources
    out = {}
    for mode in ("one", "scalar"):
        plan = _plan(nusi, grid, mode=mode)
        plan.set_source(0, 1.0 * _S(plan, 2.0) + 0.5 * _S(plan, 3.0))
        pts = [_pt(grid, k, nr, source_model=sources.tabulated(0)) for k in range(len(PHYS)) for nr in (True, False)]
        out[mode] = plan.evolve(pts)
        if mode == "scalar":
            again = plan.evolve(pts)
            assert plan.kernels()[1] == "k_cascade"
            assert np.array_equal(again[0], out[mode][0]) and np.array_equal(again[1], out[mode][1])
        plan.close()
    e = _err(out["one"][0], out["one"][1], out["scalar"][0], out["scalar"][1])
    print("%s: MFMA vs scalar cascade on S2 + 0.5 S3: %.2e" % (grid, e))
    assert np.any(out["scalar"][0] > 0)
    assert e <= cases.FLUX_RTOL, e


# --- 6. surfaces ---------------------------------------------------------------------------------------------------
def test_object_api_and_pyprop(nusi):
    from nusiprop_amd import _lib, sources
    grid = "G6"
    N, lo, hi = GRIDS[grid]
    kw = _pt(grid, 0, True, si=2.5, norm=2.0)
    plan = _plan(nusi, grid, max_points=1, mode="auto")
    alo, ahi, z = plan.source_axis()
    fn = sources.broken_power_law(2.0, 3.0, 1e15)
    S, w = sources.bin_integrals(fn, alo, ahi), np.array([(1.0 + float(v)) ** 2 for v in z])
    plan.set_source(0, S, w)
    pf, pfl = plan.evolve([dict(kw, source_model=sources.tabulated(0))])
    plan.set_source(0, fn, lambda v: (1.0 + v) ** 2)          # the callable forms: the same vectors, the same bits
    cf, cfl = plan.evolve([dict(kw, source_model=sources.tabulated(0))])
    assert np.array_equal(cf, pf) and np.array_equal(cfl, pfl)
    plf, plfl = plan.evolve([kw])                               # the constructor's source (the power law)
    plan.close()
    assert np.any(pf > 0) and not np.array_equal(pf, plf)

    okw = {k: v for k, v in kw.items() if k != "source_model"}
    obj = nusi.pyprop(**okw, source_model=_lib.SOURCE_POWER_LAW)
    olo, ohi, oz = obj.source_axis()
    assert np.array_equal(olo, alo) and np.array_equal(ohi, ahi) and np.array_equal(oz, z)
    obj.evolve()
    assert np.array_equal(obj.get_flux(), plf[0]) and np.array_equal(obj.get_flux_fla(), plfl[0])
    obj.set_source(S, w)
    assert not obj.evolved
    obj.evolve()
    assert np.array_equal(obj.get_flux(), pf[0]) and np.array_equal(obj.get_flux_fla(), pfl[0])
    with pytest.raises(nusi.NusiError) as ei:                   # no free-streaming energy for a tabulated spectrum
        obj.check_energy_conservation()
    assert ei.value.code == _lib.NUSI_EPARAM and "tabulated" in str(ei.value)
    # a copy keeps the source (and evolves it on its own plan)
    L = _lib.load()
    h2 = ctypes.c_void_p()
    _lib.check(L.nusi_copy(obj._h, ctypes.byref(h2)))
    try:
        _lib.check(L.nusi_evolve(h2))
        out = np.zeros((3, N))
        _lib.check(L.nusi_get_flux(h2, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        assert np.array_equal(out, pf[0])
        _lib.check(L.nusi_set_source(h2, None, None))           # ... and the constructor's source to return to
        _lib.check(L.nusi_evolve(h2))
        _lib.check(L.nusi_get_flux(h2, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
        assert np.array_equal(out, plf[0])
    finally:
        L.nusi_destroy(h2)
    obj.set_source(None)                                         # back to the constructor's source, bit for bit
    obj.evolve()
    assert np.array_equal(obj.get_flux(), plf[0]) and np.array_equal(obj.get_flux_fla(), plfl[0])
    assert np.isfinite(obj.check_energy_conservation())


# --- 7. errors, slots ----------------------------------------------------------------------------------------------
def _refused(fn, code):
    from nusiprop_amd import NusiError
    with pytest.raises(NusiError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))


def test_errors_leave_the_plan_usable(nusi):
    from nusiprop_amd import _lib, sources
    grid = "G6"
    plan = _plan(nusi, grid, max_points=2)
    S = _S(plan, 2.5)
    _, _, z = plan.source_axis()
    tab0 = _pt(grid, 0, True, source_model=sources.tabulated(0))
    _refused(lambda: plan.evolve([tab0]), _lib.NUSI_EPARAM)                     # an empty slot (nothing registered)
    plan.set_source(0, S)
    good = plan.evolve([tab0])
    _refused(lambda: plan.evolve([dict(tab0, source_model=sources.tabulated(3))]), _lib.NUSI_EPARAM)   # empty, in storage
    _refused(lambda: plan.evolve([dict(tab0, source_model=sources.tabulated(5000))]), _lib.NUSI_EPARAM)   # ... beyond it
    _refused(lambda: plan.set_source(-1, S), _lib.NUSI_EPARAM)                  # slots out of range
    _refused(lambda: plan.set_source(_lib.SOURCE_SLOTS_MAX, S), _lib.NUSI_EPARAM)
    for k, bad in ((1, np.nan), (len(S) - 1, -1e-300), (2, np.inf)):
        Sb = S.copy()
        Sb[k] = bad
        _refused(lambda: plan.set_source(0, Sb), _lib.NUSI_EPARAM)
    for bad in (np.nan, -1.0):
        wb = np.ones(len(z))
        wb[-1] = bad
        _refused(lambda: plan.set_source(0, S, wb), _lib.NUSI_EPARAM)
    again = plan.evolve([tab0])                                                  # slot 0 kept its source throughout
    assert np.array_equal(again[0], good[0]) and np.array_equal(again[1], good[1])
    # at least 1024 slots, the storage grown on demand (slot 0 survives the growth)
    plan.set_source(1023, S)
    both = plan.evolve([tab0, dict(tab0, source_model=sources.tabulated(1023))])
    assert np.array_equal(both[0][0], both[0][1]) and np.array_equal(both[1][0], both[1][1])
    plan.set_source(1023, None)                                                  # cleared: empty again
    _refused(lambda: plan.evolve([dict(tab0, source_model=sources.tabulated(1023))]), _lib.NUSI_EPARAM)
    assert np.array_equal(plan.evolve([tab0])[0], good[0])
    plan.close()


def test_replacing_a_slot_affects_later_calls_only(nusi):
    """The first call's device buffers are read only after the slot was replaced and the second call ran."""
    from nusiprop_amd import sources
    # the HIP runtime libnusi.so itself links, for the device buffers (tests/test_gpu_parity.py's _hip: torch's
    # separately bundled runtime must not be initialised after libnusi's)
    H = ctypes.CDLL("/opt/rocm/lib/libamdhip64.so.7")
    vp = ctypes.c_void_p
    H.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
    H.hipFree.argtypes = [vp]
    H.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
    grid = "G47"
    plan = _plan(nusi, grid, max_points=1)
    S = _S(plan, 2.5)
    arr = plan.params_array([_pt(grid, 0, True, source_model=sources.tabulated(0))])
    plan.set_source(0, S)
    want, _ = plan.evolve(arr)
    nb = 3 * plan.N * 8
    bufs = [vp() for _ in range(4)]          # flux, flux_fla of the first call; of the second
    for d in bufs:
        assert H.hipMalloc(ctypes.byref(d), nb) == 0
    try:
        plan.evolve_device(arr, bufs[0].value, bufs[1].value)
        plan.set_source(0, 2.0 * S)
        plan.evolve_device(arr, bufs[2].value, bufs[3].value)
        plan.stage_ms()                       # (synchronises the plan's stream)
        host = [np.zeros((3, plan.N)) for _ in bufs]
        for h, d in zip(host, bufs):
            assert H.hipMemcpy(h.ctypes.data, d, nb, 2) == 0
    finally:
        for d in bufs:
            H.hipFree(d)
    fa, fb = host[0:2], host[2:4]
    plan.close()
    assert np.array_equal(fa[0], want[0]) and np.any(fa[0] > 0)
    assert cases.rel_err(fb[0], 2.0 * fa[0]) <= cases.FLUX_RTOL and cases.rel_err(fb[1], 2.0 * fa[1]) <= cases.FLUX_RTOL
