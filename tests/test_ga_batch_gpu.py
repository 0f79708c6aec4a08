"""Gamma / alphaTilde's batch path on the GPU (NUSI_OPT_GA_BATCH): k_ga_dilogs_batch evaluates the reference order's
GSL dilogarithms per alpha batch -- the values that do not read the coupling once per batch, the others with the
batch's tables on neighbouring lanes -- and k_gamma_alphat<true, 1, true> combines them.

Grid: N_E = 45, lE 12 -> 12.75 (T = 91: the core bins share edges, the 46 redshift-extended bins do not).  Every
call goes through Plan in the reference order with NUSI_OPT_ALPHA_BATCH = 16 and, unless stated, NUSI_OPT_GA_BATCH = 2
(the batch path also for calls of at most 16 tables).  Every case asserts Gamma and alphaTilde bit-equal to the
reference-order oracle's tables, Gamma, alphaTilde and alpha bit-equal to the same call on the per-table kernel
(NUSI_OPT_GA_BATCH = 1), equal per-point warnings, the fluxes within FLUX_RTOL of the oracle, and the path query.

The flux assertion is dropped where the oracle's own flux is NaN or has diverged (group E of
cases.mixed_batch_groups: its five points are the couplings of index 0 .. 4, whose oracle fluxes are checked here for
being finite first; a point with a non-finite or > 1e200 oracle flux keeps its table and warning assertions only).
"""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

FLUX_RTOL = cases.FLUX_RTOL
BATCH_PATH = "k_ga_dilogs_batch + k_gamma_alphat[pre]"
GRID = (45, 12.0, 12.75)


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


def _scan():
    """[m_phi index][coupling index] -> point"""
    N, lo, hi = GRID
    pts = cases.scan_points(n_mphi=2, n_g=9, N=N, lEmin=lo, lEmax=hi)
    return [pts[9 * i:9 * i + 9] for i in range(2)]


def _run(nusi, pts, ga_batch=2, pre_kb=None):
    from nusiprop_amd import _lib
    p0 = pts[0]
    plan = nusi.Plan(p0["N_bins_E"], p0["lEmin"], p0["lEmax"], p0["zmax"], max_points=len(pts), reference_order=True)
    plan.set_option(_lib.OPT_ALPHA_BATCH, 16)
    plan.set_option(_lib.OPT_GA_BATCH, ga_batch)
    if pre_kb is not None:
        plan.set_option(_lib.OPT_GA_PRE_KB, pre_kb)
    flux, fla = plan.evolve(pts)
    T, N = plan.T, plan.N
    tabs = [plan.tables(i) for i in range(len(pts))]
    warn = plan.warnings(len(pts))
    path = plan.ga_kernel()
    plan.close()
    return dict(flux=flux, fla=fla, tabs=tabs, warn=warn, path=path, T=T, N=N)


_ref_cache = {}


def _reference(oracle_mod, kw):
    """(Gamma, alphaTilde, flux, flux_fla, T) of the reference-order oracle, computed once per point"""
    key = tuple(sorted(kw.items()))
    if key not in _ref_cache:
        o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
        with oracle_mod.reference_order(1), np.errstate(all="ignore"):
            G, aT, al = o.tables()
            f, fl = o.cascade(G, aT, al)
        for a in (G, aT, f, fl):
            a.setflags(write=False)
        _ref_cache[key] = (G, aT, f, fl, o.T)
    return _ref_cache[key]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _check(nusi, oracle_mod, pts, r, expect_path=BATCH_PATH):
    """r (the batch path's run) against the oracle and against the per-table kernel on the same call"""
    assert r["path"] == expect_path
    r1 = _run(nusi, pts, ga_batch=1)
    assert r1["path"] != BATCH_PATH
    assert r["warn"] == r1["warn"]
    for k, kw in enumerate(pts):
        G, aT, f_ref, fla_ref, To = _reference(oracle_mod, kw)
        assert To == r["T"]
        Gg, aTg, Ag = r["tabs"][k]
        assert np.array_equal(Gg, G), (k, "Gamma differs at %s" % np.flatnonzero(Gg != G)[:5])
        assert np.array_equal(aTg, aT), (k, "alphaTilde differs at %s" % np.flatnonzero(aTg != aT)[:5])
        for a, b, what in zip(r["tabs"][k], r1["tabs"][k], ("Gamma", "alphaTilde", "alpha")):
            assert np.array_equal(_bits(a), _bits(b)), (k, what + " differs from the per-table kernel's")
        finite = np.all(np.isfinite(f_ref)) and np.all(np.isfinite(fla_ref)) and np.max(np.abs(f_ref)) < 1e200
        if finite:
            assert cases.rel_err(r["flux"][k], f_ref) <= FLUX_RTOL, k
            assert cases.rel_err(r["fla"][k], fla_ref) <= FLUX_RTOL, k
        else:   # (group E: the oracle's own flux is NaN or has diverged; tables and warnings are asserted above)
            assert kw["mntot"] == cases.MSUM_MIN_NO, (k, "only group E's oracle fluxes may be non-finite")


@pytest.mark.parametrize("nb", [1, 2, 5, 9])
def test_batch_size(nusi, oracle_mod, nb):
    """one batch of nb tables (one m_phi): nb not dividing 64, and a lone table"""
    pts = _scan()[0][:nb]
    _check(nusi, oracle_mod, pts, _run(nusi, pts))


def test_two_batches_of_different_size(nusi, oracle_mod):
    g = _scan()
    pts = g[0][:9] + g[1][:4]
    _check(nusi, oracle_mod, pts, _run(nusi, pts))


def _mixed():
    groups = cases.mixed_batch_groups()
    pts = [p for name in sorted(groups) for p in groups[name]]
    order = np.random.default_rng(11).permutation(len(pts))
    return groups, [pts[i] for i in order]


def test_mixed_groups_in_one_call_take_the_auto_path(nusi, oracle_mod):
    """Dirac, inverted ordering, resonant-only, the nearly massless lightest state and m_phi = 1e8 shuffled into one
    call of 33 tables: more than 16 tables, so the automatic rule takes the batch path"""
    _, pts = _mixed()
    assert len(pts) == 33
    _check(nusi, oracle_mod, pts, _run(nusi, pts, ga_batch=0))


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "Dp", "E", "F"])
def test_mixed_group_alone(nusi, oracle_mod, name):
    pts = cases.mixed_batch_groups()[name]
    _check(nusi, oracle_mod, pts, _run(nusi, pts))


def test_chunks_of_the_value_block(nusi, oracle_mod):
    """9 + 4 tables under a block budget that holds the batch of 9 but not both batches (the budget in KiB: a batch
    of this grid takes 230 KiB, and NUSI_OPT_GA_PRE_MB counts whole MiB), so each batch gets a producer and a consumer
    launch of its own, the second one's tables at pc0 = 9.  The same bits as in one launch."""
    g = _scan()
    pts = g[0][:9] + g[1][:4]
    T, N = 91, GRID[0]
    U = N + 1 + 2 * (T - N)   # distinct edges: the core's N + 1, two per extended bin
    per_table = 8 * 3 * 4 * (U + T) + 4        # the values that read the coupling, and the table's batch number
    per_batch = 8 * 3 * (6 * U + 8 * T)        # the batch's shared values
    kb = -(-(9 * per_table + per_batch) // 1024)
    assert 9 * per_table + per_batch <= (kb << 10) < 13 * per_table + 2 * per_batch, (per_table, per_batch)
    r = _run(nusi, pts, pre_kb=kb)
    assert r["T"] == T
    _check(nusi, oracle_mod, pts, r)
    r1 = _run(nusi, pts)
    assert np.array_equal(_bits(r1["flux"]), _bits(r["flux"])) and np.array_equal(_bits(r1["fla"]), _bits(r["fla"]))
    for a, b in zip(r["tabs"], r1["tabs"]):
        for x, y in zip(a, b):
            assert np.array_equal(_bits(x), _bits(y))


def test_auto_rule(nusi):
    """The measured cut-over: the batch path won at every batch size, batches of one table
    included, so the automatic rule is the table count alone -- a call of at most 16 tables, below the cut-over, keeps
    the few-table path (one value per work-item, Gamma / alphaTilde beside alpha), 18 tables take the batch path even
    in batches of at most 2; the other alpha kernel kinds and the shared order, which form no such batches or read no
    GSL values, keep the per-table kernel."""
    from nusiprop_amd import _lib
    g = _scan()
    pts = g[0] + g[1]
    plan = nusi.Plan(*GRID, pts[0]["zmax"], max_points=len(pts), reference_order=True)
    plan.set_option(_lib.OPT_ALPHA_BATCH, 16)
    plan.evolve(pts[:16])
    assert plan.ga_kernel() == "k_ga_dilogs + k_gamma_alphat[pre]"
    plan.evolve(pts)
    assert plan.ga_kernel() == BATCH_PATH
    plan.set_option(_lib.OPT_ALPHA_BATCH, 2)
    plan.evolve(pts)
    assert plan.ga_kernel() == BATCH_PATH
    plan.set_option(_lib.OPT_ALPHA_KERNEL, 2)
    plan.evolve(pts)
    assert plan.ga_kernel() == "k_gamma_alphat"
    plan.set_option(_lib.OPT_ALPHA_KERNEL, 0)
    plan.set_option(_lib.OPT_REFERENCE_ORDER, 0)
    plan.evolve(pts)
    assert plan.ga_kernel() == "k_gamma_alphat"
    plan.close()
