"""The reference-order batch kernel's partly filled tiles on the GPU: tiles of at most 128 entries run two points of
the batch per iteration of the point loop (AlphaTile::pair in k_alpha_batch), and the redshift-extended bins are cut into runs of 8
from the first extended bin (nusi_alpha_tiles.hpp).  Every call here goes through Plan in the reference order with
batches of >= 3 tables (NUSI_OPT_ALPHA_BATCH = 8: the automatic cap of so small a grid is one table per batch); Gamma,
alphaTilde and every alpha entry are compared bit for bit to the reference-order oracle, the fluxes to FLUX_RTOL of its
evolve().

Grids (physics: cases.scan_points with C4's parameter ranges, two m_phi x seven couplings):
* N_E = 45, lE 12 -> 12.75 (T = 91): C4's layout in small -- core rows, 46 extended bins in runs 8, 8, 8, 8, 8, 6;
  batches of 3 and 4 (an idle half in the last pair; a whole number of pairs), a batch of 7 (pairs across the chunk
  boundary of 4 points, an odd batch), a resonant-only batch of 3 (only m = n + 1 entries computed);
* N_E = 40, lE 12 -> 12.8 (T = 78): the core / extended boundary inside a tile, the per-table classes 1 and 2 beside
  the batched tiles; a batch of 5;
* N_E = 31, lE 12 -> 12.5 (T = 79): 49 extended bins, the last run a remainder of one bin; a batch of 3.
"""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

FLUX_RTOL = cases.FLUX_RTOL
BATCH_LABEL = "k_alpha_mcorner + k_alpha_batch[refo]"
GRIDS = {"c4small": (45, 12.0, 12.75), "inside": (40, 12.0, 12.8), "remainder": (31, 12.0, 12.5)}


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


def _points(grid, **over):
    """[m_phi index][coupling index] -> point, on a grid of GRIDS"""
    N, lo, hi = GRIDS[grid]
    pts = cases.scan_points(n_mphi=2, n_g=7, N=N, lEmin=lo, lEmax=hi)
    return [[dict(p, **over) for p in pts[7 * i:7 * i + 7]] for i in range(2)]


def _run(nusi, pts):
    from nusiprop_amd import _lib
    p0 = pts[0]
    plan = nusi.Plan(p0["N_bins_E"], p0["lEmin"], p0["lEmax"], p0["zmax"], max_points=len(pts), reference_order=True)
    plan.set_option(_lib.OPT_ALPHA_BATCH, 8)
    flux, fla = plan.evolve(pts)
    T = plan.T
    tabs = [plan.tables(i) for i in range(len(pts))]
    names = plan.kernels()
    plan.close()
    return flux, fla, tabs, names, T


_ref_cache = {}


def _reference(oracle_mod, kw):
    """(Gamma, alphaTilde, alpha, flux, flux_fla, T) of the reference-order oracle, computed once per point"""
    key = tuple(sorted(kw.items()))
    if key not in _ref_cache:
        o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
        with oracle_mod.reference_order(1):
            G, aT, al = o.tables()
            f, fl = o.cascade(G, aT, al)
        for a in (G, aT, al, f, fl):
            a.setflags(write=False)
        _ref_cache[key] = (G, aT, al, f, fl, o.T)
    return _ref_cache[key]


def _check(nusi, oracle_mod, pts, flux, fla, tabs, T):
    iu = np.triu_indices(T, 1)
    for k, kw in enumerate(pts):
        G, aT, al, f_ref, fla_ref, To = _reference(oracle_mod, kw)
        assert To == T
        Gg, aTg, Ag = tabs[k]
        assert np.array_equal(Gg, G), (k, "Gamma differs at %s" % np.flatnonzero(Gg != G)[:5])
        assert np.array_equal(aTg, aT), (k, "alphaTilde differs at %s" % np.flatnonzero(aTg != aT)[:5])
        Ad = nusi.unpack_alpha(Ag, T)
        if kw["non_resonant"]:
            bad = np.flatnonzero(Ad[iu] != al[iu])
            assert bad.size == 0, (k, "alpha differs in %d entries, first (n, m) = (%d, %d)"
                                   % (bad.size, iu[0][bad[0]], iu[1][bad[0]]))
        else:   # the resonant-only table: its m = n + 1 entries, 0.0 elsewhere
            d = np.arange(T - 1)
            assert np.array_equal(Ad[d, d + 1], al[d, d + 1]), k
            off = np.ones((T, T), bool)
            off[d, d + 1] = False
            assert not np.any(Ad[off]), k
        assert cases.rel_err(flux[k], f_ref) <= FLUX_RTOL, k
        assert cases.rel_err(fla[k], fla_ref) <= FLUX_RTOL, k


@pytest.fixture(scope="module")
def seven(nusi):
    """the 7-table call on the C4-like grid: batches of 3 and 4"""
    g = _points("c4small")
    pts = g[0][:3] + g[1][:4]
    return (pts,) + _run(nusi, pts)


def test_batches_of_3_and_4(nusi, oracle_mod, seven):
    pts, flux, fla, tabs, names, T = seven
    assert names[0] == BATCH_LABEL
    assert T > 45 + 8   # (the extended bins: read from the plan, 91 at zmax 5)
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


def test_batch_of_7(nusi, oracle_mod):
    pts = _points("c4small")[0]
    flux, fla, tabs, names, T = _run(nusi, pts)
    assert names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


def test_boundary_inside_tile_batch_of_5(nusi, oracle_mod):
    pts = _points("inside")[0][:5]
    flux, fla, tabs, names, T = _run(nusi, pts)
    assert names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


def test_short_remainder_batch_of_3(nusi, oracle_mod):
    pts = _points("remainder")[1][:3]
    flux, fla, tabs, names, T = _run(nusi, pts)
    assert names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


def test_resonant_only_batch_of_3(nusi, oracle_mod):
    pts = _points("c4small", non_resonant=False)[0][:3]
    flux, fla, tabs, names, T = _run(nusi, pts)
    assert names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


def test_batched_equals_alone(nusi, seven):
    """Each point of the 7-table call evolved alone (the k-split path of calls of few tables, every tile one point
    at a time) gives the same table bits."""
    pts, flux, fla, tabs, names, T = seven
    for k, kw in enumerate(pts):
        _, _, t1, n1, _ = _run(nusi, [kw])
        assert n1[0] == BATCH_LABEL
        for a, b in zip(tabs[k], t1[0]):
            assert np.array_equal(a, b), k
