"""The reference-order batch kernel's staged chunks on the GPU: the instance without phi-phi stages the member corners
(Dcr, Dci, A) of four points of the batch at a time in the X | mem block and runs their combines without a barrier
between them, in the full tiles two points per thread at a time (k_alpha_batch, kStage).  Every call here goes
through Plan in the reference order with NUSI_OPT_ALPHA_BATCH = 16 (the automatic cap of so small a grid is one table
per batch) and batches of >= 3 tables
(smaller calls take the k-split path, which keeps the point-by-point loop); Gamma, alphaTilde and every alpha entry
are compared bit for bit to the reference-order oracle, the fluxes to FLUX_RTOL of its evolve().

Grid: N_E = 45, lE 12 -> 12.75 (T = 91), C4's layout in small -- full, diagonal and paired tiles.  Physics:
cases.scan_points with C4's parameter ranges, two m_phi x nine couplings; one m_phi's points form one batch.
* chunk arithmetic: batches of 4 (one full chunk), 5 (4 + 1: a last chunk of one point, in the paired tiles an idle
  half), 6 (4 + 2), 8 (two full chunks), 9 (4 + 4 + 1); and 7 (4 + 3): in the full tiles a thread takes a chunk's
  points two at a time (alpha_k_two), a last odd one alone;
* a resonant-only batch of 5 (only the m = n + 1 entries computed, no corner phase);
* two batches of 6 with a member-corner block of 4 MiB, which holds fewer than the call's 12 tables: each batch gets
  a launch of its own, the second reads its corners relative to a first table pc0 = 6;
* every point of the batch of 5 alone (the k-split path) gives the same table bits.
"""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

FLUX_RTOL = cases.FLUX_RTOL
BATCH_LABEL = "k_alpha_mcorner + k_alpha_batch[refo]"
GRID = (45, 12.0, 12.75)


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


def _points(**over):
    """[m_phi index][coupling index] -> point"""
    N, lo, hi = GRID
    pts = cases.scan_points(n_mphi=2, n_g=9, N=N, lEmin=lo, lEmax=hi)
    return [[dict(p, **over) for p in pts[9 * i:9 * i + 9]] for i in range(2)]


def _run(nusi, pts, corner_mb=None):
    from nusiprop_amd import _lib
    p0 = pts[0]
    plan = nusi.Plan(p0["N_bins_E"], p0["lEmin"], p0["lEmax"], p0["zmax"], max_points=len(pts), reference_order=True)
    plan.set_option(_lib.OPT_ALPHA_BATCH, 16)
    if corner_mb is not None:
        plan.set_option(_lib.OPT_REFO_CORNER_MB, corner_mb)
    flux, fla = plan.evolve(pts)
    T, N = plan.T, plan.N
    tabs = [plan.tables(i) for i in range(len(pts))]
    names = plan.kernels()
    plan.close()
    return flux, fla, tabs, names, T, N


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
def five(nusi):
    """the batch of 5 on the grid: a full chunk and a last chunk of one point"""
    pts = _points()[0][:5]
    return (pts,) + _run(nusi, pts)


def test_batch_of_5(nusi, oracle_mod, five):
    pts, flux, fla, tabs, names, T, _ = five
    assert names[0] == BATCH_LABEL
    assert T > 45 + 8   # (the extended bins: read from the plan, 91 at zmax 5)
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


@pytest.mark.parametrize("nb", [4, 6, 7, 8, 9])
def test_chunk_arithmetic(nusi, oracle_mod, nb):
    pts = _points()[0][:nb]
    flux, fla, tabs, names, T, _ = _run(nusi, pts)
    assert names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


def test_resonant_only_batch_of_5(nusi, oracle_mod):
    pts = _points(non_resonant=False)[0][:5]
    flux, fla, tabs, names, T, _ = _run(nusi, pts)
    assert names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)


def test_two_launch_chunks_of_the_corner_block(nusi, oracle_mod):
    """Two batches of 6 under a 4 MiB member-corner block: the block holds fewer than the call's 12 tables (and at
    least one batch), so the batches go in launches of their own and the second one's tables sit at pc0 = 6."""
    g = _points()
    pts = g[0][:6] + g[1][:6]
    flux, fla, tabs, names, T, N = _run(nusi, pts, corner_mb=4)
    assert names[0] == BATCH_LABEL
    # the block per table (mcorner_ensure): 6 doubles per pair of distinct bin edges ut <= us -- the N core bins are
    # contiguous (N + 1 edges), each of the T - N redshift-extended bins has its own two
    U = N + 1 + 2 * (T - N)
    per = 8 * 6 * (U * (U + 1) // 2)
    assert 6 <= (4 << 20) // per < 12, per
    _check(nusi, oracle_mod, pts, flux, fla, tabs, T)
    # the same bits as with every table in one launch
    f1, fla1, tabs1, _, _, _ = _run(nusi, pts)
    assert np.array_equal(f1, flux) and np.array_equal(fla1, fla)
    for a, b in zip(tabs, tabs1):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


def test_batched_equals_alone(nusi, five):
    """Each point of the batch of 5 evolved alone (the k-split path of calls of few tables, every tile one point at
    a time through the point-by-point loop) gives the same table bits."""
    pts, flux, fla, tabs, names, T, _ = five
    for k, kw in enumerate(pts):
        _, _, t1, n1, _, _ = _run(nusi, [kw])
        assert n1[0] == BATCH_LABEL
        for a, b in zip(tabs[k], t1[0]):
            assert np.array_equal(a, b), k
