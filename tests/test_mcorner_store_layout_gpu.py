"""k_alpha_mcorner's stores of a workgroup's (Dcr, Dci) pairs on scans, with the (table, corner) of each pair stepped
from one division per work-item: batches large enough that a work-item stores more than once, with a step that is no
multiple of the corners per workgroup, give the tables of each point evolved alone, bit for bit.

The stepped loop runs only when a launch chunk has more than 256 jobs per workgroup, and its steps (dq, dr, the wrap)
matter only from a work-item's second store on.  launch_alpha sizes the workgroups from the chunk: jobs = 256 max(1,
min(4, 3 NC ntb / (2048 x 256))), cb = jobs / nb corners per workgroup.  On the C4 grid (N_E = 300, lE 12 -> 17: NC =
77 421 corners) one batch of
*  6 tables has jobs =  512, cb =  85: two stores per work-item, a step of 256 pairs = 3 tables + 1 corner;
*  7 tables has jobs =  768, cb = 109: three stores, a step of 2 tables + 38 corners;
* 11 tables has jobs = 1024, cb =  93: four stores, a step of 2 tables + 70 corners.
In each the corner index wraps in some lanes and not in others in the same iteration, and NC is no multiple of cb, so
the last workgroup is partly outside the axis.  These figures are computed here from the grid's edges by the launch's
own arithmetic and asserted before anything is compared (test_the_batches_step_and_wrap, CPU).  (The C4 scan itself
has nb = 32, cb = 32: a step of exactly 8 tables, no wrap.)

The reference is each point evolved alone: a call of one table has 256 jobs per workgroup, so a work-item stores once,
at the (table, corner) of its one division -- no step takes part --, and such tables are held to the reference-order
oracle by tests/test_reference_order_gpu.py.  A wrong (table, corner) of a pair puts another corner's dilogarithm
into a tile's corner row, which no entry that reads it survives bit for bit.
"""
import numpy as np
import pytest

from tests import cases
from tests.test_alpha_mcorner_div import BATCH_LABEL, _unique_edges

GRID = (300, 12.0, 17.0)
G11 = np.logspace(-3, 0, 11)
SUBSETS = {6: [0, 2, 4, 6, 8, 10], 7: [0, 1, 3, 5, 7, 9, 10], 11: list(range(11))}
EXPECT = {6: (512, 85, 2, 3, 1), 7: (768, 109, 3, 2, 38), 11: (1024, 93, 4, 2, 70)}   # jobs, cb, stores, dq, dr


def _points():
    N, lo, hi = GRID
    base = cases.scan_points(n_mphi=1, n_g=1, N=N, lEmin=lo, lEmax=hi, mphi_range=(6.5, 6.5))[0]
    return [dict(base, g=float(g)) for g in G11]


def _layout(NC, nb):
    """launch_alpha_t's workgroup size for a chunk of one batch of nb tables, and the store loop's steps"""
    jobs = 256 * max(1, min(4, NC * 3 * nb // (2048 * 256)))
    cb = jobs // nb
    stores = -(-cb * nb // 256)
    dq = 256 // cb
    return jobs, cb, stores, dq, 256 - dq * cb


def test_the_batches_step_and_wrap(oracle_mod):
    o = oracle_mod.Oracle(**cases.oracle_kwargs(_points()[0]))
    ue, _ = _unique_edges(o)
    NC = ue.size * (ue.size + 1) // 2
    assert NC == 77421
    for nb, want in EXPECT.items():
        jobs, cb, stores, dq, dr = _layout(NC, nb)
        assert (jobs, cb, stores, dq, dr) == want, nb
        assert jobs > 256 and stores > 1 and 0 < dr < cb and NC % cb != 0
        r0 = np.arange(256) % cb                     # a work-item's corner at its first store
        wraps = r0 + dr >= cb                        # ... wraps at its second
        assert wraps.any() and not wraps.all(), nb
    assert _layout(NC, 1)[:3] == (256, 256, 1)       # a point alone: one store per work-item, no step


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _tables(plan, n):
    return [tuple(np.array(x) for x in plan.tables(i)) for i in range(n)]


@pytest.fixture(scope="module")
def alone():
    """the tables of each of the eleven points evolved in a call of its own"""
    import nusiprop_amd
    nusiprop_amd.load()
    pts = _points()
    p0 = pts[0]
    plan = nusiprop_amd.Plan(p0["N_bins_E"], p0["lEmin"], p0["lEmax"], p0["zmax"], max_points=1, reference_order=True)
    out = []
    for kw in pts:
        plan.evolve([kw])
        out.append(_tables(plan, 1)[0])
    plan.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("nb", sorted(SUBSETS))
def test_batch_equals_points_alone(alone, nb):
    import nusiprop_amd
    from nusiprop_amd import _lib
    sel = SUBSETS[nb]
    pts = [_points()[i] for i in sel]
    p0 = pts[0]
    plan = nusiprop_amd.Plan(p0["N_bins_E"], p0["lEmin"], p0["lEmax"], p0["zmax"], max_points=nb, reference_order=True)
    plan.set_option(_lib.OPT_ALPHA_BATCH, 16)   # one batch of nb tables, whatever the automatic cap
    plan.evolve(pts)
    tabs = _tables(plan, nb)
    names = plan.kernels()
    plan.close()
    assert names[0] == BATCH_LABEL
    for k, i in enumerate(sel):
        for got, ref, what in zip(tabs[k], alone[i], ("Gamma", "alphaTilde", "alpha")):
            bad = np.flatnonzero(_bits(got) != _bits(ref))
            assert bad.size == 0, (nb, i, "%s differs in %d entries, first at %d" % (what, bad.size, bad[0]))
