"""The reference-order alpha batch kernel (k_alpha_batch[refo], the library default) on mixed and edge batches.

tests/test_alpha_paired_tiles.py and tests/test_alpha_staged_chunks.py drive the staged chunks (kStage), the paired
tiles (kPair = 2) and the two-points-per-thread combine (alpha_k_two) with batches whose points differ in g alone,
Majorana / normal ordering throughout.  Here the batches differ in everything the kernel reads per point or per
batch; every call goes through Plan in the reference order with NUSI_OPT_ALPHA_BATCH = 16 unless stated, on the grid
N_E = 45, lE 12 -> 12.75 (T = 91), and for every point of every call
* Gamma, alphaTilde and every alpha entry equal the reference-order oracle's bit for bit (resonant-only tables: the
  m = n + 1 band, 0.0 elsewhere),
* plan.warnings()[k] & 7 equals the oracle's warning word of that point,
* flux and flavour flux are within cases.FLUX_RTOL of the oracle's cascade of its own tables.

The groups (cases.mixed_batch_groups; couplings from logspace(-3, 0, 9), M1 = 10^6.5, M2 = 1e8).  alpha_batches()
keys a batch on (phi-phi, m_phi, the three masses, majorana, non_resonant), so each group is ONE batch under cap 16
-- the test cannot read the batches back, this is by construction:
  A   Majorana, NO, mntot 0.1, M1, 5 couplings; flav 0, 1, 2, 0, 1, si 2.0 .. 3.0, norm 1, 6, 0.5, 2, 1: u[k], a_s,
      a_st, a_nrm, a_gr all differ from point to point (4 + 1: alpha_k_two on the pairs (0, 1), (2, 3), point 4 alone)
  B   Dirac, mntot 0.1, M1, the last 6 couplings (cornered == false under kStage, 4 + 2); warnings 0, 0, 0, 0, 0, 2
  C   inverted ordering, mntot 0.2, M1, 4 couplings
  D   Majorana resonant-only, M1, 3 couplings;  Dp  Dirac resonant-only, M1, 3 couplings
  E   Majorana, mntot = cases.MSUM_MIN_NO (a nearly massless lightest state with the non-resonant channels on: state
      0 takes the S'+ < 1e-5 Taylor branch everywhere, ~1020 negative alpha entries per table), M1, the couplings of
      index 0 .. 4; warnings 3, 3, 1, 1, 3.  Dropped: index 5, 6, 7 (g = 0.075, 0.178, 0.422), whose oracle flux is
      NaN (Gamma goes negative), and index 8 (g = 1), whose oracle flux is finite but diverged (-1.6e268)
  F   Majorana, mntot 0.06, M2, the 7 couplings from index 2 on (4 + 3); warnings 1, 1, 1, 1, 0, 0, 0
A .. E share m_phi: only masses and flags keep them apart, and a key that dropped one of them would merge two groups
into one batch whose shared leaves (from the batch's first point) are wrong for the others.

kWarnAlpha (bit 4) fires nowhere on m_phi in 10^5.5 .. 10^8, g in 1e-3 .. 1 for any of these kinds, so NO GPU TEST PINS
THE ROUTING OF alpha_k_two's SECOND WARNING WORD (w2 -> table p0 + q + kPair); the predicate itself is pinned on the
host (tests/test_hostcheck_tables.py::test_alpha_k_two_bit_identical).

FLUX_RTOL rests on every summed term of the cascade being non-negative, which group E's negative
alpha entries break; E's fluxes are asserted all the same: at its five kept couplings (g <= 0.032, where the
absorption is still weak) they measured 9.6e-15 .. 7.6e-14 of the oracle's on an MI355X, inside the unchanged bound
(_check prints every point's figure before it asserts).
"""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

FLUX_RTOL = cases.FLUX_RTOL
BATCH_LABEL = "k_alpha_mcorner + k_alpha_batch[refo]"
GRID = cases.MIXED_GRID
GROUPS = ["A", "B", "C", "D", "Dp", "E", "F"]
EXPECTED_WARNINGS = {"A": [0] * 5, "B": [0, 0, 0, 0, 0, 2], "C": [0] * 4, "D": [0] * 3, "Dp": [0] * 3,
                     "E": [3, 3, 1, 1, 3], "F": [1, 1, 1, 1, 0, 0, 0]}


@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


class Run:
    """one Plan.evolve call: flux, fla, tabs [(Gamma, alphaTilde, packed alpha)], warn, names, T, N"""


def _run(nusi, pts, cap=16, corner_mb=None):
    from nusiprop_amd import _lib
    N, lo, hi = GRID
    plan = nusi.Plan(N, lo, hi, pts[0]["zmax"], max_points=len(pts), reference_order=True)
    plan.set_option(_lib.OPT_ALPHA_BATCH, cap)
    if corner_mb is not None:
        plan.set_option(_lib.OPT_REFO_CORNER_MB, corner_mb)
    r = Run()
    r.flux, r.fla = plan.evolve(pts)
    r.T, r.N = plan.T, plan.N
    r.tabs = [plan.tables(i) for i in range(len(pts))]
    r.warn = plan.warnings(len(pts))
    r.names = plan.kernels()
    plan.close()
    for a in (r.flux, r.fla) + tuple(x for t in r.tabs for x in t):
        a.setflags(write=False)
    return r


_ref_cache = {}


def _reference(oracle_mod, kw):
    """(Gamma, alphaTilde, alpha, flux, flux_fla, T, warnings) of the reference-order oracle, once per point"""
    key = tuple(sorted(kw.items()))
    if key not in _ref_cache:
        o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
        with oracle_mod.reference_order(1):
            G, aT, al = o.tables()
            w = o.warnings()
            f, fl = o.cascade(G, aT, al)
        for a in (G, aT, al, f, fl):
            a.setflags(write=False)
        _ref_cache[key] = (G, aT, al, f, fl, o.T, w)
    return _ref_cache[key]


def _check(nusi, oracle_mod, pts, r, fluxes=True):
    T = r.T
    iu = np.triu_indices(T, 1)
    for k, kw in enumerate(pts):
        G, aT, al, f_ref, fla_ref, To, w_ref = _reference(oracle_mod, kw)
        assert To == T
        Gg, aTg, Ag = r.tabs[k]
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
        assert (r.warn[k] & 7) == w_ref, (k, r.warn[k], w_ref)
        if fluxes:
            assert np.all(np.isfinite(f_ref)) and np.all(np.isfinite(fla_ref)), k
            e1, e2 = cases.rel_err(r.flux[k], f_ref), cases.rel_err(r.fla[k], fla_ref)
            print("point %d (mntot %.4g, g %.4g): flux rel err %.3e, flavour flux %.3e" % (k, kw["mntot"], kw["g"], e1, e2))
            assert e1 <= FLUX_RTOL, (k, e1)
            assert e2 <= FLUX_RTOL, (k, e2)


def _same_bits(ra, ka, rb, kb):
    for x, y in zip(ra.tabs[ka], rb.tabs[kb]):
        assert np.array_equal(x, y), (ka, kb)
    assert np.array_equal(ra.flux[ka], rb.flux[kb]) and np.array_equal(ra.fla[ka], rb.fla[kb]), (ka, kb)
    assert ra.warn[ka] == rb.warn[kb], (ka, kb)


_alone_cache = {}


def _alone(nusi, name):
    """group `name` as a call of its own, once"""
    if name not in _alone_cache:
        _alone_cache[name] = _run(nusi, cases.mixed_batch_groups()[name])
    return _alone_cache[name]


def _all_points():
    """every group's points in one list, shuffled: (points, [(group, index in group)] per point)"""
    g = cases.mixed_batch_groups()
    pts = [p for name in GROUPS for p in g[name]]
    src = [(name, i) for name in GROUPS for i in range(len(g[name]))]
    perm = np.random.default_rng(20260416).permutation(len(pts))
    return [pts[j] for j in perm], [src[j] for j in perm]


@pytest.fixture(scope="module")
def hetero(nusi):
    pts, src = _all_points()
    return pts, src, _run(nusi, pts)


@pytest.mark.parametrize("name", GROUPS)
def test_group_alone(nusi, oracle_mod, name):
    pts = cases.mixed_batch_groups()[name]
    r = _alone(nusi, name)
    assert r.names[0] == BATCH_LABEL and r.T == 91
    assert len(pts) >= 3   # (fewer tables would take the k-split path)
    _check(nusi, oracle_mod, pts, r)
    assert [w & 7 for w in r.warn] == EXPECTED_WARNINGS[name]


def test_heterogeneous_call(nusi, oracle_mod, hetero):
    """All groups in one call, the input order shuffled: the sort by the batching key must keep unlike groups apart,
    and perm / slot_of must bring every table and warning word back to the caller's index.  Every point also equals
    its group's own call bit for bit (all tables are distinct, so no two points share a cascade workgroup)."""
    pts, src, r = hetero
    assert r.names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, r)
    for k, (name, i) in enumerate(src):
        _same_bits(r, k, _alone(nusi, name), i)


def test_heterogeneous_call_in_corner_chunks(nusi, hetero):
    """The same call under a 4 MiB member-corner block, which holds 9 of its 33 tables: the launch chunks cut between
    unlike batches, and every batch reads its corners relative to its chunk's first table (p0 - pc0)."""
    pts, src, r = hetero
    r4 = _run(nusi, pts, corner_mb=4)
    assert r4.names[0] == BATCH_LABEL
    # the block per table (mcorner_ensure): 6 doubles per pair of distinct bin edges ut <= us -- the N core bins are
    # contiguous (N + 1 edges), each of the T - N redshift-extended bins has its own two
    U = r4.N + 1 + 2 * (r4.T - r4.N)
    per = 8 * 6 * (U * (U + 1) // 2)
    assert (U, per) == (138, 460368)
    held = (4 << 20) // per
    assert held == 9
    largest = max(len(v) for v in cases.mixed_batch_groups().values())
    assert largest <= held < len(pts)
    for k in range(len(pts)):
        _same_bits(r4, k, r, k)


def test_long_run_is_split(nusi, oracle_mod):
    """40 tables of one key: cap 16 cuts the run into near-equal batches of 13 / 13 / 14 (4 + 4 + 4 + 1 and + 2), cap
    255 leaves one batch of 40 (ten chunks, every point through alpha_k_two in the full tiles), cap 0 is automatic
    (on so small a grid one table per batch)."""
    base = cases.mixed_batch_groups()["A"][0]
    pts = [dict(base, flav=2, g=float(g)) for g in np.logspace(-3, 0, 40)]
    r16 = _run(nusi, pts, cap=16)
    assert r16.names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, r16)
    for cap in (255, 0):
        rc = _run(nusi, pts, cap=cap)
        assert rc.names[0] == BATCH_LABEL
        for k in range(len(pts)):
            _same_bits(rc, k, r16, k)


def test_gamma_groups_inside_a_batch(nusi, oracle_mod):
    """Group A's 5 tables, each carrying 3 points that differ in si and norm only (15 points, the table slots
    shared): tables and warnings per point against the oracle, fluxes within FLUX_RTOL (the gamma-batched cascade may
    differ from a lone run to rounding: no bit equality across calls here)."""
    pts = []
    for p in cases.mixed_batch_groups()["A"]:
        pts += [p, dict(p, si=p["si"] + 0.125, norm=3.0 * p["norm"]), dict(p, si=p["si"] - 0.125, norm=0.25 * p["norm"])]
    order = np.random.default_rng(7).permutation(len(pts))
    pts = [pts[j] for j in order]
    r = _run(nusi, pts)
    assert r.names[0] == BATCH_LABEL
    _check(nusi, oracle_mod, pts, r)


@pytest.mark.parametrize("name", ["B", "E"])
def test_batched_equals_alone(nusi, name):
    """Each point of the Dirac batch and of the massless-lightest batch evolved alone (the k-split path of calls of
    few tables, the point-by-point loop) gives the batch's table bits."""
    pts = cases.mixed_batch_groups()[name]
    r = _alone(nusi, name)
    for k, kw in enumerate(pts):
        r1 = _run(nusi, [kw])
        assert r1.names[0] == BATCH_LABEL
        for a, b in zip(r.tabs[k], r1.tabs[0]):
            assert np.array_equal(a, b), k
        assert r1.warn[0] == r.warn[k], k
