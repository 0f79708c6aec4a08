"""The cascade kernels (k_cascade_bs in its one-point, pair and gamma-batch shapes, k_cascade_bs_impulse, k_cascade) at
every boundary of the redshift-step count nst = N_z - 1.

Which instance of nusi_cascade.hip runs, how many step passes it makes and how long its last pass is all follow from
nst (wf_nj, cascade_bs_config; in nusi_cascade_bs_body.inc njp = min(NJ, nst - jb), Ts = N - 1 + njp,
nblk = (Ts + 3) / 4).  The other cascade tests keep zmax = 5 and so reach only nst in {6, 10, 11, 16, 21, 32, 47, 63,
109, 134, 187}.  Here the steps come from zmax on grids of spacing d = 0.02 decades, (N, lo, lo + 0.02 N) with
zmax = 10^(d (nst - 0.5)) - 1: the rule N_z = int(log(1 + zmax) / log(Emax[0] / Emin[0]) + 2) then lands half a step
from either neighbour.  Every case asserts plan.Nz - 1 == nst == oracle.Nz - 1 first, and the kernel name the
selection rule of nusi_plan_evolve reports (Plan.kernels()[1]).

Cases (N = 40, T = 39 + nst, unless stated; "passes" as a sum of the steps of each pass):

  family                     nst   instance <NJ, P, SPL, RT, CW>   passes           name asserted
  one point per workgroup      1   <16, 1, 1, 4, 1>                1                k_cascade_bs
  (OPT_CASCADE_RHS = 1)        2   <16, ...>                       2                k_cascade_bs
                              15   <16, ...>                       15               k_cascade_bs
                              16   <16, ...>  (full)               16               k_cascade_bs
                              17   <32, 1, 1, 4, 1>  (smallest)    17               k_cascade_bs
                              31   <32, ...>                       31               k_cascade_bs
                              32   <32, ...>  (full)               32               k_cascade_bs
                              33   <48, 1, 1, 4, 1>  (smallest)    33               k_cascade_bs
                              47   <48, ...>                       47               k_cascade_bs
                              48   <48, ...>  (full)               48               k_cascade_bs
                              49   <48, ...>                       48 + 1           k_cascade_bs
                              95   <48, ...>                       48 + 47          k_cascade_bs
                              96   <48, ...>                       48 + 48          k_cascade_bs
                              97   <48, ...>                       48 + 48 + 1      k_cascade_bs
  forced step passes           1   <16, 1, 1, 8, 1>                1                k_cascade_bs
  (OPT_STEP_PASSES = 1)       15                                   15               k_cascade_bs
                              16                                   16               k_cascade_bs
                              17                                   16 + 1           k_cascade_bs
                              32                                   16 + 16          k_cascade_bs
                              33                                   16 + 16 + 1      k_cascade_bs
                              48                                   16 + 16 + 16     k_cascade_bs
                              49                                   3 x 16 + 1       k_cascade_bs
  pairs (automatic)            1   <16, 2, 1, 2, 2>                1                k_cascade_bs_pairs
                              16   <16, 2, ...>                    16               k_cascade_bs_pairs
                              17   <32, 2, 1, 2, 2>                17               k_cascade_bs_pairs
                              32   <32, 2, ...>                    32               k_cascade_bs_pairs
                              33   <48, 2, 1, 2, 2>                33               k_cascade_bs_pairs
                              48   <48, 2, ...>                    48               k_cascade_bs_pairs
                              49   <48, 2, ...>                    48 + 1           k_cascade_bs_pairs
                              97   <48, 2, ...>                    48 + 48 + 1      k_cascade_bs_pairs
  gamma batches (automatic)    1   <6, 16, 1, 2, 2>                1                k_cascade_bs_gamma
  of 3 + 3 and of 16           5                                   5                k_cascade_bs_gamma
                               6                                   6                k_cascade_bs_gamma
                               7                                   6 + 1            k_cascade_bs_gamma
                              11                                   6 + 5            k_cascade_bs_gamma
                              12                                   6 + 6            k_cascade_bs_gamma
                              13                                   6 + 6 + 1        k_cascade_bs_gamma
                              47                                   7 x 6 + 5        k_cascade_bs_gamma
                              48                                   8 x 6            k_cascade_bs_gamma
                              49                                   8 x 6 + 1        k_cascade_bs_gamma
                              97                                   16 x 6 + 1       k_cascade_bs_gamma
  tabulated power law, one     1, 16, 17, 48, 49, 97: the one-point instances above, their sources read a block
  point per workgroup          ahead from k_source_tab's table                      k_cascade_bs
  DSNB on (40, 4.0, 4.8)       1, 2, 16: <16, 1, ...>; 17: <32, 1, ...>             k_cascade_bs
                               1, 2, 16, 17 in a batch of 3: <6, 16, ...>           k_cascade_bs_gamma
  impulse (Plan.response)      1, 5, 6, 7, 12, 13, 49: <6, 16, 1, 2, 2>, passes as the gamma batch's; T mod 16 =
                               8, 12, 13, 14, 3, 4, 8                               k_cascade_bs_impulse
  stage-count residues         the one-point instance, the gamma batches and the impulse at nst 48 and 49 again at
                               N = 41, 42, 43: Ts mod 4 of the first and the last pass takes every residue and nblk
                               both parities
  the scalar kernel            every nst of the one-point list, its three names     k_cascade

No case's kernel name differs from the grouping it is named for: at T <= 139 the pair and gamma-batch shapes fit at
every nst (bs_fits_t), beyond 48 steps included, so the rule sends nothing to another kernel.  Alone a pair launch is
named "k_cascade_bs_pairs" ("pairs" only inside a combined name).

Physics: scan_points(...)[0] with m_phi = 10^6.5, g = 0.1, si = 2.5, the power-law source; a Dirac point, a second
Majorana point and a resonant-only point give the one-point launches distinct tables.  Two preconditions are asserted
on the oracle alone for every (grid, point, nst), so that no case is vacuous (test_preconditions_on_the_oracle runs
just these without a GPU):
  * the interaction is visible: flux_fla differs from the same point's at g = 1e-9 by >= 1e-2 in some bin;
  * the last step is visible: flux and flux_fla differ from the run of nst - 1 steps on the same grid by >= 1e-6 in
    some bin (1e5 x FLUX_RTOL; the smallest measured is 4e-5 at nst = 50).  At nst = 1 the run of no step is the zero
    initial condition, so the effect is 1 wherever the flux is positive.
Both are relative to the larger of the two values.  The DSNB has died out by 33 steps on its grid (a last-step effect
of exactly 0), hence its short list; the late steps of the table-source path are covered by the tabulated power law.

Yardsticks, all to cases.FLUX_RTOL (the project's bound for summation-order differences) on flux and flux_fla:
  1. the oracle's cascade() on the GPU's own tables (tests/test_cascade_bs.py::_vs_oracle);
  2. the scalar k_cascade on the same points, with the same exact zeros; its three names bit-equal to each other;
  3. for tabulated points, the oracle's power-law evolve() under reference_order(1) against a power law put through
     Plan.set_source (the construction of tests/test_tabulated_source_gpu.py);
  4. for the response, response.apply_host(G[0], power_law_integrals) / fs against that same oracle run.
A launch of non-resonant points alone runs the kNR instance, the same points with a resonant-only one added the
per-point-flag instance: the non-resonant points must have equal bits in both.  Grouped launches agree with the
one-point-per-workgroup launch of the same points to FLUX_RTOL with the same zeros (no bits: the step passes differ).

Worst relative error against the oracle per family, measured on the MI355X (each item prints its own; the bound
asserted stays FLUX_RTOL = 1e-11): one point per workgroup 1.5e-13, forced step passes 1.4e-13, pairs 1.5e-13, gamma
batches of three 1.7e-13 and of sixteen 1.8e-13, tabulated 1.3e-13, DSNB 1.6e-13 (one point and batch), impulse
1.3e-13, the scalar kernel 1.5e-15.  The same table is in DESIGN.md sec. 2, "Step boundaries".
"""
import numpy as np
import pytest

from tests import cases

gpu = pytest.mark.gpu
FLUX_RTOL = cases.FLUX_RTOL
D = 0.02                       # the grids' spacing in decades
INTERACTION_MIN = 1e-2
LAST_STEP_MIN = 1e-6

ONE = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 95, 96, 97]
FORCED = [1, 15, 16, 17, 32, 33, 48, 49]
PAIRS = [1, 16, 17, 32, 33, 48, 49, 97]
GAMMA = [1, 5, 6, 7, 11, 12, 13, 47, 48, 49, 97]
TAB = [1, 16, 17, 48, 49, 97]
DSNB = [1, 2, 16, 17]
IMPULSE = [1, 5, 6, 7, 12, 13, 49]
RESIDUES = [(nst, N) for nst in (48, 49) for N in (41, 42, 43)]


def _with_residues(lst):
    return [(nst, 40) for nst in lst] + RESIDUES


def zmax_of(nst):
    return 10.0 ** (D * (nst - 0.5)) - 1.0


def _pt(nst, N=40, lo=12.0, **over):
    p = cases.scan_points(n_mphi=1, n_g=1, N=N, lEmin=lo, lEmax=lo + D * N)[0]
    p.update(mphi=10 ** 6.5, g=0.1, si=2.5, zmax=zmax_of(nst))
    p.update(over)
    return p


# --- the points of each family: (point, slot) lists; slot None = the point as it stands, else the power law `point`
# put through source slot `slot` of the plan -------------------------------------------------------------------------
DIRAC = dict(mphi=10 ** 6.8, g=0.2, majorana=False)
SECOND = dict(mphi=10 ** 6.2, g=0.05, si=2.2)
RES = dict(non_resonant=False)
LOW = dict(lo=4.0, mphi=10 ** 6.5 / 200)      # the DSNB's grid (40, 4.0, 4.8)


def one_pts(nst, N):
    """(non-resonant points, resonant-only points): three distinct tables, one of them Dirac; a fourth, resonant-only."""
    return [(_pt(nst, N), None), (_pt(nst, N, **DIRAC), None), (_pt(nst, N, **SECOND), None)], [(_pt(nst, N, **RES), None)]


def pair_pts(nst, N):
    sis = ((2.1, 1.0), (2.9, 2.5))
    return ([(_pt(nst, N, si=s, norm=n), None) for s, n in sis], [(_pt(nst, N, si=s, norm=n, **RES), None) for s, n in sis])


def gamma3_pts(nst, N):
    def three(**over):
        return [(_pt(nst, N, **over), None), (_pt(nst, N, norm=1.0, **over), 0), (_pt(nst, N, si=2.0, norm=3.0, **over), None)]
    return three(), three(**RES)


def gamma16_pts(nst, N):
    return [(_pt(nst, N, si=2.0 + 0.06 * k, norm=1.0 + 0.1 * k), None) for k in range(16)], []


def tab_pts(nst, N):
    return [(_pt(nst, N), 0), (_pt(nst, N, si=2.0), 1)], [(_pt(nst, N, **RES), 0)]


def dsnb_pts(nst, N):
    """One table: two DSNB points and a power law (a mixed batch); resonant-only, a DSNB point of its own table."""
    return ([(_pt(nst, N, source_model=0, **LOW), None), (_pt(nst, N, source_model=0, norm=6.0, **LOW), None),
             (_pt(nst, N, si=2.2, **LOW), None)], [(_pt(nst, N, source_model=0, **dict(LOW, **RES)), None)])


def impulse_pts(nst, N):
    return [(_pt(nst, N), None)], [(_pt(nst, N, **RES), None)]


FAMILIES = [("one", _with_residues(ONE), one_pts), ("forced", [(n, 40) for n in FORCED], one_pts),
            ("pairs", [(n, 40) for n in PAIRS], pair_pts), ("gamma3", _with_residues(GAMMA), gamma3_pts),
            ("gamma16", _with_residues(GAMMA), gamma16_pts), ("tab", [(n, 40) for n in TAB], tab_pts),
            ("dsnb", [(n, 40) for n in DSNB], dsnb_pts), ("impulse", _with_residues(IMPULSE), impulse_pts)]


# --- the oracle alone: step counts and preconditions -----------------------------------------------------------------
_EVOLVE, _CHECKED, _PL = {}, set(), {}


def _key(p):
    return tuple(sorted(p.items()))


def _evolve(oracle_mod, p):
    """(flux, flux_fla, Nz, warnings) of the oracle's evolve(), once per point."""
    k = _key(p)
    if k not in _EVOLVE:
        o = oracle_mod.Oracle(**cases.oracle_kwargs(p))
        f, fl = o.evolve()
        f.setflags(write=False)
        fl.setflags(write=False)
        _EVOLVE[k] = (f, fl, o.Nz, o.warnings())
    return _EVOLVE[k]


def _differ(a, b):
    """max |a - b| / max(|a|, |b|) over the entries where either is nonzero."""
    s = np.maximum(np.abs(a), np.abs(b))
    m = s > 0
    return float(np.max(np.abs(a - b)[m] / s[m])) if np.any(m) else 0.0


def _preconditions(oracle_mod, p, nst):
    """The step count, and the two effects that keep a case from being vacuous, on the oracle alone."""
    k = (_key(p), nst)
    if k in _CHECKED:
        return
    f, fl, Nz, warn = _evolve(oracle_mod, p)
    assert Nz - 1 == nst, (Nz, nst)
    assert warn == 0 and np.all(np.isfinite(f)) and np.all(np.isfinite(fl)) and np.any(f > 0), (nst, warn)
    free = _evolve(oracle_mod, dict(p, g=1e-9))
    inter = _differ(fl, free[1])
    assert inter >= INTERACTION_MIN, (nst, inter, p)
    if nst > 1:
        f1, fl1, Nz1, _ = _evolve(oracle_mod, dict(p, zmax=zmax_of(nst - 1)))
        assert Nz1 - 1 == nst - 1
        last = min(_differ(f, f1), _differ(fl, fl1))
    else:        # no step: the zero initial condition
        last = 1.0
    assert last >= LAST_STEP_MIN, (nst, last, p)
    _CHECKED.add(k)


def _oracle_pl(oracle_mod, p):
    """(flux, flux_fla, fs) of the oracle's power-law run in the reference order at norm = 1 (fs = 1 / norm_total)."""
    q = dict(p, norm=1.0)
    k = _key(q)
    if k not in _PL:
        with oracle_mod.reference_order(1):
            o = oracle_mod.Oracle(**cases.oracle_kwargs(q))
            _, nt = o.prepare()
            f, fl = o.evolve()
        assert np.all(np.isfinite(f)) and np.all(f >= 0) and np.any(f > 0)
        f.setflags(write=False)
        fl.setflags(write=False)
        _PL[k] = (f, fl, 1.0 / nt)
    return _PL[k]


ALL_NST = sorted({nst for _, lst, _ in FAMILIES for nst, _ in lst})


@pytest.mark.parametrize("nst", ALL_NST)
def test_preconditions_on_the_oracle(oracle_mod, nst):
    """Every (grid, point, nst) of the module: nst steps, a visible interaction, a visible last step.  No GPU."""
    n = 0
    for _, lst, pts in FAMILIES:
        for s, N in lst:
            if s == nst:
                nr, res = pts(nst, N)
                for p, _ in nr + res:
                    _preconditions(oracle_mod, p, nst)
                    n += 1
    assert n > 0


def test_zmax_zero_is_one_step_on_the_oracle(oracle_mod):
    assert oracle_mod.Oracle(**cases.oracle_kwargs(_pt(1, zmax=0.0))).Nz - 1 == 1


# --- the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nusi():
    import nusiprop_amd
    nusiprop_amd.load()
    return nusiprop_amd


def _launch(nusi, oracle_mod, tagged, nst, **opts):
    """Plan.evolve of the (point, slot) list in the library's default arithmetic; opts: cascade = a CASCADE_* name, or
    OPT_* options.  Returns (flux, flux_fla, tables per point, the cascade kernel's name)."""
    from nusiprop_amd import _lib, sources
    p0 = tagged[0][0]
    plan = nusi.Plan(p0["N_bins_E"], p0["lEmin"], p0["lEmax"], p0["zmax"], max_points=len(tagged))
    try:
        assert plan.Nz - 1 == nst, (plan.Nz, nst)
        for k, v in opts.items():
            if k == "cascade":
                plan.set_cascade(getattr(_lib, "CASCADE_" + v))
            else:
                plan.set_option(getattr(_lib, "OPT_" + k.upper()), v)
        lo, hi, _ = plan.source_axis()
        pts, slots = [], {}
        for p, slot in tagged:
            if slot is None:
                pts.append(p)
                continue
            assert slots.setdefault(slot, p["si"]) == p["si"]
            fs = _oracle_pl(oracle_mod, p)[2]
            pts.append(dict(p, si=7.5, norm=p["norm"] / fs, source_model=sources.tabulated(slot)))   # (si is ignored)
        for slot, si in slots.items():
            plan.set_source(slot, sources.power_law_integrals(lo, hi, si))
        flux, fla = plan.evolve(pts)
        assert all(w == 0 for w in plan.warnings(len(pts)))
        tabs = [plan.tables(i) for i in range(len(pts))]
        return flux, fla, tabs, plan.kernels()[1]
    finally:
        plan.close()


def _vs_oracle(nusi, oracle_mod, tagged, nst, run, what):
    """Yardsticks 1 and 3 for every point of a launch; asserts the preconditions of each point first."""
    flux, fla, tabs, _ = run
    worst = 0.0
    for k, (p, slot) in enumerate(tagged):
        _preconditions(oracle_mod, p, nst)
        if slot is None:
            o = oracle_mod.Oracle(**cases.oracle_kwargs(p))
            assert o.Nz - 1 == nst
            o.prepare()
            G, aT, A = tabs[k]
            f_ref, fl_ref = o.cascade(G, aT, nusi.unpack_alpha(A, o.T))
        else:
            f_ref, fl_ref, _ = _oracle_pl(oracle_mod, p)
            f_ref, fl_ref = p["norm"] * f_ref, p["norm"] * fl_ref
        e = max(cases.rel_err(flux[k], f_ref), cases.rel_err(fla[k], fl_ref))
        worst = max(worst, e)
        assert e <= FLUX_RTOL, (what, nst, k, e, p)
    print("step-boundary %s nst=%d N=%d: worst vs the oracle %.2e" % (what, nst, tagged[0][0]["N_bins_E"], worst))


def _same_to_rounding(a, b):
    for x, y in zip(a[:2], b[:2]):
        d = max(cases.rel_err(x[k], y[k]) for k in range(len(x)))
        assert d <= FLUX_RTOL and np.array_equal(x == 0, y == 0), d


def _family(nusi, oracle_mod, what, pts, nst, N, name, one_too=False, **opts):
    """A family's launches at (nst, N): the non-resonant points alone (kNR), then with the resonant-only ones (the
    per-point-flag instance) -- equal bits for the former; every point against the oracle and the scalar kernel;
    one_too: and against its one-point-per-workgroup launch."""
    nr, res = pts(nst, N)
    a = _launch(nusi, oracle_mod, nr, nst, **opts)
    assert a[3] == name, a[3]
    b = a
    if res:
        b = _launch(nusi, oracle_mod, nr + res, nst, **opts)
        assert b[3] == name, b[3]
        assert np.array_equal(a[0], b[0][:len(nr)]) and np.array_equal(a[1], b[1][:len(nr)])
    _vs_oracle(nusi, oracle_mod, nr + res, nst, b, what)
    ref = _launch(nusi, oracle_mod, nr + res, nst, cascade="LDS")
    assert ref[3] == "k_cascade", ref[3]
    _same_to_rounding(b, ref)
    if one_too:
        one = _launch(nusi, oracle_mod, nr + res, nst, cascade_rhs=1)
        assert one[3] == "k_cascade_bs", one[3]
        _same_to_rounding(b, one)


@gpu
def test_smallest_zmax_is_one_step(nusi, oracle_mod):
    """The step rule's lower end.  zmax = 0 gives the oracle one step (test_zmax_zero_is_one_step_on_the_oracle);
    nusi_plan_create refuses it by contract (zmax > 0: tests/test_plan_errors_gpu.py), so the plan's lower end is the
    smallest positive zmax: one step, the redshift grid of the nst = 1 cases (z[N_z - 1] replaces zmax), the same bits."""
    nr, _ = one_pts(1, 40)
    tiny = [(dict(p, zmax=5e-324), s) for p, s in nr]
    a = _launch(nusi, oracle_mod, tiny, 1, cascade_rhs=1)
    b = _launch(nusi, oracle_mod, nr, 1, cascade_rhs=1)
    assert a[3] == b[3] == "k_cascade_bs"
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.any(a[0] > 0)


@gpu
@pytest.mark.parametrize("nst,N", _with_residues(ONE))
def test_one_point_per_workgroup(nusi, oracle_mod, nst, N):
    _family(nusi, oracle_mod, "one", one_pts, nst, N, "k_cascade_bs", cascade_rhs=1)


@gpu
@pytest.mark.parametrize("nst", ONE)
def test_scalar_names_bit_equal(nusi, oracle_mod, nst):
    """k_cascade under its three names: the same bits at every nst of the one-point list."""
    nr, res = one_pts(nst, 40)
    runs = [_launch(nusi, oracle_mod, nr + res, nst, cascade=c) for c in ("WAVEFRONT", "REG", "LDS")]
    for r in runs:
        assert r[3] == "k_cascade", r[3]
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])
    _vs_oracle(nusi, oracle_mod, nr + res, nst, runs[0], "scalar")


@gpu
@pytest.mark.parametrize("nst", FORCED)
def test_forced_step_passes(nusi, oracle_mod, nst):
    _family(nusi, oracle_mod, "forced", one_pts, nst, 40, "k_cascade_bs", step_passes=1)


@gpu
@pytest.mark.parametrize("nst", PAIRS)
def test_pairs(nusi, oracle_mod, nst):
    _family(nusi, oracle_mod, "pairs", pair_pts, nst, 40, "k_cascade_bs_pairs", one_too=True)


@gpu
@pytest.mark.parametrize("nst,N", _with_residues(GAMMA))
def test_gamma_batch_of_three(nusi, oracle_mod, nst, N):
    """Batches of 3 (non-resonant, then with a resonant-only batch beside it), the tabulated power law in each."""
    _family(nusi, oracle_mod, "gamma3", gamma3_pts, nst, N, "k_cascade_bs_gamma", one_too=True)


@gpu
@pytest.mark.parametrize("nst,N", _with_residues(GAMMA))
def test_gamma_batch_of_sixteen(nusi, oracle_mod, nst, N):
    _family(nusi, oracle_mod, "gamma16", gamma16_pts, nst, N, "k_cascade_bs_gamma", one_too=True)


@gpu
@pytest.mark.parametrize("nst", TAB)
def test_tabulated_one_point_per_workgroup(nusi, oracle_mod, nst):
    _family(nusi, oracle_mod, "tab", tab_pts, nst, 40, "k_cascade_bs", cascade_rhs=1)


@gpu
@pytest.mark.parametrize("nst", DSNB)
def test_dsnb(nusi, oracle_mod, nst):
    """One point per workgroup (a resonant-only DSNB point among them), then the three of one table as a batch."""
    _family(nusi, oracle_mod, "dsnb", dsnb_pts, nst, 40, "k_cascade_bs", cascade_rhs=1)
    _family(nusi, oracle_mod, "dsnb batch", lambda s, n: (dsnb_pts(s, n)[0], []), nst, 40, "k_cascade_bs_gamma", one_too=True)


@gpu
@pytest.mark.parametrize("nst,N", _with_residues(IMPULSE))
def test_impulse(nusi, oracle_mod, nst, N):
    """Plan.response at (nst, N): G . S / fs against the oracle's power law (yardstick 4), +0.0 where n <= b, and the
    last, partial group of 16 source-axis bins finite, non-negative and not empty."""
    from nusiprop_amd import response, sources
    nr, res = impulse_pts(nst, N)
    pts = [p for p, _ in nr + res]
    plan = nusi.Plan(N, pts[0]["lEmin"], pts[0]["lEmax"], pts[0]["zmax"], max_points=2)
    try:
        assert plan.Nz - 1 == nst
        lo, hi, _ = plan.source_axis()
        Ga, Gfa = plan.response(pts[:1])                       # all non-resonant: the kNR instance
        assert plan.kernels()[1] == "k_cascade_bs_impulse", plan.kernels()
        G, Gf = plan.response(pts)                             # the per-point-flag instance
        assert plan.kernels()[1] == "k_cascade_bs_impulse", plan.kernels()
    finally:
        plan.close()
    assert np.array_equal(Ga[0], G[0]) and np.array_equal(Gfa[0], Gf[0])
    M = N + nst
    assert G.shape == Gf.shape == (2, M, 3, N)
    n_idx, b_idx = np.arange(M)[:, None], np.arange(N)[None, :]
    at_or_above = np.broadcast_to((n_idx <= b_idx)[None, :, None, :], G.shape)
    last_group = 1 + 16 * ((M - 2) // 16)
    for A in (G, Gf):
        assert np.all(np.isfinite(A)) and np.all(A >= 0.0)
        z = A[at_or_above]
        assert np.all(z == 0.0) and not np.any(np.signbit(z))          # +0.0 for n <= b (column 0 included)
        assert np.all(np.max(A[:, 1:], axis=(2, 3)) > 0.0)             # every column n >= 1 has a positive entry
        # the top source-axis bins n >= N (the last group's among them) enter at bin N - 1, in step n - (N - 1)
        assert last_group < M and np.all(A[:, N:, :, N - 1].max(axis=2) > 0.0)
    S = sources.power_law_integrals(lo, hi, 2.5)
    worst = 0.0
    for k, p in enumerate(pts):
        _preconditions(oracle_mod, p, nst)
        f, fl, fs = _oracle_pl(oracle_mod, p)
        e = max(cases.rel_err(response.apply_host(G[k], S) / fs, f), cases.rel_err(response.apply_host(Gf[k], S) / fs, fl))
        worst = max(worst, e)
        assert e <= FLUX_RTOL, (nst, N, k, e)
    print("step-boundary impulse nst=%d N=%d: worst vs the oracle %.2e" % (nst, N, worst))
