"""The member-corner kernel's divisions by nusi_div.hpp (one refined reciprocal per divisor under wave votes; Smith's
complex division of the quotient z, the 1 / z map, the series' cos / sin and kmax, hypot's correction, the series_2
correction's mn / mx and t_x, t_y): the alpha tables stay bit-identical to the reference-order oracle.

Grid: N_E = 45, lE 12 -> 12.75 (T = 91), the small grid of the other alpha batch tests; every batch holds the nine
couplings g = logspace(-3, 0, 9), so a wave of k_alpha_mcorner (lanes = a batch's tables at ~7 neighbouring corners)
spans gr = g^2 / 16 pi from 2e-8 to 2e-2.
* the scan's two m_phi (10^5.5, 10^8);
* the *mixed* batch: m_phi placed so that the t of one bin edge (mass state 2, the core's top edge) is -2.002: c = 2 + t
  = -0.002 lies between the smallest and the largest gr, so at that edge's corners the lanes at g = 1 take Smith's
  first case (|c| < gr) and the lanes at g = 10^-3 the second, in one wave.  How many corners and waves are mixed in
  this sense is counted here in numpy from the grid's edges, by the kernel's own job layout, and asserted before
  anything is compared; so is a wave that mixes inverted (|z| >= 1) and non-inverted lanes.
* the host build of the same call chain (tests/hostcheck_div, built like tests/hostcheck) on the mixed batch's corners and on
  operands outside the member window, against the oracle's member_dc_ref -- Smith's division of (1 + S + t) by (2 + t -
  i gr), restated in numpy (oracle/ora_cplx.h zdiv; tests/specfun_cases.py smith), into the oracle's GSL complex dilogarithm.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import cases
from tests.specfun_cases import smith as _smith   # (a + 0 i) / (c + d i) as oracle/ora_cplx.h zdiv forms it, elementwise

BATCH_LABEL = "k_alpha_mcorner + k_alpha_batch[refo]"
GRID = (45, 12.0, 12.75)
G9 = np.logspace(-3, 0, 9)
MIX_K, MIX_T = 2, -2.002   # the mixed batch: mass state and the t of the core's top edge
DP = ctypes.POINTER(ctypes.c_double)


def _dp(a):
    return a.ctypes.data_as(DP)


def _base(**over):
    N, lo, hi = GRID
    return dict(cases.scan_points(n_mphi=1, n_g=1, N=N, lEmin=lo, lEmax=hi)[0], **over)


def _unique_edges(o):
    """the member corners' edge energies (mcorner_edges): the Stage-A axis' bin edges, shared edges counted once"""
    Emin, Emax, _, z = o.grid()
    N, T = o.N, o.T
    lo = np.concatenate([Emin, Emin[N - 1] * (1 + z[1:T - N + 1])])
    hi = np.concatenate([Emax, Emax[N - 1] * (1 + z[1:T - N + 1])])
    ue = []
    for b in range(T):
        if b == 0 or lo[b] != hi[b - 1]:
            ue.append(lo[b])
        ue.append(hi[b])
    return np.array(ue), N


@pytest.fixture(scope="module")
def mixed(oracle_mod):
    """the mixed batch's points, and the (S', t) of its member corners per mass state in the kernel's corner order"""
    o = oracle_mod.Oracle(**cases.oracle_kwargs(_base()))
    mn, _ = o.prepare()
    ue, N = _unique_edges(o)
    E = ue[N]   # the core's top edge (the N + 1 core edges come first)
    mphi = float(np.sqrt(-2 * mn[MIX_K] * E / MIX_T))
    pts = [_base(mphi=mphi, g=float(g)) for g in G9]
    m2 = mphi * mphi
    U = ue.size
    us, ut = np.tril_indices(U)   # corner c = us (us + 1) / 2 + ut, ut <= us: row-major lower triangle
    assert np.array_equal(us * (us + 1) // 2 + ut, np.arange(us.size))
    S, t = [], []
    for k in range(3):
        tk = -2 * mn[k] * ue / m2
        tk = np.where(np.abs(tk + 1) < 1e-7, tk + tk * 1e-6, tk)   # alpha_t's nudge
        S.append((2 * mn[k] * ue / m2)[us])
        t.append(tk[ut])
    gr = G9 * G9 * mphi / (16.0 * np.pi) / mphi   # Ga / m_phi (Majorana)
    return dict(pts=pts, S=np.array(S), t=np.array(t), gr=gr, ut=ut, edge=N)


def _waves(flag, nb):
    """flag [corner][table] -> per wave of k_alpha_mcorner (does any lane have it, does any lane lack it).  The
    kernel's layout for a call this small (launch_alpha_t: 256 jobs per workgroup, one per work-item): a workgroup
    takes cb = 256 / nb corners, job j = tid is corner j / nb of table j % nb, a wave 64 consecutive jobs."""
    cb = 256 // nb
    NC = flag.shape[0]
    nwg = -(-NC // cb)
    valid = np.zeros((nwg * cb, nb), bool)
    valid[:NC] = True
    f = np.zeros((nwg * cb, nb), bool)
    f[:NC] = flag
    pad = ((0, 0), (0, 256 - cb * nb))
    v = np.pad(valid.reshape(nwg, cb * nb), pad).reshape(nwg * 4, 64)
    w = np.pad(f.reshape(nwg, cb * nb), pad).reshape(nwg * 4, 64)
    return (w & v).any(axis=1), (~w & v).any(axis=1)


def test_mixed_batch_is_mixed(mixed):
    """The preconditions of the mixed batch, from the grid's edges: corners whose lanes take both of Smith's cases,
    a wave that holds both, and a wave of inverted and non-inverted lanes."""
    S, t, gr = mixed["S"][MIX_K], mixed["t"][MIX_K], mixed["gr"]
    c = 2 + t
    assert abs(c[mixed["ut"] == mixed["edge"]][0] + 0.002) < 1e-9   # the placed edge
    first = np.abs(c)[:, None] < gr[None, :]   # |c| < |d|: Smith's first case
    mixed_corners = first[:, -1] & ~first[:, 0]   # the lane at g = 1 in the first case, at g = 10^-3 in the second
    assert mixed_corners.sum() >= 1, "no corner with both of Smith's cases"
    has, lacks = _waves(first, gr.size)
    assert (has & lacks).sum() >= 1, "no wave with both of Smith's cases"
    a = 1 + S + t
    r2 = (a * a)[:, None] / ((c * c)[:, None] + (gr * gr)[None, :])
    assert not np.any(np.abs(r2 - 1) < 1e-6)   # (clear of |z| = 1: the numpy quotient decides the lanes' side)
    has, lacks = _waves(r2 >= 1, gr.size)
    assert (has & lacks).sum() >= 1, "no wave of inverted and non-inverted lanes"


# ---------------------------------------------------------------------------------------------------- GPU --
def _run(pts):
    import nusiprop_amd
    from nusiprop_amd import _lib
    nusiprop_amd.load()
    p0 = pts[0]
    plan = nusiprop_amd.Plan(p0["N_bins_E"], p0["lEmin"], p0["lEmax"], p0["zmax"], max_points=len(pts),
                             reference_order=True)
    plan.set_option(_lib.OPT_ALPHA_BATCH, 16)   # (the automatic cap of so small a grid is one table per batch)
    plan.evolve(pts)
    T = plan.T
    tabs = [tuple(np.array(x) for x in plan.tables(i)) for i in range(len(pts))]
    tabs = [(G, aT, nusiprop_amd.unpack_alpha(A, T)) for G, aT, A in tabs]
    names = plan.kernels()
    plan.close()
    return tabs, names, T


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _check_tables(oracle_mod, pts, tabs, T):
    iu = np.triu_indices(T, 1)
    for k, kw in enumerate(pts):
        o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
        with oracle_mod.reference_order(1):
            G, aT, al = o.tables()
        assert o.T == T
        Gg, aTg, Ad = tabs[k]
        assert np.array_equal(_bits(Gg), _bits(G)), (k, "Gamma differs")
        assert np.array_equal(_bits(aTg), _bits(aT)), (k, "alphaTilde differs")
        bad = np.flatnonzero(_bits(Ad[iu]) != _bits(al[iu]))
        assert bad.size == 0, (k, kw["g"], "alpha differs in %d entries, first (n, m) = (%d, %d)"
                               % (bad.size, iu[0][bad[0]], iu[1][bad[0]]))


@pytest.mark.gpu
@pytest.mark.parametrize("i_mphi", [0, 1])
def test_scan_batches_bit_identical(oracle_mod, i_mphi):
    """The scan's two m_phi, nine couplings g = 10^-3 .. 1 in one batch each."""
    N, lo, hi = GRID
    pts = cases.scan_points(n_mphi=2, n_g=9, N=N, lEmin=lo, lEmax=hi)[9 * i_mphi:9 * i_mphi + 9]
    assert pts[0]["g"] == 1e-3 and pts[-1]["g"] == 1.0
    tabs, names, T = _run(pts)
    assert names[0] == BATCH_LABEL
    _check_tables(oracle_mod, pts, tabs, T)


@pytest.mark.gpu
def test_mixed_batch_bit_identical(oracle_mod, mixed):
    """Both of Smith's cases, and inverted and non-inverted lanes, in one wave (test_mixed_batch_is_mixed holds the
    batch to that)."""
    tabs, names, T = _run(mixed["pts"])
    assert names[0] == BATCH_LABEL
    _check_tables(oracle_mod, mixed["pts"], tabs, T)


# --------------------------------------------------------------------------------------------- host build --
@pytest.fixture(scope="module")
def hdiv():
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call(["make", "-s", "-C", os.path.join(here, "hostcheck_div")])
    return ctypes.CDLL(os.path.join(here, "_build", "libhostcheck_div.so"))


def _host_dc(H, S, t, gr, inline=True):
    n = S.size
    re, im, win = np.empty(n), np.empty(n), np.empty(n, np.int32)
    S, t, gr = (np.ascontiguousarray(v, dtype=np.float64) for v in (S, t, gr))
    if inline:
        H.hc_member_dc_inl_n(n, _dp(S), _dp(t), _dp(gr), _dp(re), _dp(im), win.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    else:
        H.hc_member_dc_n(n, _dp(S), _dp(t), _dp(gr), _dp(re), _dp(im))
    return re, im, win


def test_host_chain_bit_identical_to_oracle(oracle_mod, hdiv, mixed):
    """alpha_member_ref_dc_inl on the host against the oracle's member_dc_ref (Smith's division, then GSL's complex
    dilogarithm of ora_gsl.c) and against the out-of-line chain the other kernels keep: the mixed batch's corners at
    the placed edge and every 11th other corner, all three mass states and nine couplings -- inside the member window
    -- and operands outside it (c = 0, a = 0, gr and c below 2^-50, a above 2^50), which take the plain divisions."""
    sel = np.zeros(mixed["ut"].size, bool)
    sel[::11] = True
    sel |= mixed["ut"] == mixed["edge"]
    S = np.repeat(mixed["S"][:, sel].ravel(), 9)
    t = np.repeat(mixed["t"][:, sel].ravel(), 9)
    gr = np.tile(mixed["gr"], S.size // 9)
    n_in = S.size
    xs = np.array([0.5, 1.0, 3.0, 1e-3, 2.0 ** 52, 1e20])
    ts = np.array([-2.0, -1.5, -2.0 - 2.0 ** -51, -2.0 + 2.0 ** -52, -1e-3, -1e18, -3.0])
    gs = np.array([2.0 ** -51, 2.0 ** -60, 1e-300, 2e-8, 0.02])
    Sx, tx, gx = (v.ravel() for v in np.meshgrid(xs, ts, gs, indexing="ij"))
    S = np.concatenate([S, Sx])
    t = np.concatenate([t, tx])
    gr = np.concatenate([gr, gx])
    S = np.concatenate([S, -1.0 - ts])   # a = 1 + S + t = 0, or a rounding error of it
    t = np.concatenate([t, ts])
    gr = np.concatenate([gr, np.full(ts.size, 2e-8)])
    re, im, win = _host_dc(hdiv, S, t, gr)
    assert win[:n_in].all() and n_in >= 9000   # the batch's corners are inside the member window
    assert (win[n_in:] == 0).sum() >= 100      # and the made-up operands mostly outside it
    zr, zi = _smith(1 + S + t, 2 + t, -gr)
    for i in range(S.size):
        o_re, o_im = oracle_mod.gsl_complex_dilog(zr[i], zi[i])
        assert (_bits(np.array([re[i], im[i]])) == _bits(np.array([o_re, o_im]))).all() or \
            (np.isnan(o_re) and np.isnan(re[i])) or (np.isnan(o_im) and np.isnan(im[i])), \
            (i, S[i], t[i], gr[i], re[i], im[i], o_re, o_im)
    re2, im2, _ = _host_dc(hdiv, S, t, gr, inline=False)
    same = ((_bits(re) == _bits(re2)) | (np.isnan(re) & np.isnan(re2))) & ((_bits(im) == _bits(im2)) | (np.isnan(im) & np.isnan(im2)))
    assert same.all(), np.flatnonzero(~same)[:5]


def test_host_division_forms(hdiv):
    """nusi_div.hpp's interface on the host build (the plain division behind it): equal to numpy's on operands in and
    out of the window."""
    rng = np.random.default_rng(7)
    n = 4096
    a0, a1, b = (np.ldexp(1 + rng.random(n), rng.integers(-1000, 1000, n)) * rng.choice([-1.0, 1.0], n) for _ in range(3))
    a0[:8] = [0.0, -0.0, np.inf, np.nan, 5e-324, 1.0, -1.0, 2.0 ** 380]
    b[4:12] = [0.0, -0.0, np.inf, np.nan, 5e-324, 1.0, -1.0, 2.0 ** -380]
    q0, q1 = np.empty(n), np.empty(n)
    hdiv.hc_div_shared2_n(n, _dp(a0), _dp(a1), _dp(b), _dp(q0), _dp(q1))
    with np.errstate(all="ignore"):
        h0, h1 = a0 / b, a1 / b
    assert (((_bits(q0) == _bits(h0)) | (np.isnan(q0) & np.isnan(h0))) & ((_bits(q1) == _bits(h1)) | (np.isnan(q1) & np.isnan(h1)))).all()
