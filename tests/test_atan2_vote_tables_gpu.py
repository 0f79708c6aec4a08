"""The first-range vote of nusi_libm.hpp's atan2 inside the alpha kernels: Gamma, alphaTilde and alpha stay
bit-identical to the reference-order oracle on batches whose waves both pass and fail the vote.

Grid and couplings of tests/test_alpha_mcorner_div.py (N_E = 45, lE 12 -> 12.75, T = 91; g = logspace(-3, 0, 9), gr =
g^2 / 16 pi from 2e-8 to 2e-2), every batch at one m_phi:
* *mixed*: that file's mixed batch -- the t of the core's top edge (mass state 2) is -2.002, so c = 2 + t = -0.002.  At
  that edge's corners the member quotient z = a / (c - i gr) has |Im z / Re z| = gr / |c| from 1e-5 to 10: the lanes of
  one k_alpha_mcorner wave (a batch's tables at neighbouring corners) sit in different atan2 ranges at GSL's theta =
  atan2(Im z, Re z) of an inverted call, and the batch kernel's A = carg(-((-1 + S' + i gr) / (c - i gr))) leaves
  range -1 there at the larger couplings.
* *above*, *below*: the S' of the core's top edge (mass state 2) is 1 + 5e-4, and 1 - 5e-4 (two m_phi, so two
  batches).  -1 + S' changes sign between them, A's quotient changes quadrant, and at that edge's corners |Im / Re| of
  A's quotient is gr / 5e-4, from 4e-5 to 40: the batch kernel's A leaves range -1 from g = 0.18 on.
Each batch also runs as its tables {8}, {0, 3, 6, 8} and {0, 2, 4, 6, 8}: 1 table (the batch kernel's k-split
instance), 4 (one chunk) and 5 (a chunk plus one point); every subset keeps g = 1.

What is asserted from the grid's edges in numpy, before any table is compared (test_batches_pass_and_fail_the_vote):
* k_alpha_mcorner, theta site, by the kernel's own job layout for calls this small (test_alpha_mcorner_div._waves: job
  j = tid of a workgroup is corner j / nb of table j % nb, a wave 64 consecutive jobs; the site runs under the inverted
  lanes' mask, so the vote is among a wave's inverted lanes): waves whose inverted lanes are all in range -1, and waves
  with an inverted lane outside it.
* k_alpha_batch, A, by that kernel's own layout: a workgroup takes one class-0 tile of the grid's tile list
  (alpha_tiles_build, through the host library tests/hostcheck_atan2); thread tid < cs ct is the corner of the tile's S'
  edge tid / ct and t edge tid % ct (alpha_edge_list's unique edges of the tile's m bins and n bins), active where ut <=
  us; it forms A for the batch's tables one after the other, so a wave is 64 consecutive threads at one coupling and
  the vote is among its active lanes.  Counted: waves whose active lanes all pass, and waves with one that fails.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import atan2_cases as ac
from tests import cases
from tests.test_alpha_mcorner_div import BATCH_LABEL, G9, MIX_K, MIX_T, _base, _run, _smith, _unique_edges, _waves

SUBSETS = {9: list(range(9)), 1: [8], 4: [0, 3, 6, 8], 5: [0, 2, 4, 6, 8]}
BATCHES = ["mixed", "above", "below"]
DS = 5e-4   # |S' - 1| of the placed edge in the above / below batches


def _zdiv(a, b, c, d):
    """(a + b i) / (c + d i) as oracle/ora_cplx.h zdiv forms it (Smith), elementwise"""
    with np.errstate(all="ignore"):
        first = np.abs(c) < np.abs(d)
        r1 = c / d
        den1 = (c * r1) + d
        re1, im1 = ((a * r1) + b) / den1, ((b * r1) - a) / den1
        r2 = d / c
        den2 = (d * r2) + c
        re2, im2 = ((b * r2) + a) / den2, (b - (a * r2)) / den2
    return np.where(first, re1, re2), np.where(first, im1, im2)


@pytest.fixture(scope="module")
def batches(oracle_mod):
    """per batch: its nine points, and S', t [corner] of mass state 2 in k_alpha_mcorner's corner order, gr [table]"""
    o = oracle_mod.Oracle(**cases.oracle_kwargs(_base()))
    mn, _ = o.prepare()
    ue, N = _unique_edges(o)
    E = ue[N]   # the core's top edge
    mphis = {"mixed": float(np.sqrt(-2 * mn[MIX_K] * E / MIX_T)),
             "above": float(np.sqrt(2 * mn[MIX_K] * E / (1 + DS))),
             "below": float(np.sqrt(2 * mn[MIX_K] * E / (1 - DS)))}
    us, ut = np.tril_indices(ue.size)   # corner c = us (us + 1) / 2 + ut, ut <= us
    out = {}
    # the bins' edges as indices into the unique edges (MCornerDev's eu), and which bins share an edge with the next
    Emin, Emax, _, z = o.grid()
    T = o.T
    lo = np.concatenate([Emin, Emin[N - 1] * (1 + z[1:T - N + 1])])
    hi = np.concatenate([Emax, Emax[N - 1] * (1 + z[1:T - N + 1])])
    elo, ehi, n = np.zeros(T, int), np.zeros(T, int), 0
    for bn in range(T):
        if bn == 0 or lo[bn] != hi[bn - 1]:
            elo[bn] = n
            n += 1
        else:
            elo[bn] = n - 1
        ehi[bn] = n
        n += 1
    assert n == ue.size and np.array_equal(ue[elo], lo) and np.array_equal(ue[ehi], hi)
    shared = np.concatenate([hi[:-1] == lo[1:], [False]]).astype(np.uint8)
    for name, mphi in mphis.items():
        m2 = mphi * mphi
        tk = -2 * mn[MIX_K] * ue / m2
        tk = np.where(np.abs(tk + 1) < 1e-7, tk + tk * 1e-6, tk)   # alpha_t's nudge
        out[name] = dict(pts=[_base(mphi=mphi, g=float(g)) for g in G9], S=(2 * mn[MIX_K] * ue / m2)[us], t=tk[ut],
                         gr=G9 * G9 / (16.0 * np.pi), us=us, ut=ut, edge=N, elo=elo, ehi=ehi, shared=shared, T=T)
    return out


def _clear(t):
    """no lane within 1e-9 of the vote's boundary: numpy's quotient decides the lane's side as the device's does"""
    return not np.any(np.abs(t - 0.4375) < 1e-9)


def _theta_votes(b, sel):
    """k_alpha_mcorner's theta site on the batch's tables sel: (waves whose inverted lanes all pass, waves with an
    inverted lane that fails)"""
    S, t, gr = b["S"][:, None], b["t"][:, None], b["gr"][None, sel]
    a, c = 1 + S + t, 2 + t
    zr, zi = _smith(a + 0 * gr, c + 0 * gr, -gr + 0 * c)
    r2 = zr * zr + zi * zi
    assert not np.any(np.abs(r2 - 1) < 1e-6)
    inv = r2 >= 1
    with np.errstate(all="ignore"):
        tt = np.abs(zi / zr)
    assert _clear(tt[inv])
    fail = inv & (ac.hi(tt) >= ac.R_FIRST)
    any_inv, _ = _waves(inv, len(sel))
    any_fail, _ = _waves(fail, len(sel))
    return int((any_inv & ~any_fail).sum()), int(any_fail.sum())


def _arg_fails(b, sel):
    """the batch kernel's A on the tables sel: fail [corner][table], its quotient's |Im / Re| outside range -1"""
    S, t, gr = b["S"][:, None], b["t"][:, None], b["gr"][None, sel]
    qr, qi = _zdiv(-1 + S + 0 * gr, gr + 0 * S, 2 + t + 0 * gr, -gr + 0 * t)
    with np.errstate(all="ignore"):
        tt = np.abs(qi / qr)   # (the negation changes no modulus)
    assert _clear(tt)
    return ac.hi(tt) >= ac.R_FIRST, qr


@pytest.fixture(scope="module")
def tiles0(batches):
    """the class-0 tiles (n0, ncnt, m0, mcnt) of the grid, from nusi_alpha_tiles.hpp on the host"""
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call(["make", "-s", "-C", os.path.join(here, "hostcheck_atan2")])
    H = ctypes.CDLL(os.path.join(here, "_build", "libhostcheck_atan2.so"))
    b = batches["mixed"]
    out = np.zeros((4096, 4), np.int32)
    sh = np.ascontiguousarray(b["shared"])
    n = H.hc_alpha_tiles0(int(b["T"]), sh.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 4096)
    assert 0 < n <= 4096
    return out[:n]


def _side_edges(b, b0, cnt):
    """alpha_edge_list of bins b0 .. b0 + cnt - 1: the unique-edge index behind each slot of the side's edge list"""
    e = []
    for j in range(b0, min(b0 + cnt, b["T"])):
        if not e or b["elo"][j] != e[-1]:
            e.append(b["elo"][j])
        e.append(b["ehi"][j])
    return np.array(e)


def _arg_votes(b, tiles, fail):
    """k_alpha_batch's A over the class-0 tiles: (waves whose active lanes all pass, waves with one that fails), summed
    over the tables of fail [corner][table]"""
    passed = failed = 0
    for n0, ncnt, m0, mcnt in tiles:
        te, se = _side_edges(b, n0, ncnt), _side_edges(b, m0, mcnt)
        ct, cs = te.size, se.size
        assert cs * ct <= 256 and max(cs, ct) <= 16   # (k_alpha_batch's own condition on a class-0 tile)
        tid = np.arange(cs * ct)
        us, ut = se[tid // ct], te[tid % ct]
        act = ut <= us
        c = np.where(act, us * (us + 1) // 2 + ut, 0)
        pad = (-tid.size) % 64
        act_w = np.concatenate([act, np.zeros(pad, bool)]).reshape(-1, 64)
        for q in range(fail.shape[1]):
            f_w = np.concatenate([act & fail[c, q], np.zeros(pad, bool)]).reshape(-1, 64).any(axis=1)
            passed += int((act_w.any(axis=1) & ~f_w).sum())
            failed += int(f_w.sum())
    return passed, failed


@pytest.mark.parametrize("nb", sorted(SUBSETS))
@pytest.mark.parametrize("name", BATCHES)
def test_batches_pass_and_fail_the_vote(batches, tiles0, name, nb):
    b, sel = batches[name], SUBSETS[nb]
    assert b["gr"][sel][-1] == b["gr"][8]   # g = 1 is the subset's last table
    # the placed edge
    at = (b["ut"] == b["edge"]) if name == "mixed" else (b["us"] == b["edge"])
    want = {"mixed": b["t"][at][0] + 2.002, "above": b["S"][at][0] - (1 + DS), "below": b["S"][at][0] - (1 - DS)}[name]
    assert abs(want) < 1e-9
    passed, failed = _theta_votes(b, sel)
    assert passed >= 1 and failed >= 1, (passed, failed)
    fail, qr = _arg_fails(b, sel)
    passed, failed = _arg_votes(b, tiles0, fail)
    assert passed >= 1 and failed >= 1, (passed, failed)
    read = b["ut"] <= b["us"] - 2
    if name != "mixed":   # A's quotient on either side of the placed edge: -1 + S' has the batch's sign there
        assert (np.sign(-1 + b["S"][at]) == (1 if name == "above" else -1)).all()
        assert (fail[at & read, -1]).all() and (np.sign(qr[at & read, -1]) == (1 if name == "above" else -1)).all()


@pytest.fixture(scope="module")
def oracle_tables(oracle_mod, batches):
    """each point's reference-order oracle tables, computed once"""
    out = {}
    for name, b in batches.items():
        for i, kw in enumerate(b["pts"]):
            o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
            with oracle_mod.reference_order(1):
                out[(name, i)] = tuple(o.tables()) + (o.T,)
    return out


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", sorted(SUBSETS))
@pytest.mark.parametrize("name", BATCHES)
def test_tables_bit_identical(batches, oracle_tables, name, nb):
    sel = SUBSETS[nb]
    pts = [batches[name]["pts"][i] for i in sel]
    tabs, names, T = _run(pts)
    assert names[0] == BATCH_LABEL
    iu = np.triu_indices(T, 1)
    for k, i in enumerate(sel):
        G, aT, al, To = oracle_tables[(name, i)]
        assert To == T
        Gg, aTg, Ad = tabs[k]
        assert np.array_equal(_bits(Gg), _bits(G)), (name, nb, i, "Gamma differs")
        assert np.array_equal(_bits(aTg), _bits(aT)), (name, nb, i, "alphaTilde differs")
        bad = np.flatnonzero(_bits(Ad[iu]) != _bits(al[iu]))
        assert bad.size == 0, (name, nb, i, "alpha differs in %d entries, first (n, m) = (%d, %d)"
                               % (bad.size, iu[0][bad[0]], iu[1][bad[0]]))
