"""Stage-A table formulas of the product (nusiprop_amd/csrc/nusi_physics.hpp,
compiled for the host by tests/hostcheck) against the oracle, BIT FOR BIT, on
CPU.  The GPU runs the same source (tests/test_gpu_parity.py checks the device
build); this catches a formula divergence without a GPU.

The per-point scalars (masses, |U|^2, width, norm_total) are taken from the
oracle, which is what the product's host code computes the same way
(nusi_capi.cpp build_point; nuSIprop.hpp:130-205)."""
import ctypes

import numpy as np
import pytest

from tests import cases

DP = ctypes.POINTER(ctypes.c_double)


def _dp(a):
    return a.ctypes.data_as(DP)


def extended_axis(o):
    """Stage-A energy axis (nuSIprop.hpp:217-252): the N bins, then the top bin
    redshifted by (1+z_j), j = 1..N_z-2."""
    Emin, Emax, _, z = o.grid()
    N, T = o.N, o.T
    lo, hi = np.empty(T), np.empty(T)
    lo[:N], hi[:N] = Emin, Emax
    for n in range(N, T):
        lo[n] = Emin[N - 1] * (1 + z[n - N + 1])
        hi[n] = Emax[N - 1] * (1 + z[n - N + 1])
    return lo, hi


def point_array(o, kw):
    mn, norm_total = o.prepare()
    U2 = o.mixing()
    g, mphi = kw["g"], kw["mphi"]
    Ga = g * g * mphi / (16.0 * np.pi) if kw["majorana"] else g * g * mphi / (8.0 * np.pi)
    u = U2[kw["flav"]]
    pt = np.array([mphi, g, kw["mntot"], kw["si"], kw["norm"], norm_total, Ga, *mn, *u], dtype=np.float64)
    flags = (ctypes.c_int * 4)(int(kw["majorana"]), int(kw["non_resonant"]), int(kw["phiphi"]),
                               int(kw.get("source_model", 0)))
    return pt, flags


@pytest.mark.parametrize("name", sorted(cases.SMALL_CASES))
def test_tables_bit_identical(oracle_mod, name):
    from tests.hostcheck import build_hostcheck
    H = build_hostcheck()
    kw = dict(cases.SMALL_CASES[name], N_bins_E=40)
    o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
    G, aT, al = o.tables()
    lo, hi = extended_axis(o)
    pt, flags = point_array(o, kw)
    T = o.T
    Gh, aTh, Ah = np.zeros(T), np.zeros(T), np.zeros((T, T))
    H.hc_tables.restype = ctypes.c_int
    w = H.hc_tables(_dp(pt), flags, T, _dp(lo), _dp(hi), _dp(Gh), _dp(aTh), _dp(Ah))
    assert np.array_equal(Gh, G)
    assert np.array_equal(aTh, aT)
    iu = np.triu_indices(T, 1)
    assert np.array_equal(Ah[iu], al[iu]), "%d alpha entries differ" % np.sum(Ah[iu] != al[iu])
    assert (w & 7) == o.warnings()


@pytest.mark.parametrize("name,N", [("test_cpp", 40), ("c2b", 44), ("dirac", 31), ("resonant_only", 40),
                                    ("inverted", 46), ("strong", 40)])
def test_tiled_alpha_bit_identical(oracle_mod, name, N):
    """The tile kernel's data path (edge dedup, per-edge / per-corner leaf arrays,
    TileLeaves slot mapping), emulated on the host, against the oracle: bit for bit.
    N is chosen so the tiles straddle the N | redshift-extended junction."""
    from tests.hostcheck import build_hostcheck
    H = build_hostcheck()
    kw = dict(cases.SMALL_CASES[name], N_bins_E=N)
    o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
    _, _, al = o.tables()
    lo, hi = extended_axis(o)
    pt, flags = point_array(o, kw)
    T = o.T
    Ah = np.zeros((T, T))
    H.hc_alpha_tiled.restype = ctypes.c_int
    w = H.hc_alpha_tiled(_dp(pt), flags, T, _dp(lo), _dp(hi), _dp(Ah))
    iu = np.triu_indices(T, 1)
    if kw["non_resonant"]:
        assert np.array_equal(Ah[iu], al[iu]), "%d alpha entries differ" % np.sum(Ah[iu] != al[iu])
    else:
        d = np.arange(T - 1)
        assert np.array_equal(Ah[d, d + 1], al[d, d + 1])
    assert (w & 4) == (o.warnings() & 4)


@pytest.mark.parametrize("name", sorted(cases.SMALL_CASES))
def test_reference_order_tables_bit_identical(oracle_mod, name):
    """NUSI_OPT_REFERENCE_ORDER on the device headers (the kRef instances of gamma_entry / alphat_entry /
    alpha_entry: the general complex dilogarithm, the reference's quotient and carg for the s-t member leaves)
    against the oracle in reference-order mode (ora_set_reference_order(1)): bit for bit; and they differ from
    the default order somewhere (the mode is not a no-op) wherever the s-t interference is computed."""
    from tests.hostcheck import build_hostcheck
    H = build_hostcheck()
    kw = dict(cases.SMALL_CASES[name], N_bins_E=40)
    o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
    with oracle_mod.reference_order(1):
        G, aT, al = o.tables()
    lo, hi = extended_axis(o)
    pt, flags = point_array(o, kw)
    T = o.T
    Gh, aTh, Ah = np.zeros(T), np.zeros(T), np.zeros((T, T))
    H.hc_tables_ref.restype = ctypes.c_int
    w = H.hc_tables_ref(_dp(pt), flags, T, _dp(lo), _dp(hi), _dp(Gh), _dp(aTh), _dp(Ah))
    assert np.array_equal(Gh, G)
    assert np.array_equal(aTh, aT)
    iu = np.triu_indices(T, 1)
    assert np.array_equal(Ah[iu], al[iu]), "%d alpha entries differ" % np.sum(Ah[iu] != al[iu])
    assert (w & 7) == o.warnings()
    Ad = np.zeros((T, T))
    H.hc_alpha_tiled_ref.restype = ctypes.c_int
    H.hc_alpha_tiled_ref(_dp(pt), flags, T, _dp(lo), _dp(hi), _dp(Ad))
    if kw["non_resonant"]:
        assert np.array_equal(Ad[iu], al[iu]), "tiled: %d alpha entries differ" % np.sum(Ad[iu] != al[iu])
        if kw["majorana"]:
            _, _, al0 = o.tables()
            assert np.any(al0[iu] != al[iu])


def _two_pairs():
    """(a, b) of one batch -- the same m_phi, masses and flags; Majorana, non-resonant -- on N_E = 31 of the mixed
    batches' grid"""
    _, lo, hi = cases.MIXED_GRID
    g = cases.mixed_batch_groups()
    A = [dict(p, N_bins_E=31, lEmin=lo, lEmax=hi, flav=2, si=2.5, norm=1.0) for p in g["A"]]
    E = [dict(p, N_bins_E=31, lEmin=lo, lEmax=hi) for p in g["E"]]
    return {
        "g": (A[2], A[3]),
        "flav": (A[2], dict(A[2], flav=0)),
        "g_flav_si_norm": (A[1], dict(A[4], flav=1, si=2.0, norm=6.0)),
        "same": (A[3], A[3]),
        "massless_lightest": (E[2], E[4]),
    }


TWO_PAIRS = ["g", "flav", "g_flav_si_norm", "same", "massless_lightest"]
_two_cache = {}


def _two_run(oracle_mod, pair):
    """hc_alpha_two_ref on the pair, once: (Aa, Ab, wa, wb, fallbacks, oracle alpha of a, of b, oracle warnings)"""
    if pair not in _two_cache:
        from tests.hostcheck import build_hostcheck
        H = build_hostcheck()
        a, b = _two_pairs()[pair]
        tabs, warn, pts = [], [], []
        for kw in (a, b):
            o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
            with oracle_mod.reference_order(1):
                tabs.append(o.tables()[2])
            warn.append(o.warnings())
            pts.append(point_array(o, kw))
            lo, hi = extended_axis(o)
            T = o.T
        assert list(pts[0][1]) == list(pts[1][1]) and np.array_equal(pts[0][0][7:10], pts[1][0][7:10])   # one batch
        Aa, Ab = np.zeros((T, T)), np.zeros((T, T))
        wa, wb = ctypes.c_int(-1), ctypes.c_int(-1)
        H.hc_alpha_two_ref.restype = ctypes.c_int
        nf = H.hc_alpha_two_ref(_dp(pts[0][0]), _dp(pts[1][0]), pts[0][1], T, _dp(lo), _dp(hi), _dp(Aa), _dp(Ab),
                                ctypes.byref(wa), ctypes.byref(wb))
        _two_cache[pair] = (Aa, Ab, wa.value, wb.value, nf, tabs[0], tabs[1], warn)
    return _two_cache[pair]


@pytest.mark.parametrize("pair", TWO_PAIRS)
def test_alpha_k_two_bit_identical(oracle_mod, pair):
    """alpha_k_two (k_alpha_batch's staged chunks: two points of a batch through one entry's combine, the batch's
    shared brackets formed from ANOTHER point's leaves -- here from a's, for both) on the host, leaves evaluated on the
    spot: both tables against the reference-order oracle's alpha of a and of b bit for bit, both warning words'
    kWarnAlpha bit against the oracle's (the predicate: on the GPU no scanned batch raises it, so the routing of the
    second point's word is pinned nowhere else).  The pairs differ in g, in the flavour row, in both (and si, norm),
    not at all, and one pair has the nearly massless lightest state of cases.mixed_batch_groups()'s group E (the
    Taylor branch of alpha_s, negative entries)."""
    Aa, Ab, wa, wb, nf, ala, alb, warn = _two_run(oracle_mod, pair)
    assert nf >= 0
    iu = np.triu_indices(Aa.shape[0], 1)
    assert np.array_equal(Aa[iu], ala[iu]), "a: %d alpha entries differ" % np.sum(Aa[iu] != ala[iu])
    assert np.array_equal(Ab[iu], alb[iu]), "b: %d alpha entries differ" % np.sum(Ab[iu] != alb[iu])
    assert (wa & 4) == (warn[0] & 4) and (wb & 4) == (warn[1] & 4)
    assert (wa & ~4) == 0 and (wb & ~4) == 0   # (alpha_k_two raises no other bit)


def test_alpha_k_two_fallback_fired(oracle_mod):
    """At least one of the pairs reaches alpha_k_two's shared fallback (a.at < 0 || b.at < 0: one gl33_rect
    quadrature serving both points); without it that call is not exercised.  (The massless-lightest pair takes it at
    908 (entry, k); the mntot = 0.1 pairs never do.)"""
    nf = {pair: _two_run(oracle_mod, pair)[4] for pair in TWO_PAIRS}
    assert max(nf.values()) > 0, nf


@pytest.mark.parametrize("parts", [1, 2])
@pytest.mark.parametrize("ref", [0, 1])
@pytest.mark.parametrize("name", sorted(cases.SMALL_CASES))
def test_edge_shared_gamma_alphat_bit_identical(oracle_mod, name, ref, parts):
    """k_gamma_alphat's edge-shared path (round 6: each bin edge's dilogarithms evaluated once and handed to the
    neighbouring bin; gamma_edge_vals / alphat_edge_vals + the *_pre differences), emulated on the host in both
    channel splits, against the oracle in both arithmetics: Gamma and alphaTilde bit for bit."""
    from tests.hostcheck import build_hostcheck
    H = build_hostcheck()
    kw = dict(cases.SMALL_CASES[name], N_bins_E=40)
    o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
    with oracle_mod.reference_order(ref):
        G, aT, _ = o.tables()
    lo, hi = extended_axis(o)
    pt, flags = point_array(o, kw)
    T = o.T
    Gh, aTh = np.zeros(T), np.zeros(T)
    H.hc_ga_shared.restype = ctypes.c_int
    H.hc_ga_shared(_dp(pt), flags, T, _dp(lo), _dp(hi), parts, ref, _dp(Gh), _dp(aTh))
    assert np.array_equal(Gh, G), "Gamma differs at %s" % np.flatnonzero(Gh != G)[:5]
    assert np.array_equal(aTh, aT), "alphaTilde differs at %s" % np.flatnonzero(aTh != aT)[:5]


@pytest.mark.parametrize("name", sorted(cases.SMALL_CASES) + ["C2A", "C2B"])
def test_ga_dilogs_prepass_bit_identical(oracle_mod, name):
    """The reference order's few-table path (round 6): k_ga_dilogs evaluates every GSL dilogarithm of
    Gamma / alphaTilde one per work-item (ga_pre_slot: both edges' values and alphaTilde's bin values d26, d43 and the
    t-u combination's four), k_gamma_alphat<.., kPre> reads them (ga_pre_load) -- emulated on the host: Gamma and
    alphaTilde bit for bit against the reference-order oracle (the fields start as NaN, so a field no slot writes would
    show).  BASELINE configs 2a / 2b at their own N_E = 300, the small cases at 40 bins."""
    from tests.hostcheck import build_hostcheck
    H = build_hostcheck()
    kw = getattr(cases, name) if name in ("C2A", "C2B") else dict(cases.SMALL_CASES[name], N_bins_E=40)
    o = oracle_mod.Oracle(**cases.oracle_kwargs(kw))
    with oracle_mod.reference_order(1):
        G, aT, _ = o.tables()
    lo, hi = extended_axis(o)
    pt, flags = point_array(o, kw)
    T = o.T
    Gh, aTh = np.zeros(T), np.zeros(T)
    H.hc_ga_pre.restype = ctypes.c_int
    H.hc_ga_pre(_dp(pt), flags, T, _dp(lo), _dp(hi), _dp(Gh), _dp(aTh))
    assert np.array_equal(Gh, G), "Gamma differs at %s" % np.flatnonzero(Gh != G)[:5]
    assert np.array_equal(aTh, aT), "alphaTilde differs at %s" % np.flatnonzero(aTh != aT)[:5]
