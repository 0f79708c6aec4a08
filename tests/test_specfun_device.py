"""The special functions one at a time (nusi_debug_specfun.hpp) on the host build, against the oracle, bit for bit, on the
vectors of tests/specfun_cases.py -- the vectors and references tests/test_specfun_device_gpu.py runs on gfx950.

For every function: the vector set reaches every branch the numpy restatement of its source distinguishes (asserted
first), and the host twin hc_specfun_n equals the oracle's function (ora_log .. ora_pow, ora_li2, ora_li3,
ora_complex_dilog_xy, ora_gsl_dilog, ora_gsl_clausen, ora_hypot, ora_gsl_complex_dilog_xy; for the member chains Smith's
division restated in numpy into the oracle's GSL dilogarithm) on every vector: NaN equals NaN, everything else as 64-bit
patterns, the sign of zero included.  Zero mismatches, nothing left out -- which also shows that the vector set is one
the reference handles.  The wave layouts of the GPU test are checked for their shape here.
"""
import ctypes

import numpy as np
import pytest

from tests import specfun_cases as sc

NAMES = list(sc.FN)


@pytest.fixture(scope="module")
def olib(oracle_mod):
    return sc.bind_oracle(oracle_mod.lib())


@pytest.fixture(scope="module")
def hlib():
    from tests.hostcheck import build_hostcheck
    H = build_hostcheck()
    H.hc_specfun_n.restype = ctypes.c_int
    H.hc_specfun_n.argtypes = [ctypes.c_int, ctypes.c_int] + [sc.DP] * 5
    return H


def host(H, name, a, b, c):
    o0, o1 = np.empty_like(a), np.empty_like(a)
    rc = H.hc_specfun_n(sc.FN[name], a.size, *(v.ctypes.data_as(sc.DP) for v in (a, b, c, o0, o1)))
    assert rc == 0, rc
    return o0, o1


def test_numbers_match_header():
    assert sc.header_numbers() == sc.FN
    assert set(sc.CLASSES) == set(sc.FN) and set(sc.VOTED) <= set(sc.FN)


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_bit_identical_to_oracle(olib, hlib, name):
    counts, unknown = sc.class_counts(name)
    assert not unknown, unknown
    assert all(v > 0 for v in counts.values()), counts   # every branch receives arguments, before anything is compared
    a, b, c = sc.vectors(name)
    r0, r1 = sc.reference(name, olib, a, b, c)
    h0, h1 = host(hlib, name, a, b, c)
    bad = np.flatnonzero(~(sc.same_bits(h0, r0) & sc.same_bits(h1, r1)))
    assert bad.size == 0, (name, bad.size, [(a[i], b[i], c[i], h0[i].hex(), r0[i].hex(), h1[i].hex(), r1[i].hex()) for i in bad[:4]])


@pytest.mark.parametrize("name", sc.VOTED)
def test_layouts_shape(name):
    """The wave layouts: one probe set of 64 arguments per class, each probe of its class; (a) to (e) all present, every
    wave 64 lanes, the whole within one launch's bound; the same on a second call."""
    P = sc.probes(name)
    cls = sc.classify(name, *sc.vectors(name))
    for k, idx in P.items():
        assert idx.size == 64 and (cls[idx] == k).all(), k
    L = sc.layouts(name)
    K = len(P)
    kinds = {t: sum(1 for l, _, _ in L if l.startswith(t + ":")) for t in "abcde"}
    assert kinds["a"] == K and kinds["b"] == K * (K - 1) and kinds["c"] == 3 * K * (K - 1) and kinds["d"] >= 2
    assert kinds["e"] == 4 * (K + 2)
    assert all(w.size == 64 and m.size == 64 for _, w, m in L)
    for tail in (1, 37):
        idx, act, labels = sc.layout_arrays(name, tail)
        assert idx.size == 64 * len(L) + tail and act.size == idx.size and len(labels) == len(L) + 1
    again = sc.layouts(name)
    assert all(l == m and np.array_equal(u, v) for (l, u, _), (m, v, _) in zip(L, again))
