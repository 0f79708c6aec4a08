"""The special functions one at a time on gfx950, against the oracle, bit for bit, in every wave mix.

The test-only kernel k_debug_specfun<FN> (nusi_debug_specfun.hip, entry nusi_debug_specfun, bound here with ctypes; not
in nusi.h) runs one function of nusi_debug_specfun.hpp on arrays of arguments: element i is lane i % 64 of wave i / 64,
and a lane with active[i] == 0 skips the call inside a divergent branch (exec off) and keeps the sentinel the entry
filled in.  Under __HIP_DEVICE_COMPILE__ these functions run paths the host build never compiles -- cseries' instance by
__ballot, the series' first loops leaving on wave votes, hypot's voted common case, the v_rcp_f64 short division
under div_vote, atan2's votes, the member chain's fallback for a wave with a lane outside the window -- so the
property they rest on is checked here: a lane's bits depend neither on which lanes share its wave nor on which are
active.

* every function, every vector of tests/specfun_cases.py (the set tests/test_specfun_device.py holds the host twin
  to), fully active and with alternate lanes off;
* every function with a vote or ballot in its call graph, one probe set of 64 arguments per branch class in the
  layouts (a) one class alone, (b) every ordered pair 32 + 32, (c) one lane of A at lane 0, 31, 63 in a wave of B,
  (d) seeded shuffles, (e) partly active waves (lane 0, lane 63, alternate lanes; a last wave of 1 and of 37 elements).

Each active element equals the oracle's bits for its argument (NaN equals NaN; the sign of zero counts), each inactive
one is the sentinel, and -- a second assertion, which names the property -- each probe argument's bits are the same in
every layout.  No tolerance and no exclusion.
"""
import ctypes

import numpy as np
import pytest

from tests import specfun_cases as sc

pytestmark = pytest.mark.gpu

NAMES = list(sc.FN)
IP = ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def dev():
    import nusiprop_amd
    from nusiprop_amd import _lib
    nusiprop_amd.load()
    L = ctypes.CDLL(_lib.LIB_PATH)
    L.nusi_debug_specfun.restype = ctypes.c_int
    L.nusi_debug_specfun.argtypes = [ctypes.c_int] + [sc.DP] * 3 + [IP, ctypes.c_int] + [sc.DP] * 2
    return L


@pytest.fixture(scope="module")
def ref(oracle_mod):
    """name -> the oracle's (o0, o1) on vectors(name), computed once per function and left unchanged"""
    L = sc.bind_oracle(oracle_mod.lib())
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = sc.reference(name, L, *sc.vectors(name))
            for v in cache[name]:
                v.setflags(write=False)
        return cache[name]
    return get


def run(L, name, idx, active):
    a, b, c = (np.ascontiguousarray(v[idx]) for v in sc.vectors(name))
    act = np.ascontiguousarray(active, dtype=np.int32)
    o0, o1 = np.zeros(idx.size), np.zeros(idx.size)
    rc = L.nusi_debug_specfun(sc.FN[name], *(v.ctypes.data_as(sc.DP) for v in (a, b, c)), act.ctypes.data_as(IP), idx.size,
                              o0.ctypes.data_as(sc.DP), o1.ctypes.data_as(sc.DP))
    assert rc == 0, (name, rc)
    return o0, o1


def _hex(v):
    return "%016x" % int(sc.bits(np.array([v]))[0])


def check(name, what, idx, active, o0, o1, r0, r1, labels=None):
    a, b, c = sc.vectors(name)
    off = ~active
    kept = (sc.bits(o0[off]) == sc.SENTINEL) & (sc.bits(o1[off]) == sc.SENTINEL)
    assert kept.all(), "%s %s: %d inactive elements lost the sentinel, first element %d" % (
        name, what, int((~kept).sum()), int(np.flatnonzero(off)[np.flatnonzero(~kept)[0]]))
    ok = sc.same_bits(o0, r0[idx]) & sc.same_bits(o1, r1[idx])
    bad = np.flatnonzero(active & ~ok)
    rows = []
    for i in bad[:4]:
        j = idx[i]
        rows.append("element %d (%s, lane %d): args (%s, %s, %s) device (%s, %s) oracle (%s, %s)" % (
            i, labels[i // 64] if labels else "wave %d" % (i // 64), i % 64, float(a[j]).hex(), float(b[j]).hex(),
            float(c[j]).hex(), _hex(o0[i]), _hex(o1[i]), _hex(r0[j]), _hex(r1[j])))
    if labels and bad.size:
        rows.append("layouts with a mismatch: %s" % sorted({labels[i // 64] for i in bad})[:40])
    assert bad.size == 0, "%s %s: %d active elements differ from the oracle\n%s" % (name, what, bad.size, "\n".join(rows))


@pytest.mark.parametrize("name", NAMES)
def test_vectors_bit_identical_to_oracle(dev, ref, name):
    """Every vector of the function, all lanes active; then with the odd lanes off."""
    r0, r1 = ref(name)
    idx = np.arange(r0.size)
    for what, active in (("all lanes", np.ones(idx.size, bool)), ("even lanes", idx % 2 == 0)):
        o0, o1 = run(dev, name, idx, active)
        check(name, "vectors, " + what, idx, active, o0, o1, r0, r1)


@pytest.mark.parametrize("name", sc.VOTED)
def test_wave_layouts_bit_identical_to_oracle(dev, ref, name):
    """The probe sets in every wave layout: the oracle's bits in each, and the same bits in all."""
    r0, r1 = ref(name)
    a, b, c = sc.vectors(name)
    seen, moved = {}, []
    for tail in (1, 37):
        idx, active, labels = sc.layout_arrays(name, tail)
        assert idx.size % 64 == tail
        o0, o1 = run(dev, name, idx, active)
        # each probe argument's bits across all layouts (both launches): the first occurrence against every other
        for i in np.flatnonzero(active):
            j = int(idx[i])
            first = seen.setdefault(j, (o0[i], o1[i], labels[i // 64], i % 64))
            if not (sc.same_bits(np.array(first[:2]), np.array([o0[i], o1[i]])).all()):
                moved.append("args (%s, %s, %s) gave (%s, %s) in %s lane %d and (%s, %s) in %s lane %d" % (
                    float(a[j]).hex(), float(b[j]).hex(), float(c[j]).hex(), _hex(first[0]), _hex(first[1]), first[2], first[3],
                    _hex(o0[i]), _hex(o1[i]), labels[i // 64], i % 64))
        check(name, "layouts (last wave of %d)" % tail, idx, active, o0, o1, r0, r1, labels)
    assert not moved, "%s: a lane's bits depend on the lanes that share its wave, %d times; first\n%s" % (
        name, len(moved), "\n".join(moved[:4]))
    assert set(np.concatenate(list(sc.probes(name).values())).tolist()) == set(seen)   # (every probe was visited)
