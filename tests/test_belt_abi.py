"""The toy-calibrated interval's C surface without a GPU (nusi_plan_response_belt, _host, nusi_belt_shape).

  * the header's NUSI_BELT_* are detector.BELT_* and _lib.BELT_*;
  * the three symbols are declared in include/nusi.h, bound in _lib and exported by the library;
  * without a plan the two calls refuse;
  * nusi_belt_shape, the pure function the call applies for its size limits (no plan, no device): ntab Q G >= 2^31 is
    refused at the first such table count and one table fewer is accepted, for (Q, G) = (19, 3), (1, 1) and (2^19, 64);
    C = 0 and 65, G = 0 and 65, P = 0 and 2^26 + 1 are refused whatever the other sizes are.  The size limits are checked
    here and nowhere on the GPU: a GPU test passes its arrays' own sizes only.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from nusiprop_amd import _lib, detector

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = ("NO_GRID", "NO_FIT", "BAD_POINT", "EMPTY", "LO_EDGE", "HI_EDGE", "GAPS")
NAMES = ("nusi_belt_shape", "nusi_plan_response_belt", "nusi_plan_response_belt_host")


def test_constants():
    text = open(os.path.join(ROOT, "include", "nusi.h")).read()
    macro = {k: int(v, 0) for k, v in re.findall(r"^#define (NUSI_[A-Z_]+) (\d+)$", text, flags=re.M)}
    assert macro["NUSI_BELT_GRID_MAX"] == detector.BELT_GRID_MAX == _lib.BELT_GRID_MAX == 64
    for k, b in enumerate(BITS):
        assert macro["NUSI_BELT_" + b] == getattr(detector, "BELT_" + b) == getattr(_lib, "BELT_" + b) == 1 << k, b


def test_symbols():
    text = open(os.path.join(ROOT, "include", "nusi.h")).read()
    L = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS and re.search(r"\b%s\s*\(" % name, text) and getattr(L, name).argtypes is not None, name
    assert len(L.nusi_plan_response_belt.argtypes) == 27 and len(L.nusi_plan_response_belt_host.argtypes) == 26


def test_without_a_plan_the_calls_refuse():
    L = _lib.load()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    one, r = np.ones(4), np.zeros(4, dtype=np.int32)
    p, rp = one.ctypes.data_as(dp), r.ctypes.data_as(ip)
    refused = (_lib.NUSI_EPARAM, _lib.NUSI_EHIP)
    assert L.nusi_plan_response_belt(None, None, 1, p, 1, p, p, 1, None, 1, 1, 0, 0.1, None, None, None, None, None, None,
                                     None, None, None, None, None, None, None, None) in refused
    assert L.nusi_plan_response_belt_host(None, p, 1, p, 1, p, p, 1, None, 1, 1, 0, 0.1, p, p, rp, rp, None, None, None,
                                          None, None, None, None, None, None) in refused


def _shape(C, ntab, Q, G, P):
    units = ctypes.c_longlong(-1)
    return _lib.load().nusi_belt_shape(C, ntab, Q, G, P, ctypes.byref(units)), units.value


@pytest.mark.parametrize("Q,G", ((19, 3), (1, 1), (1 << 19, 64)))
def test_the_record_count_limit(Q, G):
    first = -(-(1 << 31) // (Q * G))                               # the first table count with ntab Q G >= 2^31
    assert first * Q * G >= 1 << 31 > (first - 1) * Q * G
    for C in (1, 17, 64):
        QB = 256 >> detector._ceil_log2(C)
        assert _shape(C, first, Q, G, 3)[0] == _lib.NUSI_EPARAM, (C, Q, G)
        if first <= 2 ** 31 - 1:                                    # (at Q G = 1 the count is no int and arrives negative)
            assert "2^31" in _lib.last_error()
        code, units = _shape(C, first - 1, Q, G, 3)
        assert code == _lib.NUSI_OK and units == (first - 1) * -(-(Q * G) // QB), (C, Q, G, units)
    assert _lib.load().nusi_belt_shape(5, first - 1, Q, G, 3, None) == _lib.NUSI_OK       # units may be NULL


def test_the_other_size_limits():
    ok = dict(C=5, ntab=3, Q=19, G=3, P=37)
    assert _shape(**ok) == (_lib.NUSI_OK, 3 * 2)                    # 57 rows a table in blocks of 32
    for key, values in (("C", (0, 65)), ("G", (0, 65)), ("P", (0, (1 << 26) + 1)), ("ntab", (0, -1)), ("Q", (0, (1 << 19) + 1))):
        for v in values:
            assert _shape(**dict(ok, **{key: v}))[0] == _lib.NUSI_EPARAM, (key, v)
    for key, v in (("C", 64), ("C", 1), ("G", 64), ("G", 1), ("P", 1 << 26), ("P", 1), ("Q", 1 << 19)):
        assert _shape(**dict(ok, **{key: v}))[0] == _lib.NUSI_OK, (key, v)
