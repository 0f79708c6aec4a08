"""Response matrices, the CPU side: response.apply_host (the yardstick of nusi_plan_response_apply) and the ABI's new
entry points -- header, binding list and library agree (tests/test_sources.py's approach).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nusiprop_amd import response

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nusi.h")
NEW = ["nusi_plan_response", "nusi_plan_response_host", "nusi_plan_response_apply", "nusi_plan_response_apply_host",
       "nusi_response"]


def _random_case(seed, ntab, M, N, Q):
    rng = np.random.default_rng(seed)
    G = rng.random((ntab, M, 3, N))
    S = rng.random((Q, M))
    return G, S, rng.random(Q) + 0.5


def test_apply_host_against_einsum():
    """Random non-negative data: every term has one sign, so the two summation orders agree to M ulps of the sum
    (M = 40: <= 40 * 1.1e-16 < 1e-14)."""
    G, S, sc = _random_case(1, 3, 40, 7, 5)
    want = np.einsum("tnkb,qn->tqkb", G[:, 1:], S[:, 1:])
    got = response.apply_host(G, S)
    assert got.shape == (3, 5, 3, 7)
    assert np.max(np.abs(got - want) / want) <= 1e-14
    got = response.apply_host(G, S, scale=sc)
    assert np.max(np.abs(got - sc[None, :, None, None] * want) / want) <= 1e-14
    # the squeezed forms: one table, one spectrum vector
    assert np.array_equal(response.apply_host(G[1], S[2]), response.apply_host(G, S)[1, 2])
    assert np.array_equal(response.apply_host(G[1], S), response.apply_host(G, S)[1])
    assert np.array_equal(response.apply_host(G, S[2], scale=3.0), 3.0 * response.apply_host(G, S)[:, 2])
    with pytest.raises(ValueError):
        response.apply_host(G, S[:, :-1])


def test_apply_host_is_the_scalar_loop():
    """Bit for bit the defined sum: acc = 0.0; for n = 1 .. M-1 ascending acc = acc + G[n] * S[n] (Python floats: each
    product and each sum rounded once); then scale * acc.  Bin 0 of the source axis is never read."""
    G, S, sc = _random_case(2, 2, 9, 4, 3)
    S[1, 3] = 0.0
    got = response.apply_host(G, S, scale=sc)
    plain = response.apply_host(G, S)
    for t in range(2):
        for q in range(3):
            for k in range(3):
                for b in range(4):
                    acc = 0.0
                    for n in range(1, 9):
                        acc = acc + float(G[t, n, k, b]) * float(S[q, n])
                    assert plain[t, q, k, b] == acc
                    assert got[t, q, k, b] == float(sc[q]) * acc
    S2 = S.copy()
    S2[:, 0] = 1e300
    assert np.array_equal(response.apply_host(G, S2), plain)


# --- the C ABI's new entry points --------------------------------------------------------------------------------
def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.fixture(scope="module")
def lib():
    from nusiprop_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "nusiprop_amd", "csrc")])
    return _lib


def test_header_declares_and_binding_lists_the_entry_points(lib):
    declared = set(re.findall(r"\b(nusi_[a-z_0-9A-Z]+)\s*\(", _header_text()))
    for f in NEW:
        assert f in declared, f
        assert f in lib.EXPORTS, f
    m = re.search(r"#define\s+NUSI_OPT_RESPONSE_FIFO_KB\s+(\d+)", _header_text())
    assert m and int(m.group(1)) == lib.OPT_RESPONSE_FIFO_KB == 12
    opts = re.findall(r"#define\s+NUSI_OPT_\w+\s+(\d+)", _header_text())
    assert len(opts) == len(set(opts)), opts            # no option number used twice


def test_library_exports_and_binds_the_entry_points(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = lib.load()
    dp, vp, i = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_int
    pp = ctypes.POINTER(lib.NusiParams)
    want = {"nusi_plan_response": [vp, pp, i, dp, vp, vp, vp], "nusi_plan_response_host": [vp, pp, i, dp, dp, dp],
            "nusi_plan_response_apply": [vp, vp, i, dp, i, dp, vp, vp],
            "nusi_plan_response_apply_host": [vp, dp, i, dp, i, dp, dp], "nusi_response": [vp, dp, dp, dp]}
    for f in NEW:
        assert f in exported, f
        fn = getattr(L, f)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[f], f


def test_response_without_a_gpu_fails_loudly(lib):
    """Without a GPU there is no plan to hand in, and the response refuses with NUSI_EHIP -- no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = lib.load()
    h = ctypes.c_void_p()
    assert L.nusi_plan_create(0, 20, 12.0, 17.0, 5.0, 1, ctypes.byref(h)) == lib.NUSI_EHIP and not h.value
    p = lib.make_params(6e5, 0.01, 0.1, 2.5, N_bins_E=20)
    out = np.zeros(8)
    dp = ctypes.POINTER(ctypes.c_double)
    assert L.nusi_plan_response_host(h, ctypes.byref(p), 1, None, out.ctypes.data_as(dp), None) == lib.NUSI_EHIP
    assert b"HIP" in L.nusi_last_error() or b"device" in L.nusi_last_error()
    assert not out.any()
