"""nusiprop_amd.sources (numpy only) and the C ABI's tabulated-source entry points (CPU: no compute calls).

The bound on bin_integrals is the issue's: order-12 Gauss-Legendre against the closed form, <= 1e-13 relative on bins
of ratio up to 10^(5/24) for gamma in [2, 3] (E^-gamma over such a bin is analytic with its nearest singularity, E = 0,
2.6 half-widths from the bin's centre at the widest ratio: the 12-point rule's error is far below an ulp; what is left
is the closed form's own cancellation, ~eps / (1 - r^(1-gamma))).
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from nusiprop_amd import sources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nusi.h")
NEW = ["nusi_plan_source_axis", "nusi_plan_set_source", "nusi_source_axis", "nusi_set_source"]


def _edges(N, lEmin=12.0, lEmax=17.0):
    e = 10.0 ** (lEmin + (lEmax - lEmin) * np.arange(N + 1) / N)
    return e[:-1], e[1:]


@pytest.mark.parametrize("N", [300, 37, 24])          # bin ratios 10^(1/60), 10^(5/37), 10^(5/24)
@pytest.mark.parametrize("si", [2.0, 2.25, 2.5, 3.0])
def test_bin_integrals_match_closed_form(N, si):
    lo, hi = _edges(N)
    exact = sources.power_law_integrals(lo, hi, si)
    quad = sources.bin_integrals(lambda E: (E / 1e14) ** (-si), lo, hi, order=12)
    err = float(np.max(np.abs(quad - exact) / exact))
    print("N=%d si=%g: bin_integrals vs closed form %.2e" % (N, si, err))
    assert np.all(exact > 0)
    assert err <= 1e-13


def test_power_law_integrals_closed_form():
    lo, hi = np.array([1e12, 2e14]), np.array([3e12, 5e14])
    for si in (2.0, 2.7):
        want = [(h * (h / 1e14) ** (-si) - l * (l / 1e14) ** (-si)) / (1 - si) for l, h in zip(lo, hi)]
        assert np.array_equal(sources.power_law_integrals(lo, hi, si), np.array(want))
    # another pivot rescales the spectrum
    a = sources.power_law_integrals(lo, hi, 2.5, E0=1e13)
    b = sources.power_law_integrals(lo, hi, 2.5)
    assert np.allclose(a / b, 10.0 ** (-2.5), rtol=1e-13)


def test_tabulated_value():
    from nusiprop_amd import _lib
    assert sources.tabulated(0) == 2 == _lib.SOURCE_TABULATED == sources.SOURCE_TABULATED
    assert sources.tabulated(5) == 7
    assert sources.tabulated(1023) == _lib.SOURCE_TABULATED + 1023
    with pytest.raises(ValueError):
        sources.tabulated(-1)


def test_factories_continuous_at_break():
    Eb = 3e15
    f = sources.broken_power_law(2.0, 3.0, Eb)
    below, above = float(f(Eb * (1 - 1e-13))), float(f(Eb * (1 + 1e-13)))
    assert abs(below - above) <= 1e-12 * above            # (the slopes move it by <= 3e-13 over that step)
    assert float(f(Eb)) == pytest.approx((Eb / 1e14) ** -2.0, rel=1e-14)
    E = np.array([1e13, 1e15, 1e16, 1e17])
    assert np.allclose(f(E[:2]), (E[:2] / 1e14) ** -2.0, rtol=1e-14)       # the lower law below the break
    assert np.allclose(f(E[2:]) / f(E[2:3]), (E[2:] / E[2]) ** -3.0, rtol=1e-13)   # the upper law's slope above it
    c = sources.exp_cutoff(2.5, 1e16)
    assert np.allclose(c(E), (E / 1e14) ** -2.5 * np.exp(-E / 1e16), rtol=1e-14)
    assert float(c(1e6)) == pytest.approx((1e6 / 1e14) ** -2.5, rel=1e-9)   # far below the cutoff: the power law
    assert np.all(np.diff(c(E)) < 0)


def test_spectrum_and_weight_vectors():
    lo, hi = _edges(24)
    z = np.linspace(0.0, 5.0, 7)
    S = sources.power_law_integrals(lo, hi, 2.5)
    assert np.array_equal(sources.spectrum_vector(S, lo, hi), S)
    assert np.array_equal(sources.spectrum_vector(lambda E: (E / 1e14) ** -2.5, lo, hi),
                          sources.bin_integrals(lambda E: (E / 1e14) ** -2.5, lo, hi))
    assert sources.weight_vector(None, z) is None
    assert np.array_equal(sources.weight_vector(lambda v: (1 + v) ** 3, z), np.array([(1 + float(v)) ** 3 for v in z]))
    assert np.array_equal(sources.weight_vector(list(z), z), z)
    with pytest.raises(ValueError):
        sources.spectrum_vector(S[:-1], lo, hi)
    with pytest.raises(ValueError):
        sources.weight_vector(z[:-1], z)


# --- the C ABI's new entry points: the header, the binding list and the library agree (tests/test_capi.py's approach)
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
    m = re.search(r"#define\s+NUSI_SOURCE_TABULATED\s+(\d+)", _header_text())
    assert m and int(m.group(1)) == lib.SOURCE_TABULATED
    m = re.search(r"#define\s+NUSI_SOURCE_SLOTS_MAX\s+(\d+)", _header_text())
    assert m and int(m.group(1)) == lib.SOURCE_SLOTS_MAX >= 1024


def test_library_exports_and_binds_the_entry_points(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = lib.load()
    dp, ip, vp, i = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_void_p, ctypes.c_int
    want = {"nusi_plan_source_axis": [vp, ip, dp, dp, dp], "nusi_plan_set_source": [vp, i, dp, dp],
            "nusi_source_axis": [vp, ip, dp, dp, dp], "nusi_set_source": [vp, dp, dp]}
    for f in NEW:
        assert f in exported, f
        fn = getattr(L, f)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want[f], f


def test_params_struct_layout_unchanged(lib):
    """The slot rides in source_model: struct nusi_params keeps its fields (the last one is source_model, an int)."""
    names = [n for n, _ in lib.NusiParams._fields_]
    assert names[-1] == "source_model" and len(names) == 15
    body = re.search(r"typedef struct nusi_params \{(.*?)\} nusi_params;", _header_text(), flags=re.S).group(1)
    fields = re.findall(r"\b(?:double|int)\s+(\w+)\s*;", body)
    assert fields == names
