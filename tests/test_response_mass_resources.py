"""Register figures of the mass-resolved response's kernels in the shipped libnusi.so (CPU; reads the gfx950 code
object's metadata, like tests/test_response_resources.py).

k_cascade_mass_impulse is k_cascade_bs_impulse's body with the unit source in one row (nusi_cascade_bs_body.inc,
kMass): three wave-uniform selects in the chain wave's solve.  Its name is its own, so neither the prefix patterns of
tests/test_kernel_resources.py nor tests/test_response_resources.py's count of k_cascade_bs_impulse instances see it.
It ships at the plain impulse instance's figures ("Mass-resolved response matrices"): 128 VGPRs
(4 waves per SIMD), 5 VGPR spills and 112 B of private segment in both instances (kNR = 0 / 1).  k_response_compose
is bandwidth-bound and elementwise: no scratch.
"""
import re

from tests.test_kernel_resources import _kernels   # (the metadata reader)


def test_mass_impulse_cascade_within_register_budget(tmp_path):
    all_k = _kernels(tmp_path)
    ks = {k: v for k, v in all_k.items() if re.search(r"k_cascade_mass_impulseILb[01]E", k)}
    assert len(ks) == 2, sorted(ks)
    for k, v in ks.items():
        assert v.get("vgpr_count", 0) <= 128, (k, v)
        assert v.get("vgpr_spill_count", 0) == 5, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 112, (k, v)
    # the names keep clear of the existing counts
    assert len([k for k in all_k if re.search(r"k_cascade_bs_impulseILb[01]E", k)]) == 2
    assert not any(re.search(r"k_cascade_bsI", k) for k in ks)


def test_scalar_mass_cascade_and_compose_have_no_scratch(tmp_path):
    all_k = _kernels(tmp_path)
    for pat, vmax in ((r"k_response_composeE", 64), (r"k_cascade_massE", 256)):
        ks = {k: v for k, v in all_k.items() if re.search(pat, k)}
        assert len(ks) == 1, (pat, sorted(ks))
        (name, v), = ks.items()
        assert v.get("vgpr_spill_count", 0) == 0, (name, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (name, v)
        assert 0 < v.get("vgpr_count", 0) <= vmax, (name, v)
