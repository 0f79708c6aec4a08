"""Register figures of the response kernels in the shipped libnusi.so (CPU; reads the gfx950 code object's metadata,
like tests/test_ga_batch_resources.py).

k_cascade_bs_impulse is the gamma batch's body with an impulse source (nusi_cascade_bs_body.inc); its name is its own,
so the prefix patterns of tests/test_kernel_resources.py do not see it.  It ships at the gamma-batch instance's figures
or below ("Response matrices"): 128 VGPRs (4 waves per SIMD), 5 VGPR spills and 112 B of private
segment in both instances (kNR = 0 / 1), the spills outside the MFMA loop as in k_cascade_bs<6,16,1,2,2>.
k_response_apply is bandwidth-bound and must keep its accumulators in registers: no scratch, no spill.
"""
import re

from tests.test_kernel_resources import _kernels   # (the metadata reader)


def test_impulse_cascade_within_register_budget(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if re.search(r"k_cascade_bs_impulseILb[01]E", k)}
    assert len(ks) == 2, sorted(ks)
    for k, v in ks.items():
        assert v.get("vgpr_count", 0) <= 128, (k, v)
        assert v.get("vgpr_spill_count", 0) <= 5, (k, v)
        assert v.get("private_segment_fixed_size", 0) <= 112, (k, v)


def test_response_apply_keeps_its_accumulators_in_registers(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if re.search(r"k_response_apply", k)}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0, v
    assert v.get("private_segment_fixed_size", 0) == 0, v
    assert v.get("vgpr_count", 0) <= 64, v           # 8 waves per SIMD
