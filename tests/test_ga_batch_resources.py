"""Register budget of k_ga_dilogs_batch in the shipped libnusi.so (CPU; reads the gfx950 code object's metadata, as
tests/test_mcorner_resources.py does for the member-corner kernel).

The producer's work-items each walk one GSL series, so it is VALU-issue bound like k_alpha_mcorner: a VGPR spill or
SGPR lane spills would cost time that no parity test sees.  The bounds are the figures the kernel was measured at
("Gamma / alphaTilde per batch"): 84 VGPRs -- 4 waves per SIMD need at most 128 --, no VGPR spill,
no SGPR spill, and 48 B of private segment, the frame of the out-of-line GSL calls.
"""
import re

from tests.test_kernel_resources import _kernels   # (the metadata reader)
from tests.test_mcorner_resources import _sgpr_spills


def test_ga_batch_producer_within_register_budget(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if re.search(r"k_ga_dilogs_batch", k)}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0, v
    assert v.get("vgpr_count", 0) <= 128, v          # 4 waves per SIMD
    assert v.get("private_segment_fixed_size", 0) <= 48, v
    sg = _sgpr_spills(tmp_path, r"k_ga_dilogs_batch")
    assert sg and max(sg.values()) == 0, sg
