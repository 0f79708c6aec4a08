"""Register, LDS and scratch figures of k_detector_profile in the shipped libnusi.so (CPU; reads the gfx950 code
object's metadata through tests/test_detector_resources.py's fixture).

The kernel holds, per lane, four signals, four sums S1, four iterates and the eight terms of a step's two sums, and
runs its fp64 divisions inline: it must stay out of scratch and within 128 VGPRs (4 waves per SIMD).  Its LDS is the
block's mu for the statistic, the events kernel's 12 KiB ("The profiled statistic").
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)


def test_profile_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if re.search(r"k_detector_profile", k)}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0, v
    assert v.get("private_segment_fixed_size", 0) == 0, v
    assert 0 < v.get("vgpr_count", 0) <= 128, v       # at least 4 waves per SIMD
    assert v.get("group_segment_fixed_size", 0) == 8 * 1536, v       # the largest block of mu: C = 2, 512 x 3
