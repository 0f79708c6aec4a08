"""Register figures of k_alpha_mcorner with atan2's first-range vote (CPU; the shipped libnusi.so's metadata, read as
tests/test_mcorner_resources.py reads it, whose bounds -- 128 VGPRs, 26 SGPR lane spills -- stay the budget).

With the waves that fail a vote of atan2 calling nm::atan2_slow, a site keeps only the short first-range body inline:
the kernel was measured at 97 VGPRs and 18 SGPR lane spills ("A first-range vote in atan2").  The
form with both bodies inline at every site had 113 VGPRs and 42 SGPR lane spills -- v_writelane / v_readlane are VALU
work in a VALU-issue-bound kernel.  The bounds here sit between the two forms, not on the measured figures: 104 VGPRs
and 22 spills leave a compiler update room to move a few registers, and still tell the forms apart.
"""
import re

from tests.test_kernel_resources import _kernels
from tests.test_mcorner_resources import _sgpr_spills


def test_member_corner_kernel_keeps_the_vote_forms_registers(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if re.search(r"k_alpha_mcorner", k)}
    assert len(ks) == 1, sorted(ks)
    (_, v), = ks.items()
    assert v.get("vgpr_count", 0) <= 104, v
    sg = _sgpr_spills(tmp_path, r"k_alpha_mcorner")
    assert sg and max(sg.values()) <= 22, sg
