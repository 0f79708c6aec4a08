"""Register, LDS and scratch figures of k_detector_fit in the shipped libnusi.so (CPU; reads the gfx950 code object's
metadata through tests/test_detector_resources.py's fixture).

One instance per number of components NC = 1 + K = 2, 3, 4.  A lane iterates ONE spectrum: its bin of the signal, of
the K templates, of the background and the data, NC iterates, candidates and directions, and a round's
NC + NC (NC + 1) / 2 sums (14 at NC = 4) with the L D L^T solve and its fp64 divisions inline.  It must stay out of
scratch and within 128 VGPRs (4 waves per SIMD).  Its LDS is the block's mu and theta_1 .. theta_K for the statistic:
(256 >> ceil(log2 C)) rows of (C + K) | 1 doubles, largest at C = 1 ("The fit with floating
templates").
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)


def _lds_doubles(NC):
    best = 0
    for C in range(1, 65):
        lg = 0
        while (1 << lg) < C:
            lg += 1
        best = max(best, (256 >> lg) * ((C + NC - 1) | 1))
    return best


def test_fit_instances(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if re.search(r"k_detector_fitILi\dE", k)}
    assert sorted(int(re.search(r"k_detector_fitILi(\d)E", k).group(1)) for k in ks) == [2, 3, 4], sorted(ks)
    assert len([k for k in kernels if "k_detector_fit" in k]) == 3
    for k, v in ks.items():
        nc = int(re.search(r"k_detector_fitILi(\d)E", k).group(1))
        assert v.get("vgpr_spill_count", 0) == 0, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
        assert 0 < v.get("vgpr_count", 0) <= 128, (k, v)      # at least 4 waves per SIMD
        assert v.get("group_segment_fixed_size", 0) == 8 * _lds_doubles(nc), (k, v)
    assert [_lds_doubles(nc) for nc in (2, 3, 4)] == [768, 768, 1280]


def test_the_other_detector_kernels_are_not_counted_with_it(kernels):  # noqa: F811
    """The existing resource tests find their kernels by name: the new kernel's name holds none of theirs."""
    fit = [k for k in kernels if "k_detector_fit" in k]
    assert fit
    for k in fit:
        assert not re.search(r"k_detector_profile|k_detector_events|k_detector_fold", k), k
