"""Register, LDS and scratch figures of the ensemble limit's kernels in the shipped libnusi.so (CPU; reads the gfx950
code object's metadata through tests/test_detector_resources.py's fixture).

k_toys_limit<NC>, NC = 1 + K = 1 .. 4, is k_interval<NC>'s best fit and search inside a loop over the data sets: the
front half, the templates and tree(X) stay in registers around it, the best fit's statistic is not formed, so there is
no LDS.  k_toys_band sorts a spectrum's P limits in dynamic LDS (8 bytes per slot of 2^ceil(log2 P), 32 KiB at P = 4096),
so its fixed LDS is 0 as well; it takes 10 registers, eight waves per SIMD.

No instance may touch scratch or spill a vector register: a condition.  The VGPR counts are pinned at what the build
reaches, with the waves per SIMD they imply (512 / count, rounded down, at most 8): the loop over the data sets costs
k_interval's counts (80, 117, 155, 195) a few registers more and one wave at NC = 1; DESIGN.md has the table.

The kernels' names hold neither "k_ensemble" nor "k_interval": tests/test_ensemble_resources.py and
tests/test_limit_resources.py count their kernels by those substrings.
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)

TOYS_LIMIT = {1: (91, 5), 2: (125, 4), 3: (160, 3), 4: (200, 2)}      # NC: (VGPRs, waves per SIMD)
BAND = (10, 8)                                                         # k_toys_band: (VGPRs, waves per SIMD)
OTHERS = ("k_detector_fit", "k_detector_profile", "k_detector_events", "k_detector_fold", "k_ensemble", "k_conditional_fit",
          "k_interval")


def test_toys_limit_instances(kernels):  # noqa: F811
    ks = {int(re.search(r"k_toys_limitILi(\d)E", k).group(1)): v for k, v in kernels.items() if "k_toys_limit" in k}
    assert sorted(ks) == [1, 2, 3, 4] and len([k for k in kernels if "k_toys_limit" in k]) == 4
    for nc, v in ks.items():
        vgprs, waves = TOYS_LIMIT[nc]
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, (nc, v)
        assert v.get("vgpr_count", 0) == vgprs and min(8, 512 // vgprs) == waves, (nc, v)
        assert v.get("group_segment_fixed_size", 0) == 0, (nc, v)


def test_the_band_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if "k_toys_band" in k}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, v
    assert v.get("vgpr_count", 0) == BAND[0] and min(8, 512 // BAND[0]) == BAND[1], v
    assert v.get("group_segment_fixed_size", 0) == 0, v             # the keys live in dynamic LDS


def test_the_existing_tests_do_not_count_the_new_kernels(kernels):  # noqa: F811
    new = [k for k in kernels if "k_toys" in k]
    assert len(new) == 5, sorted(new)
    for k in new:
        assert not any(n in k for n in OTHERS), k
