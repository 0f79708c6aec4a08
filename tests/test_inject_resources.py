"""Register, LDS and scratch figures of the generator's and the calibration call's kernels in the shipped libnusi.so (CPU;
reads the gfx950 code object's metadata through tests/test_detector_resources.py's fixture).

k_inject<NC>, NC = 1 + K = 1 .. 4, is k_toys_limit<NC>'s loop over the toys with the sampler in front of the best fit and
one conditional fit in place of the search: no LDS.  k_poisson_draw is the sampler alone, one lane a count.

No instance may touch scratch or spill a vector register: a condition.  The VGPR counts are pinned at what the build
reaches, with the waves per SIMD they imply (512 / count, rounded down, at most 8); DESIGN.md has the table.

The kernels' names hold none of "k_toys", "k_ensemble", "k_interval", "k_conditional_fit", "k_detector_": the existing
resource tests count their kernels by those substrings.
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)

INJECT = {1: (120, 4), 2: (131, 3), 3: (158, 3), 4: (192, 2)}         # NC: (VGPRs, waves per SIMD)
DRAW = (72, 7)                                                         # k_poisson_draw
OTHERS = ("k_toys", "k_ensemble", "k_interval", "k_conditional_fit", "k_detector_")


def test_inject_instances(kernels):  # noqa: F811
    ks = {int(re.search(r"k_injectILi(\d)E", k).group(1)): v for k, v in kernels.items() if "k_inject" in k}
    assert sorted(ks) == [1, 2, 3, 4] and len([k for k in kernels if "k_inject" in k]) == 4
    for nc, v in ks.items():
        vgprs, waves = INJECT[nc]
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, (nc, v)
        assert v.get("vgpr_count", 0) == vgprs and min(8, 512 // vgprs) == waves, (nc, v)
        assert v.get("group_segment_fixed_size", 0) == 0, (nc, v)


def test_the_draw_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if "k_poisson_draw" in k}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, v
    assert v.get("vgpr_count", 0) == DRAW[0] and min(8, 512 // DRAW[0]) == DRAW[1], v
    assert v.get("group_segment_fixed_size", 0) == 0, v


def test_the_existing_tests_do_not_count_the_new_kernels(kernels):  # noqa: F811
    new = [k for k in kernels if "k_inject" in k or "k_poisson_draw" in k]
    assert len(new) == 5, sorted(new)
    for k in new:
        assert not any(n in k for n in OTHERS), k
