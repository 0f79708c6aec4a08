"""Register, LDS and scratch figures of the randomised-nuisance kernels in the shipped libnusi.so (CPU; reads the gfx950
code object's metadata through tests/test_detector_resources.py's fixture).

k_nuis_inject<NC, MODE> (NC = 2 .. 4; MODE 1 = NUSI_TOYS_GLOBAL, 2 = NUSI_TOYS_PRIOR) and k_nuis_belt<NC> are k_inject<NC>
and k_belt<NC> with the toy's normal draws in front of its counts; under GLOBAL the toy's K prior means are vector values
that live across both fits (and in k_nuis_belt the K centres beside them).  k_normal_draw is the normal generator alone,
one lane a variate.

No instance may touch scratch, spill a vector register or use LDS: a condition.  The VGPR counts are pinned at what the
build reaches, with the waves per SIMD they imply (512 / count, rounded down, at most 8) -- the same waves as the FIXED
instance of the same NC in every case; DESIGN.md has the table.

The kernels' names hold none of "k_inject", "k_belt", "k_poisson_draw", "k_toys", "k_ensemble", "k_interval",
"k_conditional_fit", "k_detector_": the existing resource tests count their kernels by those substrings.
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)

NUIS_INJECT = {(2, 1): (132, 3), (3, 1): (162, 3), (4, 1): (198, 2),      # (NC, MODE): (VGPRs, waves per SIMD)
               (2, 2): (132, 3), (3, 2): (158, 3), (4, 2): (192, 2)}
NUIS_BELT = {2: (144, 3), 3: (168, 3), 4: (217, 2)}                      # NC: (VGPRs, waves per SIMD)
NORMAL = (56, 8)                                                         # k_normal_draw
OTHERS = ("k_inject", "k_belt", "k_poisson_draw", "k_toys", "k_ensemble", "k_interval", "k_conditional_fit", "k_detector_")


def _clean(v, vgprs, waves, what):
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, (what, v)
    assert v.get("vgpr_count", 0) == vgprs and min(8, 512 // vgprs) == waves, (what, v)
    assert v.get("group_segment_fixed_size", 0) == 0, (what, v)


def test_nuis_inject_instances(kernels):  # noqa: F811
    names = [k for k in kernels if "k_nuis_inject" in k]
    ks = {tuple(int(x) for x in re.search(r"k_nuis_injectILi(\d)ELi(\d)EE", k).groups()): kernels[k] for k in names}
    assert sorted(ks) == sorted(NUIS_INJECT) and len(names) == 6, sorted(names)
    for key, v in ks.items():
        _clean(v, *NUIS_INJECT[key], key)


def test_nuis_belt_instances(kernels):  # noqa: F811
    names = [k for k in kernels if "k_nuis_belt" in k]
    ks = {int(re.search(r"k_nuis_beltILi(\d)E", k).group(1)): kernels[k] for k in names}
    assert sorted(ks) == [2, 3, 4] and len(names) == 3, sorted(names)
    for nc, v in ks.items():
        _clean(v, *NUIS_BELT[nc], nc)


def test_the_normal_draw_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if "k_normal_draw" in k}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    _clean(v, *NORMAL, name)


def test_the_existing_tests_do_not_count_the_new_kernels(kernels):  # noqa: F811
    new = [k for k in kernels if "k_nuis_" in k or "k_normal_draw" in k]
    assert len(new) == 10, sorted(new)
    for k in new:
        assert not any(n in k for n in OTHERS), k
