"""Register, LDS and scratch figures of the toy-calibrated interval's kernels in the shipped libnusi.so (CPU; reads the
gfx950 code object's metadata through tests/test_detector_resources.py's fixture).

k_belt<NC>, NC = 1 + K = 1 .. 4, is k_inject<NC>'s loop over the toys with one pass against the data in front, on records
(table, spectrum, grid point): no LDS.  k_belt_accept is one lane a (table, spectrum) pair.

No instance may touch scratch, spill a vector register or use LDS: conditions.  The VGPR counts are pinned at what the
build reaches; the waves per SIMD they imply (512 / count, rounded down, at most 8) are at least k_inject<NC>'s 4, 3, 3,
2.  DESIGN.md has the table.

The kernels' names hold none of "k_inject", "k_poisson_draw", "k_toys", "k_ensemble", "k_interval", "k_conditional_fit",
"k_detector_": the existing resource tests count their kernels by those substrings.
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)

BELT = {1: (126, 4), 2: (140, 3), 3: (168, 3), 4: (204, 2)}            # NC: (VGPRs, waves per SIMD)
INJECT_WAVES = {1: 4, 2: 3, 3: 3, 4: 2}                                # k_inject<NC>'s (tests/test_inject_resources.py)
OTHERS = ("k_inject", "k_poisson_draw", "k_toys", "k_ensemble", "k_interval", "k_conditional_fit", "k_detector_")


def _clean(v):
    return (v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0
            and v.get("group_segment_fixed_size", 0) == 0)


def test_belt_instances(kernels):  # noqa: F811
    names = [k for k in kernels if "k_beltILi" in k]
    ks = {int(re.search(r"k_beltILi(\d)E", k).group(1)): kernels[k] for k in names}
    assert sorted(ks) == [1, 2, 3, 4] and len(names) == 4, sorted(names)
    for nc, v in ks.items():
        vgprs, waves = BELT[nc]
        assert _clean(v), (nc, v)
        assert v.get("vgpr_count", 0) == vgprs and min(8, 512 // vgprs) == waves >= INJECT_WAVES[nc], (nc, v)


def test_the_accept_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if "k_belt_accept" in k}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert _clean(v) and min(8, 512 // max(v.get("vgpr_count", 0), 1)) == 8, v


def test_the_existing_tests_do_not_count_the_new_kernels(kernels):  # noqa: F811
    new = [k for k in kernels if "k_belt" in k]
    assert len(new) == 5, sorted(new)
    for k in new:
        assert not any(n in k for n in OTHERS), k
