"""Register, LDS and scratch figures of the ensemble kernels in the shipped libnusi.so (CPU; reads the gfx950 code
object's metadata through tests/test_detector_resources.py's fixture).

k_ensemble_profile and k_ensemble_fit<NC> (NC = 1 + K = 2, 3, 4) run the iterations of k_detector_profile and
k_detector_fit<NC> in a loop over the data sets, on those kernels' block shapes.  None may use scratch.  Four waves
per SIMD (128 registers) is the aim, as for the existing kernels, and the profile and NC = 2, 3 meet it.
k_ensemble_fit<4> does not: k_detector_fit<4> itself stands at 127, the loop over the data sets keeps a few more values
alive around the iteration, and held to 128 the compiler spills 14 registers to scratch, which is not accepted.  It is
held to three waves per SIMD (168) instead and takes 164 ("Ensembles of pseudo-experiments").

LDS: the rows of two data sets -- per spectrum of the block its mu [C], theta [W] and the status word, (C + W + 1) | 1
doubles, W = NC (the profile: 1) -- sized for the C that needs most, and the waves' records of two data sets,
2 x 4 x (W + 2) doubles: 8 (2 rows_max + 8 (W + 2)) bytes.
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)


def _rows_max(per, W):
    best = 0
    for C in range(1, 65):
        lg = 0
        while (1 << lg) < C:
            lg += 1
        best = max(best, (256 >> lg) * per * ((C + W + 1) | 1))
    return best


def _lds_bytes(per, W):
    return 8 * (2 * _rows_max(per, W) + 8 * (W + 2))


def test_ensemble_fit_instances(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if re.search(r"k_ensemble_fitILi\dE", k)}
    assert sorted(int(re.search(r"k_ensemble_fitILi(\d)E", k).group(1)) for k in ks) == [2, 3, 4], sorted(ks)
    assert len([k for k in kernels if "k_ensemble_fit" in k]) == 3
    for k, v in ks.items():
        nc = int(re.search(r"k_ensemble_fitILi(\d)E", k).group(1))
        assert v.get("vgpr_spill_count", 0) == 0, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
        # 4 waves per SIMD; NC = 4: 3 waves (512 / 3 = 170, in steps of 8), the count it has is 164
        assert 0 < v.get("vgpr_count", 0) <= (128 if nc < 4 else 168), (k, v)
        assert v.get("group_segment_fixed_size", 0) == _lds_bytes(1, nc), (k, v)
    assert [_rows_max(1, nc) for nc in (2, 3, 4)] == [1280, 1280, 1792]          # C = 1: 256 rows of 5, 5 and 7
    assert [_lds_bytes(1, nc) for nc in (2, 3, 4)] == [20736, 20800, 29056]


def test_ensemble_profile_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if "k_ensemble_profile" in k}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0, v
    assert v.get("private_segment_fixed_size", 0) == 0, v
    assert 0 < v.get("vgpr_count", 0) <= 128, v
    assert v.get("group_segment_fixed_size", 0) == _lds_bytes(4, 1) == 49344, v   # C = 1: 1024 rows of 3


def test_the_merge_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if "k_ensemble_best" in k}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, v
    assert v.get("group_segment_fixed_size", 0) == 0, v


def test_the_existing_tests_do_not_count_the_new_kernels(kernels):  # noqa: F811
    """The existing resource tests find their kernels by substring: no new name holds one of theirs."""
    new = [k for k in kernels if "k_ensemble" in k]
    assert len(new) == 5, sorted(new)
    for k in new:
        assert not re.search(r"k_detector_fit|k_detector_profile|k_detector_events|k_detector_fold", k), k
