"""Register, LDS and scratch figures of k_conditional_fit and k_interval in the shipped libnusi.so (CPU; reads the gfx950
code object's metadata through tests/test_detector_resources.py's fixture).

k_conditional_fit<NC>, NC = K = 1, 2, 3 floated templates: k_detector_fit's chain with one component fewer in the solve and
the held signal's term of den in a register.  k_interval<NC>, NC = 1 + K = 1 .. 4: the best fit's chain (k_detector_fit's,
k_detector_profile's at NC = 1), then the search -- the conditional chain with one more sum, the best fit's theta and mu,
the outer iterate -- whose long-lived flags and uniform values are held in vector registers, because the scalar file
is the tight one there ("The conditional fit and limits on the signal scale").

No instance may touch scratch or spill a vector register: a condition.  LDS is k_detector_fit's formula: per spectrum of
the block its mu and theta_1 .. theta_K, (256 >> ceil(log2 C)) rows of (C + K) | 1 doubles, the largest over C.  The VGPR
counts are pinned at what the build reaches, with the waves per SIMD they imply (512 / count, rounded down, at most 8):
k_interval<3> runs at three and k_interval<4> at two -- the price of carrying the best fit through the search; DESIGN.md
has the table.
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401  (the fixture)

CONDITIONAL = {1: (54, 8), 2: (78, 6), 3: (105, 4)}              # NC: (VGPRs, waves per SIMD)
INTERVAL = {1: (80, 6), 2: (117, 4), 3: (155, 3), 4: (195, 2)}
NAMES = ("k_detector_fit", "k_detector_profile", "k_detector_events", "k_detector_fold", "k_ensemble")


def _lds_doubles(K):
    best = 0
    for C in range(1, 65):
        lg = 0
        while (1 << lg) < C:
            lg += 1
        best = max(best, (256 >> lg) * ((C + K) | 1))
    return best


def _instances(kernels, name):
    ks = {int(re.search(name + r"ILi(\d)E", k).group(1)): v for k, v in kernels.items() if name in k}
    assert len(ks) == len([k for k in kernels if name in k])
    return ks


def _held(v, vgprs, waves, lds):
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, v
    assert v.get("vgpr_count", 0) == vgprs and min(8, 512 // vgprs) == waves, v
    assert v.get("group_segment_fixed_size", 0) == lds, v


def test_conditional_fit_instances(kernels):  # noqa: F811
    ks = _instances(kernels, "k_conditional_fit")
    assert sorted(ks) == [1, 2, 3]
    for nc, v in ks.items():
        _held(v, CONDITIONAL[nc][0], CONDITIONAL[nc][1], 8 * _lds_doubles(nc))


def test_interval_instances(kernels):  # noqa: F811
    ks = _instances(kernels, "k_interval")
    assert sorted(ks) == [1, 2, 3, 4]
    for nc, v in ks.items():
        _held(v, INTERVAL[nc][0], INTERVAL[nc][1], 8 * _lds_doubles(nc - 1))
    assert [_lds_doubles(k) for k in (0, 1, 2, 3)] == [384, 768, 768, 1280]


def test_the_existing_kernels_are_not_counted_with_them(kernels):  # noqa: F811
    """The existing resource tests find their kernels by name: the new kernels' names hold none of theirs."""
    new = [k for k in kernels if "k_conditional_fit" in k or "k_interval" in k]
    assert len(new) == 7
    for k in new:
        assert not any(n in k for n in NAMES), k
