"""Register, LDS and scratch figures of k_components_fit<J, NC> in the shipped libnusi.so (CPU; the gfx950 code object's
metadata through tests/test_detector_resources.py's fixture).

Eight instances, J = 2 .. 3 signal components and K = NC - J = 0 .. 3 templates.  None may use scratch.  A chain holds
NC iterates, candidates and directions and a round's NC + NC (NC + 1) / 2 sums (27 at NC = 6): NC <= 4 keep the 128
registers of four waves per SIMD, NC = 5 the 168 of three, NC = 6 the 256 of two.  The ceilings are the built
allocations of DESIGN.md sec. 4's table ("Signal components: k_components_fit").  LDS: a row per spectrum of the block,
(C + NC - 1) | 1 doubles -- mu and theta_1 .. theta_{NC-1} -- at the C that needs the most.
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401 (a fixture)

NAME = "k_components_fit"
CEILING = {(2, 2): 74, (2, 3): 100, (2, 4): 126, (2, 5): 159, (3, 3): 100, (3, 4): 126, (3, 5): 159, (3, 6): 197}
OTHERS = ("k_detector_fold", "k_detector_events", "k_detector_profile", "k_detector_fit", "k_ensemble_profile",
          "k_ensemble_fit", "k_ensemble_best", "k_conditional_fit", "k_interval", "k_toys_limit", "k_toys_band",
          "k_poisson_draw", "k_normal_draw", "k_inject", "k_nuis_inject", "k_belt", "k_belt_accept")


def _lds_doubles(NC):
    """fit_lds_max(NC) of nusi_detector.hip: (256 >> ceil(log2 C)) rows of (C + NC - 1) | 1 doubles, the largest over C."""
    best = 0
    for C in range(1, 65):
        lg = 0
        while (1 << lg) < C:
            lg += 1
        best = max(best, (256 >> lg) * ((C + NC - 1) | 1))
    return best


def test_components_fit_instances(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if NAME in k}
    got = {}
    for k, v in ks.items():
        m = re.search(NAME + r"ILi(\d)ELi(\d)EE", k)
        assert m, k
        got[(int(m.group(1)), int(m.group(2)))] = v
    assert len(ks) == 8 and set(got) == set(CEILING), sorted(ks)
    for (J, NC), v in sorted(got.items()):
        print("k_components_fit<%d, %d>: %s" % (J, NC, v))
        assert v.get("vgpr_spill_count", 0) == 0, (J, NC, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (J, NC, v)
        assert 0 < v.get("vgpr_count", 0) <= CEILING[(J, NC)], (J, NC, v)
        assert v.get("vgpr_count", 0) <= (128 if NC <= 4 else 168 if NC == 5 else 256), (J, NC, v)
        assert v.get("group_segment_fixed_size", 0) == 8 * _lds_doubles(NC), (J, NC, v)


def test_the_name_stands_apart(kernels):  # noqa: F811
    """The resource tests count kernels by substring: no existing kernel's name may be part of the new one's or the
    reverse, and k_detector_fit still matches exactly three."""
    for other in OTHERS:
        assert other not in NAME and NAME not in other, other
    names = {re.sub(r"^_ZN4nusi\d+", "", k) for k in kernels if k.startswith("_ZN4nusi")}
    for k in kernels:
        if NAME in k:
            assert not any(o in k for o in OTHERS), k
        else:
            assert NAME not in k, k
    assert len(names) > 8
    assert sum(1 for k in kernels if "k_detector_fit" in k) == 3
