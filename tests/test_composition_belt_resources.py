"""Register, LDS and scratch figures of k_composition_belt<NCF> and k_composition_accept in the shipped libnusi.so (CPU;
the gfx950 code object's metadata through tests/test_detector_resources.py's fixture).

Four instances, NCF = 3 + K = 3 .. 6.  The kernel holds the free fit of NCF components and the held fit of 1 + K across
the loop over the toys, with the four front sums, their trees, mu_inj and q_obs: none may use scratch and none uses LDS.
The figures are the built allocations of DESIGN.md sec. 4's table ("The composition region"): NCF = 3 keeps the 168
registers of three waves per SIMD, NCF = 4 and 5 the 256 of two, NCF = 6 takes 258 -- two past two waves -- and runs
one wave per SIMD (at two it spills two registers to 12 bytes of scratch).
"""
import re

from tests.test_detector_resources import kernels  # noqa: F401 (a fixture)

NAME = "k_composition_belt"
ACCEPT = "k_composition_accept"
BUILT = {3: (162, 3), 4: (194, 2), 5: (231, 2), 6: (258, 1)}      # NCF: (VGPRs with the accumulation registers, waves per SIMD)
OTHERS = ("k_detector_fold", "k_detector_events", "k_detector_profile", "k_detector_fit", "k_components_fit",
          "k_ensemble_profile", "k_ensemble_fit", "k_ensemble_best", "k_conditional_fit", "k_interval", "k_toys_limit",
          "k_toys_band", "k_poisson_draw", "k_normal_draw", "k_inject", "k_nuis_inject", "k_belt", "k_nuis_belt",
          "k_belt_accept")


def _waves(vgprs):
    """The waves per SIMD that a kernel of so many registers a lane can have: 512 a SIMD lane, allocated in blocks of 8."""
    return min(8, 512 // (8 * -(-vgprs // 8)))


def test_composition_belt_instances(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if NAME in k}
    got = {}
    for k, v in ks.items():
        m = re.search(NAME + r"ILi(\d)EE", k)
        assert m, k
        got[int(m.group(1))] = v
    assert len(ks) == 4 and set(got) == set(BUILT), sorted(ks)
    for NCF, v in sorted(got.items()):
        print("k_composition_belt<%d>: %s, %d waves per SIMD" % (NCF, v, _waves(v.get("vgpr_count", 0))))
        assert v.get("vgpr_spill_count", 0) == 0, (NCF, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (NCF, v)
        assert v.get("group_segment_fixed_size", 0) == 0, (NCF, v)
        assert 0 < v.get("vgpr_count", 0) <= BUILT[NCF][0], (NCF, v)
        assert _waves(v["vgpr_count"]) >= BUILT[NCF][1], (NCF, v)


def test_the_accept_kernel(kernels):  # noqa: F811
    ks = {k: v for k, v in kernels.items() if ACCEPT in k}
    assert len(ks) == 1, sorted(ks)
    (_, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, v
    assert v.get("group_segment_fixed_size", 0) == 0 and 0 < v.get("vgpr_count", 0) <= 64, v


def test_the_names_stand_apart(kernels):  # noqa: F811
    """The resource tests count kernels by substring: no existing kernel's name may be part of the new ones' or the
    reverse."""
    for new in (NAME, ACCEPT):
        for other in OTHERS + tuple(n for n in (NAME, ACCEPT) if n != new):
            assert other not in new and new not in other, (new, other)
    for k in kernels:
        if NAME in k or ACCEPT in k:
            assert not any(o in k.split("PK")[0] for o in OTHERS), k
    assert sum(1 for k in kernels if "k_belt" in k and "accept" not in k) == 4          # k_belt<1 .. 4> as before
    assert sum(1 for k in kernels if "k_components_fit" in k) == 8
