"""Register budgets of the hot kernels in the shipped libnusi.so (CPU; reads the gfx950 code object's metadata).

A kernel that spills its MFMA accumulators to scratch still passes every parity test, but runs several times
slower: the round-3 per-stage cascade with phase 2 of the records on a push wave spilled 370 VGPRs and the C4
cascade took 2.93 ms instead of 0.706 (profiles/r3/r3f).  These bounds hold the spill counts the kernels were
measured at.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nusiprop_amd", "libnusi.so")
LLVM = "/opt/rocm/lib/llvm/bin"

# kernel-name regex -> (max VGPR spills, max private segment bytes per lane)
BUDGET = {
    r"k_alpha_batchILb[01]ELb0E": (64, 1024),  # call frames of the out-of-line per-batch phases
    # the reference-order instances: the member-corner offset and one point's prefetched corner (k_alpha_mcorner's
    # block) live across the point loop, and (non-phi-phi instance) the chunk's A inline -- faster than as a call
    # despite the spills (profiles/r5/r6p); 128 VGPRs (4 waves per SIMD; kBatchWavesRefo = 3 gives the non-phi-phi
    # instance 168, shipped since round 6: spills 82 -> 35) held by keeping the complex GSL series out of the kernel's
    # call graph (gsl_cli2_real)
    r"k_alpha_batchILb1ELb1E": (96, 1024),
    r"k_alpha_batchILb0ELb1E": (40, 256),
    # the block-synchronous cascade: 96 B of private segment are the prologue's pow() call frames (no spills)
    r"k_cascade_bsILi(16|32)ELi1ELi1ELi4ELi1E": (0, 96),
    # (the wave index is readfirstlane'd: per-wave row bases in SGPRs; as VGPRs they spilled 19 / 33 into the push)
    r"k_cascade_bsILi48ELi1ELi1ELi4ELi1ELb0E": (2, 96),
    # the all-non-resonant instance (kNR): 4 spills / 112 B, outside the MFMA loop; C4 cascade 0.477 vs 0.562 ms (r4ae)
    r"k_cascade_bsILi48ELi1ELi1ELi4ELi1ELb1E": (4, 112),
    r"k_cascade_bsILi16ELi1ELi1ELi8ELi1E": (6, 128),
    r"k_cascade_bsILi(16|32)ELi2ELi1ELi2ELi2E": (0, 96),
    # (round 6: 4 -> 6 with the cheaper log's different call frames in the prologue's pow(); C5's gamma-batch cascade
    # measured unchanged, 21.5 -> 21.6 ms, profiles/r6/r7w -> r8o)
    r"k_cascade_bsILi48ELi2ELi1ELi2ELi2E": (6, 112),
    r"k_cascade_bsILi6ELi16ELi1ELi2ELi2E": (6, 112),
}


def _kernels(tmp_path):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("libnusi.so or the ROCm LLVM tools are absent")
    fat = tmp_path / "fat.bin"
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=%s" % fat, LIB, str(tmp_path / "x")],
                   check=True, capture_output=True)
    # the linked library's section holds one offload bundle per translation unit, back to back
    blob = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)] + [len(blob)]
    notes = ""
    for i in range(len(starts) - 1):
        part, co = tmp_path / ("b%d.bin" % i), tmp_path / ("b%d.co" % i)
        part.write_bytes(blob[starts[i]:starts[i + 1]])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "-type=o",
                        "-targets=hipv4-amdgcn-amd-amdhsa--gfx950", "-input=%s" % part, "-output=%s" % co, "-unbundle"],
                       check=True, capture_output=True)
        notes += subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True,
                                capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*\.name:\s+(\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.match(r"\s*\.(vgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)", line)
        if m and cur:
            out[cur][m.group(1)] = int(m.group(2))
    return out


def test_hot_kernels_within_register_budget(tmp_path):
    ks = _kernels(tmp_path)
    assert any("k_cascade_bs" in k for k in ks), "no cascade kernels in the code object"
    # round 5: the per-stage kernels of rounds 1-3 are out of the product library
    assert not any(re.search(r"k_cascade_(ws|wsp|gb|wf|reg)I", k) for k in ks), "a superseded cascade kernel is back"
    # the retired A/B variants stay out (DESIGN.md "Retired build variants"): k_alpha_batch is <kPP, kRef, kSplit> --
    # plain and phi-phi in both arithmetics, the k-split instance of each arithmetic -- with no one-launch-per-mass-state
    # instances, and no cascade instance has the 96-row push waves (RT = 6)
    batch = sorted(k for k in ks if "k_alpha_batchI" in k)
    assert len(batch) == 6, batch
    assert not any(re.search(r"k_cascade_bsILi\d+ELi\d+ELi\d+ELi6E", k) for k in ks), "a retired cascade instance is back"
    for pat, (spill, priv) in BUDGET.items():
        hits = {k: v for k, v in ks.items() if re.search(pat, k)}
        assert hits, pat
        for k, v in hits.items():
            assert v.get("vgpr_spill_count", 0) <= spill, (k, v)
            assert v.get("private_segment_fixed_size", 0) <= priv, (k, v)
            if "k_alpha_batch" in k:   # (the launch bound batch_waves: 4 waves per SIMD; the reference order's
                # non-phi-phi instance may be built at 3, kBatchWavesRefo)
                assert v.get("vgpr_count", 0) <= (168 if "k_alpha_batchILb0ELb1E" in k else 128), (k, v)
