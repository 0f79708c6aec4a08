"""Register budget of k_alpha_mcorner in the shipped libnusi.so (CPU; reads the gfx950 code object's metadata, as
tests/test_kernel_resources.py does for the batch and cascade kernels).

The kernel is VALU-issue bound, so a VGPR spill, or more SGPR lane spills (v_writelane / v_readlane are VALU work),
costs time that no parity test sees.  The bounds are the figures the kernel was measured at ("One
reciprocal per divisor"): 113 VGPRs -- 4 waves per SIMD need at most 128 --, no VGPR spill, 26 SGPR spills, and 48 B
of private segment, the frame of the call a wave outside the member window makes.
"""
import os
import re
import subprocess

from tests.test_kernel_resources import LIB, LLVM, _kernels   # (the metadata reader)


def _sgpr_spills(tmp_path, name_re):
    """.sgpr_spill_count of the kernels matching name_re (the reader above keeps the VGPR fields only)"""
    fat = tmp_path / "fat2.bin"
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=%s" % fat, LIB, str(tmp_path / "y")],
                   check=True, capture_output=True)
    blob = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    starts = [m.start() for m in re.finditer(re.escape(magic), blob)] + [len(blob)]
    out, cur = {}, None
    for i in range(len(starts) - 1):
        part, co = tmp_path / ("s%d.bin" % i), tmp_path / ("s%d.co" % i)
        part.write_bytes(blob[starts[i]:starts[i + 1]])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "-type=o",
                        "-targets=hipv4-amdgcn-amd-amdhsa--gfx950", "-input=%s" % part, "-output=%s" % co, "-unbundle"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        for line in notes.splitlines():
            m = re.match(r"\s*\.name:\s+(\S+)", line)
            if m:
                cur = m.group(1)
                continue
            m = re.match(r"\s*\.sgpr_spill_count:\s+(\d+)", line)
            if m and cur and re.search(name_re, cur):
                out[cur] = int(m.group(1))
    return out


def test_member_corner_kernel_within_register_budget(tmp_path):
    ks = {k: v for k, v in _kernels(tmp_path).items() if re.search(r"k_alpha_mcorner", k)}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0, v
    assert v.get("vgpr_count", 0) <= 128, v          # 4 waves per SIMD
    assert v.get("private_segment_fixed_size", 0) <= 48, v
    sg = _sgpr_spills(tmp_path, r"k_alpha_mcorner")
    assert sg and max(sg.values()) <= 26, sg
