"""Register, LDS and scratch figures of the detector kernels in the shipped libnusi.so (CPU; reads the gfx950 code
object's metadata, like tests/test_response_resources.py).

k_detector_fold<CT> (CT = 1 .. 4 column tiles of 16) keeps 4 CT accumulator registers (f64 x 4 each) plus the eight
staged doubles of the next K chunk per lane and must stay out of scratch; its LDS is the larger of the staged chunk
(16 rows x 130 doubles = 16 640 B) and the cross-wave reduction (3 x CT x 256 doubles).  k_detector_events holds four
accumulators per lane and 12 KiB of mu for the statistic ("The detector").
"""
import os
import re
import subprocess

import pytest

from tests.test_kernel_resources import LIB, LLVM

KEYS = "vgpr_spill_count|private_segment_fixed_size|vgpr_count|group_segment_fixed_size"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "clang-offload-bundler"))):
        pytest.skip("libnusi.so or the ROCm LLVM tools are absent")
    tmp = tmp_path_factory.mktemp("det")
    fat = tmp / "fat.bin"
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section=.hip_fatbin=%s" % fat, LIB, str(tmp / "x")],
                   check=True, capture_output=True)
    blob = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)] + [len(blob)]
    out = {}
    for i in range(len(starts) - 1):
        part, co = tmp / ("b%d.bin" % i), tmp / ("b%d.co" % i)
        part.write_bytes(blob[starts[i]:starts[i + 1]])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "-type=o",
                        "-targets=hipv4-amdgcn-amd-amdhsa--gfx950", "-input=%s" % part, "-output=%s" % co, "-unbundle"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        # one list entry ("  - .key:") per kernel, its keys in alphabetical order (so .name sits in the middle)
        for entry in re.split(r"\n  - (?=\.)", notes):
            name = re.search(r"^    \.name:\s+(\S+)", entry, flags=re.M)
            if name:
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"^    \.(%s):\s+(\d+)" % KEYS, entry, flags=re.M)}
    return out


def test_fold_instances(kernels):
    ks = {k: v for k, v in kernels.items() if re.search(r"k_detector_foldILi\dE", k)}
    assert len(ks) == 4, sorted(ks)
    for k, v in ks.items():
        ct = int(re.search(r"k_detector_foldILi(\d)E", k).group(1))
        assert v.get("vgpr_spill_count", 0) == 0, (k, v)
        assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
        # arch VGPRs + accumulators: at least 3 waves per SIMD (512 / 3 = 170) at CT = 4, 4 (128) up to CT = 2
        assert v.get("vgpr_count", 0) <= (128 if ct <= 2 else 168), (k, v)
        assert v.get("group_segment_fixed_size", 0) == 8 * max(16 * 130, 3 * ct * 256), (k, v)


def test_events_kernel(kernels):
    ks = {k: v for k, v in kernels.items() if re.search(r"k_detector_events", k)}
    assert len(ks) == 1, sorted(ks)
    (name, v), = ks.items()
    assert v.get("vgpr_spill_count", 0) == 0, v
    assert v.get("private_segment_fixed_size", 0) == 0, v
    assert v.get("vgpr_count", 0) <= 64, v            # 8 waves per SIMD
    assert v.get("group_segment_fixed_size", 0) == 8 * 1536, v       # the largest block of mu: C = 2, 512 x 3
