"""The alpha table's tile list (nusiprop_amd/csrc/nusi_alpha_tiles.hpp) on the host (CPU): tests/tilecheck/tilecheck.cpp,
a stand-alone g++ program, checks for the grids (N_E, T) = (300, 346) [C4], (45, 91), (40, 78), (31, 79), (60, 106),
(1200, 1333) and T - N = 0 .. 60 at N = 45 that every entry n < m < T is owned by exactly one (tile, thread slot),
that no side of a batched tile has more than 17 distinct edges (and every class fits its launch's LDS capacity), that
the tiles the batch kernel runs two points at a time list at most 128 entries with every list index in range, and
that C4 has 210 core + 120 + 21 workgroups per batch, none of fewer than 30 entries.  Run plain and once under
AddressSanitizer + UndefinedBehaviorSanitizer (host code: an index error in the entry list is how the paired kernel
could fault a GPU)."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "tilecheck", "tilecheck.cpp")
INC = os.path.join(os.path.dirname(HERE), "nusiprop_amd", "csrc")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:abort_on_error=0",
           UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def _run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", INC, "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "OK", r.stdout[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    c4 = [ln for ln in lines if ln.startswith("N 300 T 346:")]   # C4's census, as the program printed it
    assert len(c4) == 1
    return c4[0]


@pytest.mark.parametrize("name,flags", [("tilecheck", ["-O2"]), ("tilecheck_asan", ["-O1"] + SAN)])
def test_tile_partition(tmp_path, name, flags):
    c4 = _run(tmp_path, name, flags)
    assert "class 0 351 tiles" in c4 and "210 core, 120 core x extended, 21 extended, 0 other" in c4


def test_c4_no_workgroup_under_30_entries(tmp_path):
    """No workgroup of (300, 346) holds fewer than 30 entries: the tiles on the diagonal of the extended triangle take
    their n bins one bin below their m bins (36 entries for 8 bins; a run of 8 against itself would have 28, the last
    run of 6 bins 15)."""
    c4 = _run(tmp_path, "tilecheck", ["-O2"])
    smallest = int(c4.split("; min ")[1].split(" entries")[0])
    print("C4: the smallest workgroup holds %d entries" % smallest)
    assert smallest >= 30, c4
