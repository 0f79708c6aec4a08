"""The job map of k_ga_dilogs_batch on the host (CPU): tests/hostcheck_ga is a stand-alone program over the producer's
own functions (ga_batch_job, ga_batch_value, ga_batch_field, ga_batch_need, ga_pre_load_batch; nusi_physics.hpp).
For table axes with shared and unshared edges and batches of nb = 1, 3, 32 and 64 tables (and 5, Dirac, resonant-only)
it runs every job of the grid and checks that every field the consumer loads was written by exactly one job, that its
value is bit-equal to ga_pre_slot's for that (point, k, bin, slot) -- one edge lies inside alphat_t's |t + 1| < 1e-7
nudge --, and that every value a bin's branches read is one a job evaluates.  The program reports per case and exits
non-zero on the first mismatches.
"""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_producer_job_map_and_values():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "hostcheck_ga")])
    r = subprocess.run([os.path.join(HERE, "_build", "hostcheck_ga")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines and all(ln.startswith("ok ") for ln in lines), r.stdout[-4000:]
    nbs = {int(m.group(1)) for m in (re.search(r" nb (\d+) ", ln) for ln in lines) if m}
    assert {1, 3, 32, 64} <= nbs, nbs
    # the cases with an edge inside the nudge window, and the resonant-only batch that needs nothing
    assert any(" nudge 1:" in ln for ln in lines)
    assert any(" nr 0 " in ln and "(0 needed)" in ln for ln in lines)
