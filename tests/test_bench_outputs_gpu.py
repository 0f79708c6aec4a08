"""bench.py's plain run and --dump-outputs on the GPU: one child process runs a 24-point C4 block for 3 timed
steps; the line has the headline fields and none of what --full adds, and DIR/flux.npy / DIR/fla.npy hold what
Plan.evolve computes for the same points (same library, same kernels: the parity tests' flux bound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = 24


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("bench_dump"))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--points", str(POINTS), "--dump-outputs", d], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=110)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(lines[0]), d


def test_plain_line(plain_run):
    j, _ = plain_run
    assert j["steps"] == 3 and j["warmup"] == 1 and j["unit"] == "propagations/s" and j["dtype"] == "f64"
    assert j["higher_is_better"] is True and j["invalid_outputs"] == 0 and not j["full"]
    assert j["ms_per_step"] > 0
    assert abs(j["value"] - POINTS / (j["ms_per_step"] * 1e-3)) <= 1e-9 * j["value"]   # value = points per step time
    for k in ("parity", "cpu_baseline", "secondary_lines", "single_propagation"):
        assert k not in j
    assert j["dump_outputs"]["points"] == POINTS and not j["dump_outputs"]["sampled"]


def test_dumped_outputs_are_the_plans(plain_run):
    import nusiprop_amd as nu
    from nusiprop_amd import scan
    _, d = plain_run
    flux, fla = np.load(os.path.join(d, "flux.npy")), np.load(os.path.join(d, "fla.npy"))
    assert sorted(os.listdir(d)) == ["fla.npy", "flux.npy", "points.npy"]
    assert flux.dtype == fla.dtype == np.float64 and flux.shape == fla.shape == (POINTS, 3, 300)
    assert np.array_equal(np.load(os.path.join(d, "points.npy")), np.arange(float(POINTS)))
    pts = scan.c4_points(si=2.5)[:POINTS]
    plan = nu.Plan(300, 12.0, 17.0, 5.0, max_points=POINTS)   # the library default arithmetic, as the plain run's
    want_flux, want_fla = plan.evolve(pts)
    plan.close()
    assert np.all(np.isfinite(fla)) and np.all(fla >= 0) and np.any(fla > 0)
    for k in range(POINTS):
        assert cases.rel_err(flux[k], want_flux[k]) <= cases.FLUX_RTOL, k
        assert cases.rel_err(fla[k], want_fla[k]) <= cases.FLUX_RTOL, k
