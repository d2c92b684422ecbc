"""bench.py end to end on one GPU (configuration 2: 100k Gaussians, 800x800): a plain run prints the headline line
only -- every other measurement is behind ``--full`` -- and ``--dump-outputs`` writes the arrays of one call of the
timed path from the state the timed steps started from."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FULL_ONLY = ["fwd_bwd_ms_per_view", "fwd_bwd_ms_per_view_host_synced", "kernels_ms", "kernel_launches_per_step",
             "kernels_hbm", "roofline", "cpu_baseline", "dropin_api_step"]


def run_bench(args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "2"] + args,
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_only_and_dumps_outputs(tmp_path):
    P, W, H, steps = 100_000, 800, 800, 3
    res = run_bench(["--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert res["full"] is False and not [k for k in FULL_ONLY if k in res]
    assert res["steps"] == steps and res["unit"] == "views/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f32" and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(1000.0 / res["ms_per_step"], rel=1e-2)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == sorted(["render", "radii", "viewspace_grad", "num_rendered", "loss", "exp_avg_xyz",
                                  "exp_avg_features_dc", "exp_avg_features_rest", "exp_avg_opacity",
                                  "exp_avg_scaling", "exp_avg_rotation"])
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 1000 * 1000
    assert got["render"].shape == (3, H, W) and 0.0 < got["render"].mean() < 1.0
    assert got["radii"].shape == (P,) and got["viewspace_grad"].shape == (P, 3) and got["exp_avg_xyz"].shape == (P, 3)
    # the dumped call starts where the first timed step did, and the forward has no order-dependent sums
    assert got["num_rendered"][0] == res["config"]["num_rendered_timed_first"] > 0
    assert np.abs(got["exp_avg_xyz"]).max() > 0
    assert 0.0 < got["loss"][0] < 1.0


def test_full_run_keeps_every_measurement():
    res = run_bench(["--steps", "3", "--warmup", "1", "--full", "--cpu-baseline", "off"])
    assert res["full"] is True and not [k for k in FULL_ONLY if k not in res]
    assert res["fwd_bwd_ms_per_view"] > 0 and res["kernels_ms"]["render_bwd"] > 0
    assert res["dropin_api_step"]["ms_per_step"] > 0 and res["roofline"]["kernel"]
