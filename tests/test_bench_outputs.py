"""bench.py --dump-outputs on the GPU: a plain one-GPU run on the fused path
with an odd step count (multi-step launches of the even part, then one
single-step launch) writes the state its timed steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_dumps_the_fused_state_after_an_odd_step_count(tmp_path):
    from stsphere.engine import Engine
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--N", "32",
                        "--tiles-per-edge", "2", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    out = json.loads(lines[0])
    c = out["config"]
    assert out["status"] == "ok" and out["steps"] == 5 and out["ms_per_step"] > 0
    assert c["runtime"] == "fused" and c["steps_per_launch"] == 4, c
    assert c["direct_launch_steps"] == 4 and c["eager_steps"] == 1 and c["kernel_launches"] == 1, c
    assert out["finite"] is None and out["mass"] is None          # --full only
    # the PyTorch fp64 reference of the same 2 + 5 steps; 1e-10 of each field's
    # maximum is the bound of the fused multi-step launches in smoke()
    ref = Engine(ShallowWater("tc5"), TileLayout(32, 2, 1, ng=2), 0, grid=CubedSphereGrid(32), dtype=torch.float64,
                 device="cuda:0", backend="torch", integrator="ssprk3", dt=c["dt_s"])
    ref.step(7)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{n}.npy" for n in ShallowWater.fields)
    for f, name in enumerate(ShallowWater.fields):
        got = np.load(tmp_path / f"{name}.npy")
        want = ref.global_field(f)
        assert got.dtype == np.float64 and got.shape == (6, 32, 32)
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{name}: max rel diff vs reference {err:.3e}")
        assert np.isfinite(got).all() and err < 1e-10, (name, err)
