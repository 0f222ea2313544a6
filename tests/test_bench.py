"""bench.py contract on the CPU (torch backend, gloo): the self-launching
multi-rank entry point and the one-rank JSON line."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=300):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_one_rank_cpu():
    out = _run(["--backend", "torch", "--N", "12", "--steps", "2", "--warmup", "1", "--full"])
    assert out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert out["metric"] == "cell-updates/sec (whole node) at C12"
    assert out["value"] > 0 and out["finite"] and out["higher_is_better"] is True
    assert out["max_abs_diff_vs_1gpu"] is None


def test_bench_plain_run_dumps_the_final_state_cpu(tmp_path):
    """A plain run (no --full) skips the checks beyond the headline figure, and
    --dump-outputs writes the state after warmup + steps (an odd step count),
    one [6, N, N] array per field, equal to an engine stepped the same way."""
    import numpy as np
    import torch
    from stsphere.engine import Engine
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    out = _run(["--backend", "torch", "--N", "12", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0 and out["status"] == "ok"
    assert out["finite"] is None and out["mass"] is None and out["max_abs_diff_vs_1gpu"] is None
    eng = Engine(ShallowWater("tc5"), TileLayout(12, 2, 1, ng=2), 0, grid=CubedSphereGrid(12), dtype=torch.float64,
                 device="cpu", backend="torch", integrator="ssprk3", dt=out["config"]["dt_s"])
    eng.step(4)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{n}.npy" for n in ShallowWater.fields)
    for f, name in enumerate(ShallowWater.fields):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float64 and got.shape == (6, 12, 12)
        assert np.array_equal(got, eng.global_field(f)), name


def test_dump_outputs_samples_a_large_state_the_same_way_every_time(tmp_path, monkeypatch):
    """Above the size limit every field is written as the same seeded sample of
    its cells, identical from call to call, and the whole stays under the limit."""
    import numpy as np
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4000)
    fields = np.arange(3 * 6 * 10 * 10, dtype=np.float32).reshape(3, 6, 10, 10)
    bench.dump_outputs(str(tmp_path / "a"), fields, ["h", "u", "v"])
    bench.dump_outputs(str(tmp_path / "b"), fields, ["h", "u", "v"])
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("h", "u", "v")}
    assert sum(g.nbytes for g in got.values()) <= 4000 and all(g.dtype == np.float32 for g in got.values())
    assert got["h"].shape == (333,) and len(np.unique(got["h"])) == 333 and got["h"].max() < 600
    assert np.array_equal(got["u"], got["h"] + 600) and np.array_equal(got["v"], got["h"] + 1200)
    for n, g in got.items():
        assert np.array_equal(g, np.load(tmp_path / "b" / f"{n}.npy"))
    monkeypatch.setattr(bench, "DUMP_LIMIT", 3 * 600 * 4)          # exactly fits: written whole
    bench.dump_outputs(str(tmp_path / "c"), fields, ["h", "u", "v"])
    assert np.array_equal(np.load(tmp_path / "c" / "u.npy"), fields[1])


@pytest.mark.parametrize("gpus,t", [(2, 1), (3, 1)])
def test_bench_self_launches_ranks_cpu(gpus, t):
    """--gpus N without torchrun spawns N ranks; the warmup state and the final
    state must equal one rank's bit for bit."""
    out = _run(["--gpus", str(gpus), "--backend", "torch", "--N", "12", "--tiles-per-edge", str(t),
                "--steps", "2", "--warmup", "1", "--full"])
    assert out["n_gpus"] == gpus
    assert out["max_abs_diff_vs_1gpu_warmup"] == 0.0 and out["max_abs_diff_vs_1gpu"] == 0.0
    assert out["config"]["comm"] == "torch.distributed"


def test_bench_deadline_kills_hung_rank_cpu():
    """A rank that never returns (test hook) is killed at --timeout: the parent
    prints one status=timeout JSON line naming each rank's last phase and exits
    non-zero, well inside the driver's own limit."""
    import time
    env = dict(os.environ, OMP_NUM_THREADS="1", STSP_BENCH_HANG_RANK="1")
    env.pop("WORLD_SIZE", None)
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--backend", "torch",
                        "--N", "12", "--steps", "2", "--warmup", "1", "--timeout", "25"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=200)
    assert r.returncode != 0
    assert time.time() - t0 < 120
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout + r.stderr
    out = json.loads(lines[0])
    assert out["status"] == "timeout" and out["value"] is None
    # phases carry the transport being tried (warmup_<comm>, verify_<comm>)
    assert out["phases"]["1"]["phase"].startswith("warmup")
    assert out["phases"]["0"]["phase"].split("_")[0] in ("warmup", "verify")


def test_bench_preflight_refuses_missing_gpus():
    """--gpus N on the HIP backend with fewer visible GPUs: one status=error
    line, no ranks started (this container has no GPU at all)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("enough GPUs visible")
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.pop("STSP_SHARE_GPU", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "2"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert out["status"] == "error" and "GPU" in out["error"]
