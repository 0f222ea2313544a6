"""Time-dependent winds on the device (ops/csrc/wind_kernel.hip, ops/wind.py):
the table kernel against the twin's transports, HIP stepping against the twin,
the device's step clock under graph replay, virtual ranks, and the shipped
config through the command line.  Every figure is printed before it is
asserted."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from stsphere.engine import Engine, GraphStepper, VirtualCluster
from stsphere.models import initial_conditions as ic
from stsphere.models.advection import Advection
from stsphere.models.geometry import CubedSphereGrid
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
SHAPES = [(16, 1), (16, 2), (24, 1)]       # n = 16, 8, and 24 (partial blocks)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _engine(N, t, flow="deform_nd", case="slotted_cylinders", limiter=2, backend="hip", dtype=torch.float64,
            integrator="ssprk3", device="cuda", **kw):
    return Engine(Advection(case, limiter=limiter, flow=flow), TileLayout(N, t, 1, ng=3 if limiter == 4 else 2),
                  grid=_grid(N), dtype=dtype, device=device, backend=backend, integrator=integrator, **kw)


# ---- the tables ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flow", ic.DEFORM_FLOWS)
@pytest.mark.parametrize("N,t", SHAPES)
def test_tables_match_the_twin(flow, N, t):
    e64, e32 = _engine(N, t, flow), _engine(N, t, flow, dtype=torch.float32)
    ph, geo = e64.physics, e64.geo
    T = ph.period
    # (step count, abscissa, dt): t = 0, T / 2 (where c(t) vanishes) and 0.3 T
    for count, cs, dt in ((0, 0.0, 100.0), (1, 0.0, 0.5 * T), (1, 0.5, 0.2 * T)):
        tm = (count + cs) * dt
        ux, uy = ph.transports(geo, tm)
        if flow in ic.STREAM_FLOWS:
            scale = float(np.abs(ph.streamfunction(geo, tm)).max())
        else:
            scale = float(max(np.abs(ux).max(), np.abs(uy).max()))                                # max |U|
        for e in (e64, e32):
            e.tens["ex"].fill_(float("nan"))
            e.tens["ey"].fill_(float("nan"))
            e.clock.set(count)
            e.clock.update(cs, dt)
        torch.cuda.synchronize()
        assert int(e64.clock.count) == count
        for key, u in (("ex", ux), ("ey", uy)):
            k64, k32 = e64.tens[key].cpu(), e32.tens[key].cpu()
            err = float((k64 - torch.as_tensor(u)).abs().max())
            print(f"{flow} C{N} t{t} time {tm / T:.2f} T {key}: |kernel - twin| {err:.3e}, bound {64 * EPS64 * scale:.3e}")
            assert bool(torch.isfinite(k64).all()) and err <= 64 * EPS64 * scale
            r = k64.float()         # the fp32 table is the fp64 one rounded, to 1 ulp of fp32
            inf = torch.tensor(float("inf"))
            assert bool(((k32 >= torch.nextafter(r, -inf)) & (k32 <= torch.nextafter(r, inf))).all())


# ---- stepping --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _twin(N, t, limiter, integrator, nsteps):
    ref = _engine(N, t, limiter=limiter, backend="torch", integrator=integrator, device="cpu")
    ref.step(nsteps)
    return ref.dt, ref.tiles_view().clone()


def _relerr(a, b):
    """tests/test_hip_kernels.py's metric: max |a - b| / max |a| per field."""
    F = a.shape[0]
    a, b = a.reshape(F, -1), b.reshape(F, -1).double().cpu()
    assert bool(torch.isfinite(b).all())
    return ((a - b).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).max().item()


@pytest.mark.parametrize("limiter", [2, 4], ids=["mc", "ppm"])
@pytest.mark.parametrize("integrator,nsteps", [("ssprk3", 20), ("rk4", 8)])
@pytest.mark.parametrize("N,t", [(16, 1), (24, 1), (16, 2)])
def test_stepping_matches_the_twin(N, t, limiter, integrator, nsteps):
    dt, want = _twin(N, t, limiter, integrator, nsteps)
    for dtype, bound in ((torch.float64, 1e-11), (torch.float32, 1e-4)):
        hip = _engine(N, t, limiter=limiter, dtype=dtype, integrator=integrator, dt=dt)
        hip.step(nsteps)
        torch.cuda.synchronize()
        err = _relerr(want, hip.tiles_view())
        print(f"C{N} t{t} limiter {limiter} {integrator} x{nsteps} {dtype}: rel {err:.3e} (bound {bound:g})")
        assert int(hip.clock.count) == hip.step_count == nsteps
        assert err < bound


# ---- graph and clock ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("integrator", ["ssprk3", "euler"])
def test_graph_replay_keeps_the_clock(integrator):
    kw = dict(integrator=integrator)
    eager = _engine(16, 2, **kw)
    dt = eager.dt * (0.3 if integrator == "euler" else 1.0)
    eager.dt = dt
    g = _engine(16, 2, dt=dt, **kw)
    gs = GraphStepper(g, steps_per_graph=4)
    torch.cuda.synchronize()
    assert g.step_count == 0 and int(g.clock.count) == 0        # the warm-up steps ticked; the capture did not
    gs.run(11)
    eager.step(11)
    torch.cuda.synchronize()
    assert g.step_count == 11 and int(g.clock.count) == 11
    assert torch.equal(g.tiles_view(), eager.tiles_view())
    gs.run(5)
    eager.step(5)
    torch.cuda.synchronize()
    assert int(g.clock.count) == 16 and torch.equal(g.tiles_view(), eager.tiles_view())
    # a state set from outside: the device's clock follows step_count
    q0 = torch.as_tensor(g.physics.initial_state(g.geo))
    for e in (g, eager):
        e.step_count = 3
        e.set_state(q0)
    assert int(g.clock.count) == 3
    gs.run(4)
    eager.step(4)
    torch.cuda.synchronize()
    assert int(g.clock.count) == 7 and torch.equal(g.tiles_view(), eager.tiles_view())
    # and it is the time that matters: the same state from another step count goes elsewhere
    late = _engine(16, 2, dt=dt, **kw)
    late.step(4)
    assert not torch.equal(late.tiles_view(), eager.tiles_view())


# ---- virtual ranks -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flow", ["deform_nd", "deform_div"])
def test_virtual_ranks_match_one_rank(flow):
    one = _engine(16, 2, flow)
    four = VirtualCluster(lambda: Advection("slotted_cylinders", flow=flow), TileLayout(16, 2, 4, ng=2), grid=_grid(16),
                          device="cuda", backend="hip", dt=one.dt)
    one.step(10)
    four.step(10)
    torch.cuda.synchronize()
    assert all(int(e.clock.count) == 10 for e in four.engines)
    assert np.array_equal(one.global_field(), four.global_field())


# ---- the shipped config ------------------------------------------------------------------------------------------

def test_shipped_config_runs_from_the_command_line(tmp_path):
    src = os.path.join(REPO, "sharding-the-sphere-fall-2025-jax-devlab-examples_amd", "configs", "c96_deform_1gpu.yaml")
    with open(src) as f:
        cfg = yaml.safe_load(f)
    assert cfg["physics"]["flow"] == "deform_nd" and cfg["physics"]["case"] == "cosine_bells"
    cfg["grid"]["N"] = 16
    cfg["io"]["output_dir"] = str(tmp_path / "run")
    path = tmp_path / "c16_deform.yaml"
    path.write_text(yaml.safe_dump(cfg))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "stsphere", "run", str(path)], capture_output=True, text=True, env=env,
                       timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0
    assert "Error norms at t = 1.000 T" in r.stdout and "relative mass drift" in r.stdout
    # the steps replayed from the graph: no quiet fall-back to eager stepping
    summary = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{"steps"')][-1])
    print(f"runtime {summary['runtime']}, {summary['graph_steps']} of {summary['steps_run']} steps replayed")
    assert summary["runtime"] == "graph" and summary["graph_steps"] >= summary["steps_run"] - 30 > 0


def test_solver_steps_through_the_graph(tmp_path):
    from stsphere import driver as S
    cfg = {"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": "gpu"}, "grid": {"N": 16},
           "physics": {"model": "advection", "case": "cosine_bells", "flow": "deform_nd", "limiter": "mc"},
           "time": {"integrator": "ssprk3"}, "runtime": {"steps_per_graph": 8},
           "io": {"output_dir": str(tmp_path / "run")}}
    s = S.Solver(cfg, verbose=False)
    summary = s.run(nsteps=20)
    eager = _engine(16, 2, case="cosine_bells", dt=s.dt)
    eager.step(20)
    torch.cuda.synchronize()
    assert summary["runtime"] == "graph" and summary["graph_steps"] == 16 and summary["steps_run"] == 20
    assert int(s.engines[0].clock.count) == 20
    assert np.array_equal(s.gather_global()[0], eager.global_field())
    with pytest.raises(ValueError, match="time-dependent"):
        from stsphere.ops.native_runtime import NativeStepper
        NativeStepper(s.engines[0])
    s.close()
