"""Time-dependent winds of the advection model on the PyTorch twin
(models/advection.py, models/initial_conditions.py, engine.py): the
deformational flows of Nair & Lauritzen (2010) and Lauritzen et al. (2012).
The default wind is unchanged; the streamfunction transports are discretely
non-divergent and keep a constant; the stage times give every integrator its
order; the tracer returns to its start; tilings and ranks agree to the bit;
the solver parses, reports, resumes and refuses.  Every figure is printed
before it is asserted."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from stsphere import driver as S
from stsphere.engine import Engine, VirtualCluster
from stsphere.ensemble import Ensemble
from stsphere.models import initial_conditions as ic
from stsphere.models.advection import Advection
from stsphere.models.errors import williamson_norms
from stsphere.models.geometry import DAY, CubedSphereGrid
from stsphere.models.integrators import get_integrator
from stsphere.parallel.layout import TileLayout

EPS = np.finfo(np.float64).eps
LIM = {"none": 0, "mc": 2, "ppm": 4}


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _engine(N, flow="deform_nd", case="gaussian_hills", limiter="mc", t=1, integrator="ssprk3", cls=Advection, **kw):
    lim = LIM[limiter]
    return Engine(cls(case, limiter=lim, flow=flow), TileLayout(N, t, 1, ng=3 if lim == 4 else 2), grid=_grid(N),
                  integrator=integrator, **kw)


class MidpointAdvection(Advection):
    """The same wind through the midpoint rule U = (v . m) L."""

    def transports(self, geo, t=0.0):
        return self.midpoint_transports(geo, t)


# ---- the default wind ----------------------------------------------------------------------------

def test_default_wind_is_unchanged():
    a = Advection()
    assert a.flow == "solid_body" and a.period == 12 * DAY and not a.time_dependent
    e = Engine(a, TileLayout(16, 1, 1, ng=2), grid=_grid(16))
    geo, g = e.geo, _grid(16)
    u0 = 2.0 * math.pi * g.radius / (12.0 * DAY)
    ux = np.sum(ic.solid_body_wind(geo.xmid, u0, 0.0, g.radius) * geo.mx[:, None, :, :], axis=-1) * geo.lx
    uy = np.sum(ic.solid_body_wind(geo.ymid, u0, 0.0, g.radius) * geo.my[:, :, None, :], axis=-1) * geo.ly
    assert np.array_equal(e.tens["ex"].numpy(), ux) and np.array_equal(e.tens["ey"].numpy(), uy)
    b = Engine(Advection(flow="solid_body"), TileLayout(16, 1, 1, ng=2), grid=_grid(16))
    ex0 = e.tens["ex"].clone()
    e.step(5)
    b.step(5)
    assert torch.equal(e.state, b.state) and torch.equal(e.tens["ex"], ex0)
    with pytest.raises(ValueError, match="unknown flow"):
        Advection(flow="deform")


def test_stage_abscissae():
    want = {"euler": [0.0], "ssprk2": [0.0, 1.0], "ssprk3": [0.0, 1.0, 0.5], "rk4": [0.0, 0.5, 0.5, 1.0]}
    for name, c in want.items():
        assert [s.t for s in get_integrator(name).stages] == c
    e = _engine(16, dt=100.0)
    e.step_count = 7
    assert [e.stage_time(s) for s in e.integ.stages] == [700.0, 800.0, 750.0]


# ---- the streamfunction transports ---------------------------------------------------------------------

def _solid_body_difference(N):
    """max |U_psi - U_midpoint| / max |U| of solid-body rotation, psi = -R u0 sin(th)."""
    a = Advection()
    e = Engine(a, TileLayout(N, 1, 1, ng=2), grid=_grid(N))
    g = _grid(N)
    _, lat = a.vertex_lonlat(e.geo)
    psi = -g.radius * a._u0(g) * np.sin(lat)
    ex, ey = -(psi[:, 1:, :] - psi[:, :-1, :]), psi[:, :, 1:] - psi[:, :, :-1]
    ux, uy = a.midpoint_transports(e.geo)
    return max(np.abs(ex - ux).max(), np.abs(ey - uy).max()) / max(np.abs(ux).max(), np.abs(uy).max())


def test_streamfunction_form_of_solid_body_rotation():
    # measured: C16 4.02e-4, C32 1.00e-4 (ratio 0.250: the midpoint rule's second order)
    d16, d32 = _solid_body_difference(16), _solid_body_difference(32)
    print(f"psi form vs midpoint rule: C16 {d16:.3e}, C32 {d32:.3e}, ratio {d32 / d16:.3f}")
    assert d16 < 1e-3
    assert d32 < 0.3 * d16


@pytest.mark.parametrize("flow", ic.STREAM_FLOWS)
def test_discrete_divergence(flow):
    e = _engine(16, flow=flow)
    ph = e.physics
    t = 0.3 * ph.period
    ex, ey = ph.transports(e.geo, t)
    div = (ex[:, :, 1:] - ex[:, :, :-1]) + (ey[:, 1:, :] - ey[:, :-1, :])
    bound = 8 * EPS * np.abs(ph.streamfunction(e.geo, t)).max()
    mid = ph.midpoint_transports(e.geo, t)
    dmid = (mid[0][:, :, 1:] - mid[0][:, :, :-1]) + (mid[1][:, 1:, :] - mid[1][:, :-1, :])
    print(f"{flow}: max |sum of a cell's four U| {np.abs(div).max():.3e} (bound {bound:.3e}); midpoint rule "
          f"{np.abs(dmid).max():.3e}; max |U| {np.abs(ex).max():.3e}")
    assert np.abs(div).max() <= bound
    # the vertex differences are the wind: they agree with the midpoint rule to its truncation error
    assert max(np.abs(ex - mid[0]).max(), np.abs(ey - mid[1]).max()) < 5e-3 * np.abs(mid[0]).max()


def test_constant_is_preserved():
    e = _engine(16, case="constant")
    m = _engine(16, case="constant", cls=MidpointAdvection)
    e.step(20)
    m.step(20)
    d = float((e.tiles_view() - 1.0).abs().max())
    dm = float((m.tiles_view() - 1.0).abs().max())
    print(f"q = 1 after 20 steps of deform_nd: vertex differences {d:.3e}, midpoint rule {dm:.3e}")
    assert d <= 1e-13
    assert dm > 1e-8


# ---- stage times ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _quarter(integrator, nsteps):
    e = _engine(16, limiter="none", integrator=integrator)
    e.dt = 0.25 * e.physics.period / nsteps
    e.step(nsteps)
    return e.tiles_view().clone()


@pytest.mark.parametrize("integrator,need", [("ssprk3", 7.0), ("rk4", 12.0), ("ssprk2", 4.0)])
def test_stage_times_by_step_halving(integrator, need):
    """|q_60 - q_240| / |q_120 - q_240| at t = T / 4: 2^p + 1 for order p (9, 17, 5); a wind frozen at
    the step's start gives 3 with every integrator.  Measured: ssprk3 9.01, rk4 17.3, ssprk2 5.04."""
    q60, q120, q240 = (_quarter(integrator, k) for k in (60, 120, 240))
    r = float((q60 - q240).norm() / (q120 - q240).norm())
    print(f"{integrator}: step-halving ratio {r:.3f}")
    assert r >= need


# ---- return to start -----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _return_run(N, limiter):
    """gaussian_hills, SSP-RK3, one period at cfl 0.9 (dt shortened to land on T): (norms, mass drift)."""
    e = _engine(N, limiter=limiter)
    ph, g = e.physics, _grid(N)
    ns = int(math.ceil(ph.period / e.dt))
    e.dt = ph.period / ns
    q0 = e.global_field()
    e.step(ns)
    q, A = e.global_field(), g.areas()
    assert np.array_equal(ph.exact(g, e.time, e.dt), q0) and ph.exact(g, 0.5 * ph.period, e.dt) is None
    return williamson_norms(q, q0, A), float(abs((q * A).sum() - (q0 * A).sum()) / (q0 * A).sum())


def test_return_to_start_c16():
    (mc, dm), (ppm, dp) = _return_run(16, "mc"), _return_run(16, "ppm")
    print(f"C16 gaussian_hills after one period: MC l2 {mc['l2']:.4f}, PPM l2 {ppm['l2']:.4f}; "
          f"mass drift {dm:.2e}, {dp:.2e}")
    assert ppm["l2"] < mc["l2"] < 1.0
    assert dm < 1e-12 and dp < 1e-12


@pytest.mark.slow
def test_return_to_start_converges():
    (c16, _), (c32, d32) = _return_run(16, "mc"), _return_run(32, "mc")
    print(f"gaussian_hills, MC, one period: l2 C16 {c16['l2']:.4f}, C32 {c32['l2']:.4f}; mass drift {d32:.2e}")
    assert c32["l2"] < c16["l2"]
    assert d32 < 1e-12


# ---- tilings and ranks ---------------------------------------------------------------------------------

@pytest.mark.parametrize("flow", ["deform_nd", "deform_div"])
def test_tilings_and_ranks_agree_bitwise(flow):
    a = _engine(16, flow=flow, case="slotted_cylinders")
    b = _engine(16, flow=flow, case="slotted_cylinders", t=2, dt=a.dt)
    c = VirtualCluster(lambda: Advection("slotted_cylinders", flow=flow), TileLayout(16, 2, 4, ng=2), grid=_grid(16),
                       dt=a.dt)
    for x in (a, b, c):
        x.step(10)
    assert a.step_count == 10 and all(e.step_count == 10 for e in c.engines)
    assert np.array_equal(a.global_field(), b.global_field())
    assert np.array_equal(a.global_field(), c.global_field())


# ---- solver -----------------------------------------------------------------------------------------------

def _cfg(tmp, **physics):
    ph = {"model": "advection", "case": "gaussian_hills", "flow": "deform_nd", "limiter": "mc", "period_days": 12}
    ph.update(physics)
    return {"parallelization": {"tiles_per_edge": 1, "num_devices": 1, "device_type": "cpu"},
            "grid": {"N": 8}, "physics": ph, "time": {"integrator": "ssprk3"},
            "io": {"output_dir": os.path.join(str(tmp), "run")}}


def test_solver_config_and_error_norms(tmp_path):
    s = S.Solver("physics: {model: advection, case: cosine_bells, flow: deform_div, period_days: 5}\n"
                 "grid: {N: 8}\nparallelization: {num_devices: 1}\n", verbose=False)
    s.initialize()
    assert s.physics.flow == "deform_div" and s.physics.period == 5 * DAY and s.physics.time_dependent
    s = S.Solver(_cfg(tmp_path), verbose=False)
    s.initialize()
    ns = s.physics.period / s.dt
    assert abs(ns - round(ns)) < 1e-9 and not s._use_native()      # a whole number of steps per period
    # an even count (the default step gives 259 at C8), so that a step lands on T / 2
    ns = 260
    cfg = _cfg(tmp_path)
    cfg["time"]["dt"] = 12 * DAY / ns
    s = S.Solver(cfg, verbose=False)
    s.initialize()
    assert s.dt < s.physics.max_dt(s.grid)
    s.step(ns // 2)
    assert abs(s.time - 0.5 * s.physics.period) < 1e-6 * s.dt and s.error_norms() is None      # t = T / 2
    s.step(ns // 2 - 1)
    assert s.error_norms() is None
    summary = s.run(nsteps=1)
    norms = s.error_norms()
    print(f"C8 after one period: {norms}; q in [{summary['q_min']:.4f}, {summary['q_max']:.4f}], "
          f"mass drift {summary['mass_drift']:.2e}")
    assert set(norms) == {"l1", "l2", "linf"} and 0 < norms["l2"] < 2
    assert summary["err_l2"] == norms["l2"] and abs(summary["mass_drift"]) < 1e-12
    assert summary["q_min"] <= summary["q_max"]


def test_solver_checkpoint_resumes_on_the_trajectory(tmp_path):
    a = S.Solver(_cfg(tmp_path), verbose=False)
    a.initialize()
    a.step(7)
    path = a.save_checkpoint()
    a.step(6)
    b = S.Solver(_cfg(tmp_path), verbose=False)
    b.initialize()
    b.restore_checkpoint(path)
    assert b.step_count == 7
    b.step(6)
    assert np.array_equal(a.gather_global(), b.gather_global())
    c = S.Solver(_cfg(tmp_path), verbose=False)      # the wind of another time leaves the trajectory
    c.initialize()
    c.restore_checkpoint(path)
    c.engines[0].step_count = 0
    c.step(6)
    assert not np.array_equal(a.gather_global(), c.gather_global())


def test_refusals(tmp_path, monkeypatch):
    bad = _cfg(tmp_path)
    bad["physics"].update(model="swe", case="tc2")
    with pytest.raises(ValueError, match="physics.flow"):
        S.make_physics(S.load_config(bad).physics)
    bad = _cfg(tmp_path, flow=None)
    bad["physics"].update(model="diffusion", case="lima_flag")
    with pytest.raises(ValueError, match="period_days"):
        S.make_physics(S.load_config(bad).physics)
    with pytest.raises(ValueError, match="unknown flow"):
        S.make_physics(S.load_config(_cfg(tmp_path, flow="swirl")).physics)
    march = _cfg(tmp_path)
    march["runtime"] = {"block": [64, 4]}
    with pytest.raises(ValueError, match="march block"):
        S.Solver(march, verbose=False).initialize()
    for mode in ("streams", "batched"):
        with pytest.raises(ValueError, match="time-dependent"):
            Ensemble(lambda: Advection("gaussian_hills", flow="deform_nd"), TileLayout(8, 1, 1, ng=2), 2, mode=mode)
    monkeypatch.setenv("WORLD_SIZE", "6")
    spmd = _cfg(tmp_path)
    spmd["parallelization"].update(num_devices=6)
    with pytest.raises(ValueError, match="one process per rank"):
        S.Solver(spmd, verbose=False).initialize()
