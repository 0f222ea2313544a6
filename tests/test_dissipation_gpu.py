"""The gfx950 dissipation kernels (ops/csrc/dissipation_kernel.hip) against
their PyTorch twin (models/dissipation.py), with the project's bounds, and the
plumbing through the solver.  Measured values: profiles/dissipation/README.md."""
import functools

import numpy as np
import pytest
import torch

import rough_states as rs
from stsphere.driver import Solver
from stsphere.engine import Engine, VirtualCluster
from stsphere.models.swe import ShallowWater
from stsphere.ops.dissipation import apply_all
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

# (N, tiles per edge): 16 + a partial block of 8; 16 + a partial block one cell wide;
# n = 12 with tile edges inside panels
SHAPES = [(24, 1), (17, 1), (24, 2)]
TAU = 600.0


def _engine(N, t, device, case="tc5", dtype=torch.float64):
    return Engine(ShallowWater(case), TileLayout(N, t, 1, ng=2), grid=rs.grid_of(N), dtype=dtype, device=device,
                  backend="hip" if device != "cpu" else "torch")


@functools.lru_cache(maxsize=None)
def _cpu(N, t, case="tc5"):
    return _engine(N, t, "cpu", case)


@functools.lru_cache(maxsize=None)
def _state(N, kind):
    """Global fp64 state [4, 6, N, N]: the TC5 initial state or the rough one."""
    e = _cpu(N, 1)
    G0 = torch.as_tensor(e.physics.initial_state(e.geo))      # t = 1: the tiles are the panels
    return G0 if kind == "tc5" else rs.swe_state(G0, rs.grid_of(N).centers(), "rough")


def _nu(e, order, m):
    """nu that needs exactly m sub-steps of TAU (m = 1: a quarter of the bound)."""
    lam = e.dissipation().lam
    x = 0.25 if m == 1 else m - 0.5
    return x / (2.0 * TAU * lam) if order == 1 else x / (TAU * (2.0 * lam) ** 2)


@functools.lru_cache(maxsize=None)
def _twin_applied(N, t, kind, order, m, fp32=False):
    e = _cpu(N, t)
    q = rs.local_of(e, _state(N, kind))
    if fp32:
        e = _engine(N, t, "cpu", dtype=torch.float32)
        q = q.float()
    e.set_state(q)
    assert e.dissipation(order, _nu(e, order, m)).apply(TAU) == m
    return e.tiles_view().clone()


# ---- 1. laplacian() ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rough", "smooth"])
@pytest.mark.parametrize("N,t", SHAPES)
def test_laplacian_matches_twin(N, t, kind):
    c, g = _cpu(N, t), _engine(N, t, "cuda:0")
    if kind == "rough":
        x = rs.local_of(c, _state(N, "rough"))
    else:
        p = torch.as_tensor(np.moveaxis(c.geo.center, -1, 0))
        x = torch.stack([35 * p[2] ** 4 - 30 * p[2] ** 2 + 3, p[0] * p[1], p[2], p[0] * p[0] - p[1] * p[2]])
    ref = c.dissipation().laplacian(x)
    assert g.dissipation().hip and not c.dissipation().hip          # the kernels against the twin
    got = g.dissipation().laplacian(x.cuda())
    torch.cuda.synchronize()
    errs = [float((got[k].cpu() - ref[k]).abs().max() / ref[k].abs().max()) for k in range(4)]
    print(f"laplacian C{N} t={t} {kind}: error / max |L x| {['%.2e' % v for v in errs]}")
    assert bool(torch.isfinite(got).all()) and max(errs) <= 1e-11


# ---- 2. one application -------------------------------------------------------------------------

def _field_errs(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return [float((got[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in range(ref.shape[0])]


@pytest.mark.parametrize("kind", ["tc5", "rough"])
@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("order", [1, 2])
def test_one_application_matches_twin(order, m, kind):
    N, t = 24, 2
    ref = _twin_applied(N, t, kind, order, m)
    g = _engine(N, t, "cuda:0")
    q0 = rs.install(g, _state(N, kind))
    d = g.dissipation(order, _nu(_cpu(N, t), order, m))
    assert d.hip and d.apply(TAU) == m
    torch.cuda.synchronize()
    errs = _field_errs(g.tiles_view(), ref)
    moved = float((g.tiles_view().cpu() - q0).abs().max())
    print(f"apply order {order} m {m} {kind}: error / max |field| {['%.2e' % v for v in errs]}, moved {moved:.3e}")
    assert moved > 0 and max(errs) <= 1e-12
    # the same-rank ghost slots are current
    q = g.state.clone()
    g.refresh_halos(q)
    assert torch.equal(q, g.state)


@pytest.mark.parametrize("order", [1, 2])
def test_one_application_fp32_state(order):
    N, t = 24, 1
    ref = _twin_applied(N, t, "rough", order, 1, fp32=True)
    g = _engine(N, t, "cuda:0", dtype=torch.float32)
    rs.install(g, _state(N, "rough"))
    g.dissipation(order, _nu(_cpu(N, t), order, 1)).apply(TAU)
    torch.cuda.synchronize()
    errs = _field_errs(g.tiles_view(), ref)
    print(f"apply fp32 order {order}: error / max |field| {['%.2e' % v for v in errs]}")
    assert g.tiles_view().dtype == torch.float32 and max(errs) <= 1e-6


# ---- 3. virtual ranks on one GPU --------------------------------------------------------------

@pytest.mark.parametrize("nd", [2, 8])
@pytest.mark.parametrize("order", [1, 2])
def test_virtual_ranks_match_one_rank(order, nd):
    N, t = 24, 2
    one = _engine(N, t, "cuda:0")
    rs.install(one, _state(N, "rough"))
    nu = _nu(_cpu(N, t), order, 1)
    one.dissipation(order, nu).apply(TAU)
    vc = VirtualCluster(lambda: ShallowWater("tc5"), TileLayout(N, t, nd, ng=2), grid=rs.grid_of(N), device="cuda:0",
                        backend="hip")
    for e in vc.engines:
        rs.install(e, _state(N, "rough"))
    apply_all([e.dissipation(order, nu) for e in vc.engines], TAU)
    torch.cuda.synchronize()
    a, b = rs.global_of(one), rs.global_of(vc.engines)
    errs = [float((a[k] - b[k]).abs().max() / a[k].abs().max()) for k in range(4)]
    print(f"{nd} virtual ranks order {order}: {['%.2e' % v for v in errs]}, bitwise {torch.equal(a, b)}")
    assert max(errs) <= 1e-12
    ref = _twin_applied(N, t, "rough", order, 1)
    assert max(_field_errs(one.tiles_view(), ref)) <= 1e-12


# ---- 4. fixed point and conservation on the device -----------------------------------------------

@pytest.mark.parametrize("order,nu", [(1, 1.0e5), (2, 1.0e15)])
def test_mountain_fixed_point_and_mass(order, nu):
    g = _engine(24, 1, "cuda:0")
    b = g.tens["b"]
    q = torch.zeros((4,) + tuple(b.shape), dtype=torch.float64, device="cuda:0")
    q[0] = 5960.0 - b
    g.set_state(q)
    d = g.dissipation(order, nu)
    d.apply(TAU)
    out = g.tiles_view()
    assert float((out[0] - q[0]).abs().max()) <= 1e-12 * float(q[0].max())
    assert bool((out[1:4] == 0).all())
    rs.install(g, _state(24, "rough"))
    A = g.tens["area"]
    m0 = float((g.tiles_view()[0] * A).sum())
    q0 = g.tiles_view().clone()
    for _ in range(4):
        d.apply(TAU)
    assert not torch.equal(q0, g.tiles_view())
    assert abs(float((g.tiles_view()[0] * A).sum()) - m0) < 1e-13 * m0


# ---- 5. the solver --------------------------------------------------------------------------------

def _cfg(out, device, diss=None, case="galewsky", tracers=None):
    c = {"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": device},
         "grid": {"N": 24, "halo": 2, "dtype": "float64"},
         "physics": {"model": "swe", "case": case, "limiter": "mc"},
         "time": {"integrator": "ssprk3", "dt": 150.0}, "io": {"output_dir": str(out)},
         "runtime": {"steps_per_graph": 4, "fused": "auto"}}
    if diss is not None:
        c["physics"]["dissipation"] = diss
    if tracers is not None:
        c["physics"]["tracers"] = tracers
    return c


def test_solver_hip_matches_torch_backend(tmp_path):
    diss = {"order": 1, "nu": 1.0e5, "interval": 2}
    g = Solver(_cfg(tmp_path / "g", "gpu", diss), verbose=False)
    c = Solver(_cfg(tmp_path / "c", "cpu", diss), verbose=False)
    g.run(nsteps=8)
    c.run(nsteps=8)
    a, b = g.gather_global(), c.gather_global()
    err = max(np.abs(a[f] - b[f]).max() / np.abs(b[f]).max() for f in range(4))
    print(f"solver galewsky C24, 8 steps, interval 2, runtime {'fused' if g.fused is not None else 'native'}: {err:.3e}")
    assert err < 1e-11
    assert type(g.runner).__name__ == "NativeStepper"
    plain = Solver(_cfg(tmp_path / "p", "cpu"), verbose=False)
    plain.run(nsteps=8)
    assert np.abs(plain.gather_global() - b).max() > 0
    e = g.engines[0]
    q = e.state.clone()
    e.refresh_halos(q)
    assert torch.equal(q, e.state)
    g.close()


# ---- 6. tracers -----------------------------------------------------------------------------------

def test_tracers_without_depth_keep_h_and_hq(tmp_path):
    kw = dict(case="tc5", tracers=["cap", "gradient"])
    a = Solver(_cfg(tmp_path / "a", "gpu", {"order": 1, "nu": 1.0e5, "depth": False, "interval": 2}, **kw),
               verbose=False)
    b = Solver(_cfg(tmp_path / "b", "gpu", **kw), verbose=False)
    a.initialize()
    b.initialize()
    a.step(2)            # two steps, then the operator
    b.step(2)
    ga, gb = a.gather_global(), b.gather_global()
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[4:], gb[4:])
    assert not np.array_equal(ga[1:4], gb[1:4])
    a.close()
    b.close()
