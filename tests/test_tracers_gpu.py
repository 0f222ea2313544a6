"""Shallow water with passive tracers on the GPU: the stage kernel
``ops/csrc/swe_tracer_stage.hip`` against its fp64 PyTorch twin
(``models/swe.py::ShallowWaterTracers``), with the project's bounds: relative
error below 1e-11 for fp64 and below 1e-4 for fp32."""
import functools

import numpy as np
import pytest
import torch

from stsphere.engine import Engine, VirtualCluster
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater, ShallowWaterTracers
from stsphere.parallel.layout import TileLayout

from tracer_states import TRACER_SETS, increment_error, install, make_state

pytestmark = pytest.mark.gpu

BLOCKS = [(16, 16), (16, 8)]
FP64_BOUND, FP32_BOUND = 1e-11, 1e-4


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _phys(nq, lim, case="tc5", tracers=None):
    return ShallowWaterTracers(case, tracers=tracers or TRACER_SETS[nq], limiter=lim)


@functools.lru_cache(maxsize=None)
def _reference(N, t, nq, lim, integ, steps):
    """The twin's state after ``steps`` steps (fp64, computed once per case and
    shared by the block shapes and precisions), and its dt."""
    ref = Engine(_phys(nq, lim), TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=torch.float64, device="cuda",
                 backend="torch", integrator=integ)
    ref.step(steps)
    torch.cuda.synchronize()
    return ref.tiles_view().detach().clone(), ref.dt


def _hip(N, t, nq, lim, block, dtype=torch.float64, integ="ssprk3", dt=None):
    return Engine(_phys(nq, lim), TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=dtype, device="cuda", backend="hip",
                  integrator=integ, block=block, dt=dt)


def _relerr(a, hip):
    F = a.shape[0]
    b = hip.tiles_view().double()
    assert bool(torch.isfinite(b).all()), f"{int((~torch.isfinite(b)).sum())} non-finite values in the hip state"
    a, b = a.reshape(F, -1), b.reshape(F, -1)
    return ((a - b).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).max().item()


def _check(N, t, nq, lim, block, dtype=torch.float64, integ="ssprk3", steps=4):
    a, dt = _reference(N, t, nq, lim, integ, steps)
    hip = _hip(N, t, nq, lim, block, dtype, integ, dt)
    assert hip.compute.phys_id == 3 and (hip.compute.bx, hip.compute.by) == block
    hip.step(steps)
    torch.cuda.synchronize()
    err = _relerr(a, hip)
    print(f"C{N} t={t} nq={nq} lim={lim} block={block} {dtype} {integ}: rel err {err:.3e}")
    assert err < (FP64_BOUND if dtype == torch.float64 else FP32_BOUND)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("nq", [1, 2, 4])
@pytest.mark.parametrize("t", [1, 2])
def test_kernel_matches_twin(t, nq, lim, block):
    _check(24, t, nq, lim, block)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_integrators(integ):
    _check(24, 2, 2, 2, (16, 16), integ=integ)


@pytest.mark.parametrize("block", BLOCKS)
def test_fp32(block):
    _check(24, 2, 2, 2, block, dtype=torch.float32)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("N,t", [(17, 1), (34, 2), (20, 1)])
def test_partial_blocks_and_one_cell_wide_last_block(N, t, block):
    """n = 17: the last block is one cell wide, so the last-but-one block's
    window reaches the ghost strip (block_sides); n = 20: a partial block."""
    _check(N, t, 2, 2, block)


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("cls", ["rough", "plateau"])
def test_rough_start(cls, t):
    """Rough SWE state and rough tracers (tracer_states): both signs of the
    depth flux and every slope arm, measured on the increment of one step."""
    N = 16
    L = TileLayout(N, t, 1, ng=2)
    for lim in (0, 1, 2, 3):
        ref = Engine(_phys(2, lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="torch")
        G = make_state(ref, cls)
        for block in BLOCKS:
            r = Engine(_phys(2, lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="torch", dt=ref.dt)
            hip = Engine(_phys(2, lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="hip",
                         block=block, dt=ref.dt)
            q0 = install(r, G)
            install(hip, G)
            r.step(1)
            hip.step(1)
            torch.cuda.synchronize()
            errs = increment_error(r, hip, q0, bound=FP64_BOUND, block=block, what=f"{cls} lim {lim} block {block}")
            print(f"{cls} t={t} lim={lim} block={block}: increment errors {['%.2e' % e for e in errs]}")


@pytest.mark.parametrize("ranks", [2, 8])
def test_remote_ghosts_virtual_ranks(ranks):
    """Several virtual ranks on one GPU against one rank: the receive-buffer
    gather (rows of 4 + NQ values) and the interior / boundary block lists."""
    N = 24
    mk = lambda: _phys(2, 2)   # noqa: E731
    single = Engine(mk(), TileLayout(N, 2, 1, ng=2), grid=_grid(N), device="cuda", backend="hip")
    vc = VirtualCluster(mk, TileLayout(N, 2, ranks, ng=2), grid=_grid(N), device="cuda", backend="hip", dt=single.dt)
    single.step(5)
    vc.step(5)
    torch.cuda.synchronize()
    for f in range(6):
        a, b = single.global_field(f), vc.global_field(f)
        assert abs(a - b).max() <= 1e-12 * max(1.0, abs(a).max()), f


def test_properties_on_the_device():
    """q = 0.75 stays constant, a 0/1 cap stays in [0, 1] with MC, and the
    tracer masses drift by rounding only: C24, 20 steps."""
    N = 24
    e = Engine(_phys(2, 2, tracers=[0.75, "cap"]), TileLayout(N, 2, 1, ng=2), grid=_grid(N), device="cuda",
               backend="hip")
    A = e.tens["area"]
    m0 = [(e.tiles_view()[4 + k] * A).sum().item() for k in range(2)]
    e.step(20)
    torch.cuda.synchronize()
    v = e.tiles_view()
    q = v[4:] / v[0]
    dev = (q[0] - 0.75).abs().max().item()
    lo, hi = q[1].min().item(), q[1].max().item()
    drift = [abs((v[4 + k] * A).sum().item() - m0[k]) / abs(m0[k]) for k in range(2)]
    print(f"constancy {dev:.2e}; cap min {lo:.3e} max - 1 {hi - 1:.3e}; mass drift {drift}")
    assert dev < 1e-13
    assert -1e-12 <= lo and hi <= 1.0 + 1e-12
    assert max(drift) < 1e-13


def test_swe_fields_match_the_plain_stage_kernel():
    """h and M of a tracer run against the plain SWE run on stage_kernel.hip."""
    N = 24
    L = TileLayout(N, 2, 1, ng=2)
    worst = 0.0
    for block in BLOCKS:
        a = Engine(ShallowWater("tc5", limiter=2), L, grid=_grid(N), device="cuda", backend="hip", block=block)
        b = Engine(_phys(2, 2), L, grid=_grid(N), device="cuda", backend="hip", block=block, dt=a.dt)
        a.step(8)
        b.step(8)
        torch.cuda.synchronize()
        x, y = a.tiles_view().reshape(4, -1), b.tiles_view()[:4].reshape(4, -1)
        err = ((x - y).abs().amax(1) / x.abs().amax(1)).max().item()
        print(f"SWE fields, tracer kernel vs stage kernel, block {block}: rel diff {err:.3e}")
        worst = max(worst, err)
    assert worst < FP64_BOUND


def _solver(tmp, tracers):
    import stsphere as S
    c = {"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": "gpu"},
         "grid": {"N": 24}, "physics": {"model": "swe", "case": "tc5", "limiter": "mc"},
         "time": {"nsteps": 8, "dt": 150.0}, "io": {"output_dir": str(tmp)}, "runtime": {"fused": "off"}}
    if tracers:
        c["physics"]["tracers"] = tracers
    s = S.Solver(c, verbose=False)
    s.initialize()
    return s


def test_solver_diagnostics_on_a_tracer_run(tmp_path):
    """Vorticity, invariants, u and particle positions of a tracer run equal
    the plain run's (fused: off) to 1e-11; tracer(0) = hq0 / h."""
    lat, lon = np.linspace(-1.2, 1.2, 7), np.linspace(0.1, 6.0, 7)
    out = {}
    for name, tr in (("plain", None), ("tracers", ["cap", "gradient"])):
        s = _solver(tmp_path / name, tr)
        s.add_particles(lat, lon)
        s.step(8)
        out[name] = dict(vort=s.derived_field("vorticity"), inv=s.invariants(), u=s.latlon_field("u", 8, 16),
                         pos=np.stack(s.particle_positions()), s=s)
    a, b = out["plain"], out["tracers"]
    assert b["s"].fused is None and b["s"].engines[0].compute.phys_id == 3

    def rel(x, y):
        return float(np.abs(x - y).max() / np.abs(x).max())
    errs = {"vorticity": rel(a["vort"], b["vort"]), "u": rel(a["u"], b["u"]), "particles": rel(a["pos"], b["pos"]),
            # the circulation is a sum that cancels to rounding: measured against the sum of |zeta| A
            "invariants": max(abs(a["inv"][k] - b["inv"][k]) / abs(a["inv"]["abs_circulation" if k == "circulation" else k])
                              for k in a["inv"])}
    print(errs)
    assert max(errs.values()) < FP64_BOUND, errs
    s = b["s"]
    g = s.gather_global()
    assert np.array_equal(s.tracer(0), g[4] / g[0])
    assert s.latlon_field("q0", 8, 16).shape == (8, 16) and s.sample(["q1"], lat, lon).shape == (1, 7)
    for x in (a["s"], s):
        x.close()
