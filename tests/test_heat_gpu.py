"""The gfx950 heat kernels (ops/csrc/heat_kernel.hip) against their PyTorch twin
(models/diffusion.py) through the engine, with the project's bounds, and the
plumbing through the solver.  Measured values: profiles/heat/README.md."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import rough_states as rs
from stsphere.driver import Solver
from stsphere.engine import Engine, VirtualCluster
from stsphere.models.diffusion import ConsistentDiffusion
from stsphere.ops import heat
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

# (N, tiles per edge): 16 + a partial block of 8; 16 + a partial block one cell wide;
# n = 12 with tile edges inside panels
SHAPES = [(24, 1), (17, 1), (24, 2)]
INTEGRATORS = ["euler", "ssprk2", "ssprk3", "rk4"]


def _engine(N, t, device, integ="ssprk3", case="lima_flag", dtype=torch.float64):
    return Engine(ConsistentDiffusion(case=case), TileLayout(N, t, 1, ng=2), grid=rs.grid_of(N), dtype=dtype,
                  device=device, backend="hip" if device != "cpu" else "torch", integrator=integ)


@functools.lru_cache(maxsize=None)
def _state(N, kind):
    """Global fp64 state [1, 6, N, N]: the rough ``scalar`` state on the Lima flag's scale,
    or the l = 3, m = 2 harmonic."""
    if kind == "rough":
        return rs.make_state(_engine(N, 1, "cpu"), "scalar")
    return rs.global_of(_engine(N, 1, "cpu", case="harmonic32"))


@functools.lru_cache(maxsize=None)
def _twin_steps(N, t, integ, kind, fp32=False):
    """The torch engine's state after 1 and after 3 steps, [1, T, n, n] each."""
    e = _engine(N, t, "cpu", integ, dtype=torch.float32 if fp32 else torch.float64)
    assert not e.compute.op.hip
    rs.install(e, _state(N, kind))
    e.step(1)
    a = e.tiles_view().clone()
    e.step(2)
    return a, e.tiles_view().clone()


def _err(got, ref):
    got, ref = got.double().cpu(), ref.double()
    return float((got - ref).abs().max() / ref.abs().max())


# ---- 8. hip engine against the torch engine -------------------------------------------------------

@pytest.mark.parametrize("kind", ["rough", "harmonic32"])
@pytest.mark.parametrize("integ", INTEGRATORS)
@pytest.mark.parametrize("N,t", SHAPES)
def test_engine_matches_twin(N, t, integ, kind):
    r1, r3 = _twin_steps(N, t, integ, kind)
    g = _engine(N, t, "cuda:0", integ)
    assert g.compute.op.hip
    q0 = rs.install(g, _state(N, kind))
    g.step(1)
    torch.cuda.synchronize()
    e1, b1 = _err(g.tiles_view(), r1), torch.equal(g.tiles_view().cpu(), r1)
    g.step(2)
    torch.cuda.synchronize()
    e3, b3 = _err(g.tiles_view(), r3), torch.equal(g.tiles_view().cpu(), r3)
    moved = float((g.tiles_view().cpu() - q0).abs().max())
    print(f"C{N} t={t} {integ} {kind}: error / max |T| after 1 step {e1:.2e} (bitwise {b1}), after 3 {e3:.2e} "
          f"(bitwise {b3}); moved {moved:.3e}")
    assert bool(torch.isfinite(g.tiles_view()).all()) and moved > 0
    assert e1 <= 1e-12 and e3 <= 1e-12


# ---- 9. fp32 state ----------------------------------------------------------------------------------

@pytest.mark.parametrize("integ", ["ssprk3", "rk4"])
def test_fp32_state(integ):
    N, t = 24, 1
    r1, r3 = _twin_steps(N, t, integ, "rough", fp32=True)
    g = _engine(N, t, "cuda:0", integ, dtype=torch.float32)
    rs.install(g, _state(N, "rough"))
    g.step(1)
    e1 = _err(g.tiles_view(), r1)
    g.step(2)
    torch.cuda.synchronize()
    e3 = _err(g.tiles_view(), r3)
    print(f"fp32 C{N} {integ}: error / max |T| after 1 step {e1:.2e}, after 3 {e3:.2e}")
    assert g.tiles_view().dtype == torch.float32 and bool(torch.isfinite(g.tiles_view()).all())
    assert e1 <= 1e-6 and e3 <= 1e-6


# ---- 10. virtual ranks on one GPU ----------------------------------------------------------------

@pytest.mark.parametrize("nd", [2, 8])
@pytest.mark.parametrize("integ", ["ssprk3", "rk4"])
def test_virtual_ranks_match_one_rank(integ, nd):
    N, t = 24, 2
    one = _engine(N, t, "cuda:0", integ)
    rs.install(one, _state(N, "rough"))
    one.step(3)
    vc = VirtualCluster(lambda: ConsistentDiffusion(), TileLayout(N, t, nd, ng=2), grid=rs.grid_of(N),
                        device="cuda:0", backend="hip", integrator=integ)
    for e in vc.engines:
        assert e.compute.op.hip
        rs.install(e, _state(N, "rough"))
    vc.step(3)
    torch.cuda.synchronize()
    a, b = rs.global_of(one), rs.global_of(vc.engines)
    print(f"{nd} virtual ranks {integ}: max difference {float((a - b).abs().max()):.2e}, bitwise {torch.equal(a, b)}")
    assert torch.equal(a, b)
    assert _err(one.tiles_view(), _twin_steps(N, t, integ, "rough")[1]) <= 1e-12


# ---- 11. ghost slots and corners -----------------------------------------------------------------

@pytest.mark.parametrize("integ", ["euler", "ssprk3"])
def test_ghost_slots_are_current_after_a_step(integ):
    g = _engine(24, 2, "cuda:0", integ)
    rs.install(g, _state(24, "rough"))
    g.step(1)
    torch.cuda.synchronize()
    # euler's new state is the other buffer (ghost slots still zero), SSP-RK3's the installed one
    # (ghost slots of the old state): neither passes without the refresh at the end of the step
    ref = g.state.clone()
    g.refresh_halos(ref)
    assert torch.equal(ref, g.state) and bool((g.state[:, g.halo_dst] != 0).any())


def test_no_corner_ghost_is_read():
    g = _engine(24, 2, "cuda:0", "rk4")
    rs.install(g, _state(24, "rough"))
    g.poison_corners()
    g.compute.op.scratch[:, g.corner_slots()] = float("nan")
    g.step(3)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g.tiles_view()).all())
    assert _err(g.tiles_view(), _twin_steps(24, 2, "rk4", "rough")[1]) <= 1e-12


# ---- 12. store-L mode ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rough", "harmonic32"])
@pytest.mark.parametrize("N,t", SHAPES)
def test_laplacian_matches_twin(N, t, kind):
    c, g = _engine(N, t, "cpu"), _engine(N, t, "cuda:0")
    rs.install(c, _state(N, kind))
    rs.install(g, _state(N, kind))
    ref = c.heat_operator().laplacian()
    assert g.heat_operator().hip and not c.heat_operator().hip
    got = g.heat_operator().laplacian()
    torch.cuda.synchronize()
    err = _err(got, ref)
    print(f"laplacian C{N} t={t} {kind}: error / max |L T| {err:.2e}, bitwise {torch.equal(got.cpu(), ref)}")
    assert bool(torch.isfinite(got).all()) and float(ref.abs().max()) > 0 and err <= 1e-11


def _cfg(out, device, N=24, t=2, nd=1, backend="auto"):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": device},
            "grid": {"N": N, "halo": 2, "dtype": "float64"},
            "physics": {"model": "diffusion", "case": "harmonic", "operator": "consistent"},
            "time": {"integrator": "ssprk3"}, "io": {"output_dir": str(out)},
            "runtime": {"backend": backend, "steps_per_graph": 4}}


def test_solver_laplacian_matches_twin(tmp_path):
    g = Solver(_cfg(tmp_path / "g", "gpu", nd=6), verbose=False)
    c = Solver(_cfg(tmp_path / "c", "cpu"), verbose=False)
    g.initialize()
    c.initialize()
    a, b = g.laplacian("T"), c.laplacian("T")
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"Solver.laplacian('T') C24, 6 virtual ranks on the GPU: error / max |L T| {err:.2e}")
    assert all(e.heat_operator().hip for e in g.engines) and err <= 1e-11


# ---- 13. the solver -------------------------------------------------------------------------------

def test_solver_hip_matches_torch_backend(tmp_path):
    g = Solver(_cfg(tmp_path / "g", "gpu"), verbose=False)
    c = Solver(_cfg(tmp_path / "c", "cpu"), verbose=False)
    sg = g.run(nsteps=8)
    c.run(nsteps=8)
    a, b = g.gather_global(), c.gather_global()
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"solver harmonic C24, 8 steps, runtime {sg['runtime']}: {err:.3e}; err_linf {sg['err_linf']:.3e}")
    assert err <= 1e-11
    assert g.backend == "hip" and g.runner is None and sg["runtime"] == "eager" and g.engines[0].compute.op.hip
    e = g.engines[0]
    q = e.state.clone()
    e.refresh_halos(q)
    assert torch.equal(q, e.state)
    g.close()


# ---- the entry point validates its descriptor ------------------------------------------------------

def test_entry_point_rejects_bad_descriptors():
    g = _engine(17, 1, "cuda:0")
    op = g.compute.op
    assert op.lib.stsp_heat_desc_size() == ctypes.sizeof(heat.HeatDesc)
    stream = 0

    def rc(dtype=1, **kw):
        d = heat.HeatDesc()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(op.desc), ctypes.sizeof(d))
        d.pass_, d.mode = 2, 0
        for k, v in kw.items():
            setattr(d, k, v)
        return op.lib.stsp_heat_launch(dtype, d, stream)
    assert rc(n=0) == 1 and rc(S=op.S + 1) == 1 and rc(nblocks=op.nblocks + 1) == 1 and rc(pw=op.n) == 1
    assert rc(pass_=3) == 1 and rc(mode=3) == 1 and rc(lout=0) == 1 and rc(scratch=0) == 1
    assert rc(mode=1, out=0) == 1 and rc(pass_=1, q=0) == 1 and rc(nrecv=1, srecv=0) == 1
    assert rc(dtype=2) == 2
    torch.cuda.synchronize()
