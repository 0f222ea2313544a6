"""Batched ensembles on the GPU: one launch of ``stage_batch_kernel``
(ops/csrc/stage_kernel.hip) steps a stage of every member.  The batched kernel
runs the block body of the plain stage kernel with a base offset per member,
so every member must equal ``Engine(backend='hip', block=<the same shape>)``
run alone from the same state bit for bit.  The statistics kernel
(ops/csrc/ensemble_kernel.hip) against its twin (models/ensemble_stats.py)."""
import numpy as np
import pytest
import torch

from stsphere.engine import Engine
from stsphere.ensemble import Ensemble
from stsphere.models.advection import Advection
from stsphere.models.diffusion import Diffusion
from stsphere.models.ensemble_stats import ensemble_stats
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu


def _batched(factory, N, t, M, block, dtype=torch.float64, ng=2, integrator="ssprk3", steps_per_graph=100,
             amplitude=1e-3):
    grid = CubedSphereGrid(N)
    L = TileLayout(N, t, 1, ng=ng)
    ens = Ensemble(factory, L, M, amplitude=amplitude, grid=grid, dtype=dtype, device="cuda", backend="hip",
                   integrator=integrator, steps_per_graph=steps_per_graph, mode="batched", block=block)
    assert ens.native and ens.mode == "batched" and (block is None or ens.block == tuple(block))
    return ens, grid, L


def _alone(factory, grid, L, ens, state, nsteps, integrator="ssprk3"):
    e = Engine(factory(), L, grid=grid, dtype=ens.engines[0].dtype, device="cuda", backend="hip",
               integrator=integrator, dt=ens.dt, block=ens.block)
    e.set_state(state)
    e.step(nsteps)
    torch.cuda.synchronize()
    return e.tiles_view()


def _members_match(factory, N, t, M, block, nsteps, **kw):
    ens, grid, L = _batched(factory, N, t, M, block, **kw)
    start = [e.tiles_view().clone() for e in ens.engines]
    assert not torch.equal(start[0], start[M - 1]) or M == 1
    ens.run(nsteps)                                  # shorter than a graph chunk: eager batched launches
    torch.cuda.synchronize()
    integ = kw.get("integrator", "ssprk3")
    for m in range(M):
        got = ens.engines[m].tiles_view()
        alone = _alone(factory, grid, L, ens, start[m], nsteps, integ)
        assert bool(torch.isfinite(got).all())
        assert torch.equal(got, alone), (m, float((got - alone).abs().max()))
        assert not torch.equal(got, start[m])
    return ens


def test_batched_8x8_partial_blocks_odd_members():
    """C20, one tile per face, 8 x 8 blocks: 54 blocks per member (54 % 8 = 6, so
    the padded workgroups of the batched grid run), partial blocks, three
    members; topography (TC5), MC."""
    ens = _members_match(lambda: ShallowWater("tc5"), 20, 1, 3, (8, 8), 4)
    assert ens.engines[0].compute.nblocks == 54


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_batched_16x16_ten_wave_blocks(dtype):
    """C32 in 2 x 2 tiles (n = 16): whole 16 x 16 blocks take the border-wave
    panel-edge path; tile pushes and corner ghosts; five members."""
    _members_match(lambda: ShallowWater("tc5"), 32, 2, 5, (16, 16), 3, dtype=dtype)


def test_batched_ppm():
    _members_match(lambda: ShallowWater("tc2", limiter=4), 24, 1, 2, (16, 16), 2, ng=3)


@pytest.mark.parametrize("factory", [lambda: Advection("cosine_bell"), lambda: Diffusion()],
                         ids=["advection", "diffusion"])
def test_batched_rk4_accumulator(factory):
    """rk4: the accumulator is written in stage 1 with a null acc_in, read and
    written in place in stages 2 and 3 and is the X of stage 4."""
    _members_match(factory, 16, 1, 3, (16, 8), 3, integrator="rk4", amplitude=1e-2)


def test_batched_members_are_isolated():
    """A member of NaNs stays NaN and touches no other member."""
    factory = lambda: ShallowWater("tc5")
    ens, grid, L = _batched(factory, 20, 1, 3, (8, 8))
    ens.engines[1].set_state(torch.full_like(ens.engines[1].tiles_view(), float("nan")))
    start = [e.tiles_view().clone() for e in ens.engines]
    ens.run(3)
    torch.cuda.synchronize()
    for m in (0, 2):
        got = ens.engines[m].tiles_view()
        assert torch.equal(got, _alone(factory, grid, L, ens, start[m], 3))
    assert bool(torch.isnan(ens.engines[1].tiles_view()).all())


@pytest.mark.parametrize("integrator,nsteps", [("ssprk3", 10), ("euler", 5)])
def test_batched_graph_equals_eager(integrator, nsteps):
    """steps_per_graph = 4: chunks of 4 replayed, the rest stepped eagerly
    (euler: a remainder of 1 leaves the pools rotated; they are put back)."""
    factory = lambda: ShallowWater("tc5")
    graph, _, _ = _batched(factory, 24, 2, 3, None, integrator=integrator, steps_per_graph=4)
    eager, _, _ = _batched(factory, 24, 2, 3, None, integrator=integrator, steps_per_graph=100)
    assert graph.block == eager.block
    graph.prepare(nsteps)
    assert graph._graph is not None and graph._graph.k == 4
    graph.run(nsteps)
    eager.prepare(nsteps)
    assert eager._graph is None
    eager.run(nsteps)
    torch.cuda.synchronize()
    for m in range(3):
        assert torch.equal(graph.engines[m].tiles_view(), eager.engines[m].tiles_view())
        assert graph.engines[m].step_count == eager.engines[m].step_count == nsteps
        for k, b in enumerate(graph.batch):
            assert graph.engines[m].pool[k].data_ptr() == b[m].data_ptr()
    assert not torch.equal(graph.engines[1].tiles_view(), graph.engines[2].tiles_view())
    graph.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [4, 1])
def test_stats_kernel_against_twin(M, dtype):
    from stsphere.ops.hip_compute import choose_block
    ens, grid, L = _batched(lambda: ShallowWater("tc5"), 24, 2, M, None, dtype=dtype)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert ens.block == choose_block(12, 24 * M, cus, 2, 8 if dtype == torch.float64 else 4)
    ens.run(2)
    cells = 6 * 24 * 24
    tol = 2 * cells * np.finfo(np.float64).eps
    for field in (0, 3):
        a = ens.stats(field)
        a = dict(a, mean_field=a["mean_field"].clone(), var_field=a["var_field"].clone())
        b = ens.stats(field)
        x = torch.stack([e.tiles_view()[field] for e in ens.engines])
        tw = ensemble_stats(x, ens.engines[0].tens["area"].reshape(x.shape[1:]))
        for k in ("mean_field", "var_field"):
            assert a[k].dtype == torch.float64 and a[k].shape == (24, 12, 12)
            assert torch.equal(a[k], tw[k]) and torch.equal(b[k], tw[k])
        for k in ("mean", "spread_rms", "max_var"):
            assert a[k] == b[k]                                   # the same number on every run
        assert a["max_var"] == tw["max_var"]
        assert abs(a["spread_rms"] - tw["spread_rms"]) <= tol * tw["spread_rms"]
        if field == 0:       # the height is positive: its area-weighted mean is a sum of positive terms too
            assert abs(a["mean"] - tw["mean"]) <= tol * abs(tw["mean"])
        if M == 1:
            assert a["max_var"] == 0.0 and a["spread_rms"] == 0.0
        else:
            assert a["max_var"] > 0.0
