"""Batched ensembles (ensemble.py mode='batched') on the CPU: the [M, F, S]
storage and its lockstep rotation, members equal to their engines stepped
alone, the statistics twin against a direct evaluation of its formulas, the
refusals, and the argument checks of ``stsp_stage_batch_launch`` (which return
before any launch, so they need no GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from stsphere.engine import Engine
from stsphere.ensemble import Ensemble
from stsphere.models.advection import Advection
from stsphere.models.diffusion import ConsistentDiffusion
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import LayeredShallowWater, ShallowWater, ShallowWaterTracers
from stsphere.parallel.layout import TileLayout

GRID = CubedSphereGrid(8)
LAYOUT = TileLayout(8, 1, 1, ng=2)


def _ensemble(members=3, integrator="ssprk3", mode="batched", **kw):
    return Ensemble(lambda: ShallowWater("tc5"), LAYOUT, members, amplitude=1e-3, grid=GRID, integrator=integrator,
                    mode=mode, **kw)


def _shares_storage(ens):
    for m, e in enumerate(ens.engines):
        assert len(e.pool) == len(ens.batch) == e.integ.nbuf
        for k, b in enumerate(ens.batch):
            assert b.shape == (ens.members,) + tuple(e.pool[k].shape) and b.is_contiguous()
            assert e.pool[k].data_ptr() == b[m].data_ptr() and e.pool[k].is_contiguous()
            b[m, 0, 0] += 1.0                         # a write through the batch is seen through the pool
            assert e.pool[k][0, 0] == b[m, 0, 0]
            b[m, 0, 0] -= 1.0


@pytest.mark.parametrize("integrator,nsteps", [("ssprk3", 3), ("euler", 3)])
def test_batched_storage_and_members_match_single_runs(integrator, nsteps):
    """euler rotates its two buffers every step (rotation (1, 0), period 2): an
    odd step count leaves the pools rotated, in every member alike."""
    ens = _ensemble(3, integrator)
    assert ens.mode == "batched" and not ens.native
    _shares_storage(ens)
    start = [e.tiles_view().clone() for e in ens.engines]
    ref = Engine(ShallowWater("tc5"), LAYOUT, grid=GRID, integrator=integrator, dt=ens.dt)
    assert torch.equal(start[0], ref.tiles_view())               # member 0 unperturbed
    assert not torch.equal(start[1], start[2])
    ens.run(nsteps)
    _shares_storage(ens)
    for m in range(3):
        alone = Engine(ShallowWater("tc5"), LAYOUT, grid=GRID, integrator=integrator, dt=ens.dt)
        alone.set_state(start[m])
        alone.step(nsteps)
        assert torch.equal(ens.engines[m].tiles_view(), alone.tiles_view())
        assert ens.engines[m].step_count == nsteps
    assert ens.states().shape == (3, 4, 6, 8, 8)
    assert ens.global_fields(0).shape == (3, 6, 8, 8)


def _direct(x, area):
    """The formulas of models/ensemble_stats.py in numpy, member by member."""
    x = np.asarray(x, dtype=np.float64)
    M = x.shape[0]
    s = x[0].copy()
    for m in range(1, M):
        s = s + x[m]
    mean = s / M
    v = np.zeros_like(mean)
    for m in range(M):
        d = x[m] - mean
        v = v + d * d
    var = v / M
    A = np.asarray(area, dtype=np.float64)
    return mean, var, (A * mean).sum() / A.sum(), np.sqrt((A * var).sum() / A.sum()), var.max()


@pytest.mark.parametrize("mode", ["batched", "streams"])
def test_stats_twin_against_direct_evaluation(mode):
    ens = _ensemble(3, mode=mode)
    ens.run(2)
    cells = 6 * 8 * 8
    tol = 2 * cells * np.finfo(np.float64).eps
    for field in (0, 2):
        st = ens.stats(field)
        assert set(st) == {"mean_field", "var_field", "mean", "spread_rms", "max_var"}
        x = ens.states()[:, field].numpy()
        area = ens.engines[0].tens["area"].reshape(x.shape[1:]).numpy()
        mean, var, gm, rms, vmax = _direct(x, area)
        assert st["mean_field"].shape == (6, 8, 8) and st["mean_field"].dtype == torch.float64
        assert np.array_equal(st["mean_field"].numpy(), mean) and np.array_equal(st["var_field"].numpy(), var)
        assert st["max_var"] == vmax and vmax > 0
        assert abs(st["spread_rms"] - rms) <= tol * rms
        if field == 0:           # the height: positive everywhere, so the mean is a sum of positive terms too
            assert abs(st["mean"] - gm) <= tol * abs(gm)
    # sums of non-negative terms on both sides: 2 cells eps bounds any reordering
    sp = ens.spread()["spread_rms"]
    assert abs(ens.stats(0)["spread_rms"] - sp) <= tol * sp
    with pytest.raises(ValueError):
        ens.stats(4)


def test_stats_of_one_member_has_no_variance():
    ens = _ensemble(1)
    st = ens.stats(0)
    assert torch.equal(st["var_field"], torch.zeros(6, 8, 8, dtype=torch.float64))
    assert st["spread_rms"] == 0.0 and st["max_var"] == 0.0
    assert torch.equal(st["mean_field"], ens.engines[0].tiles_view()[0])


def test_batched_refusals():
    with pytest.raises(ValueError, match="mode"):
        _ensemble(2, mode="fused")
    with pytest.raises(ValueError, match="one rank"):
        Ensemble(lambda: ShallowWater("tc5"), TileLayout(8, 1, 6, ng=2), 2, grid=GRID, mode="batched")
    with pytest.raises(ValueError, match="two_pass"):
        Ensemble(lambda: ConsistentDiffusion(), LAYOUT, 2, grid=GRID, mode="batched")
    # the HIP-backend refusals come before anything touches the device
    hip = dict(grid=GRID, device="cuda", backend="hip", mode="batched")
    with pytest.raises(ValueError, match="kernel physics 3"):
        Ensemble(lambda: ShallowWaterTracers("tc5"), LAYOUT, 2, **hip)
    with pytest.raises(ValueError, match="kernel physics 4"):
        Ensemble(lambda: LayeredShallowWater("tc2"), LAYOUT, 2, **hip)
    with pytest.raises(ValueError, match="march"):
        Ensemble(lambda: ShallowWater("tc5"), LAYOUT, 2, block=(64, 4), **hip)


def test_batched_cli_from_config_cpu():
    from stsphere.__main__ import run_ensemble
    cfg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "sharding-the-sphere-fall-2025-jax-devlab-examples_amd", "configs", "plumbing_cpu.yaml")
    r = run_ensemble(cfg, 2, 1e-3, nsteps=2, batched=True)
    s = run_ensemble(cfg, 2, 1e-3, nsteps=2)
    assert r["mode"] == "batched" and s["mode"] == "streams" and not r["native"]
    assert r["field0_spread_rms_final"] == s["field0_spread_rms_final"] > 0


def test_batch_launch_argument_checks():
    """members = 0, a stride shorter than F * S and a descriptor with remote
    set return their documented codes; so do the refused shapes and physics."""
    from stsphere.ops import native
    if not os.path.exists(native.lib_path()):
        pytest.skip("library not built")
    lib = ctypes.CDLL(native.lib_path(), mode=ctypes.RTLD_GLOBAL)
    assert hasattr(lib, "stsp_stage_batch_launch")
    fn = lib.stsp_stage_batch_launch
    ci = ctypes.c_int
    fn.argtypes = [ci, ci, ci, ci, ctypes.POINTER(native.StageDesc), ci, ctypes.c_longlong, ctypes.c_void_p]
    fn.restype = ci
    d = native.StageDesc()
    d.ntile, d.n, d.mg, d.pw = 6, 8, 2, 12
    d.S = 6 * 12 * 12
    d.nblocks = 6
    F = 4                                             # shallow water
    assert fn(2, 1, 16, 16, d, 0, F * d.S, None) == -20
    assert fn(2, 1, 16, 16, d, -3, F * d.S, None) == -20
    assert fn(2, 1, 16, 16, d, (1 << 31) // 8, F * d.S, None) == -20     # 8 * members workgroups pass 2^31
    assert fn(2, 1, 16, 16, d, 3, F * d.S - 1, None) == -21
    assert fn(0, 0, 8, 8, d, 3, d.S - 1, None) == -21                      # advection: F = 1
    d.remote = 1
    assert fn(2, 1, 16, 16, d, 3, F * d.S, None) == -22
    d.remote, d.xg = 0, 1
    assert fn(2, 1, 16, 16, d, 3, F * d.S, None) == -22
    d.xg = 0
    assert fn(2, 1, 64, 4, d, 3, F * d.S, None) == -2                      # the streaming stage
    assert fn(3, 1, 16, 16, d, 3, F * d.S, None) == -3 and fn(4, 1, 16, 16, d, 3, F * d.S, None) == -3
    assert fn(2, 7, 16, 16, d, 3, F * d.S, None) == -4
