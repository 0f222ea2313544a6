"""Three to eight stacked layers on the GPU: the layer-streaming stage kernel
``ops/csrc/swe_layers_stream.hip`` against its fp64 PyTorch twin
(``models/swe.py::LayeredShallowWater``), with the project's bounds: relative
error below 1e-11 for fp64 and below 1e-4 for fp32.  The case is ``tc5``:
every layer moves over the mountain, so grad b != 0 and no coupling gradient
is zero.  L = 3 starts the recurrences of the kernel's layer pass, L = 4 has
two middle layers (layers above and below each), L = 8 is the ceiling."""
import functools
import os

import numpy as np
import pytest
import torch
import yaml

from stsphere.engine import Engine, VirtualCluster, assemble_global
from stsphere.models.geometry import CubedSphereGrid
from stsphere.ops.hip_compute import LAYER_LDS_MAX, layers_stream_lds_bytes
from stsphere.parallel.layout import TileLayout

from layer_states import increment_error, install, layer_physics, make_state

pytestmark = pytest.mark.gpu

BLOCKS = [(16, 16), (16, 8)]
FP64_BOUND, FP32_BOUND = 1e-11, 1e-4


def _phys(nl, lim=2, case="tc5", depths=None):
    return layer_physics(lim, case=case, depths=depths or [2000.0] * (nl - 1) + [5960.0])


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


@functools.lru_cache(maxsize=None)
def _reference(nl, N, t, lim, integ, steps):
    """The twin's state after ``steps`` steps (fp64, computed once per case and
    shared by the block shapes and precisions), and its dt."""
    ref = Engine(_phys(nl, lim), TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=torch.float64, device="cuda",
                 backend="torch", integrator=integ)
    ref.step(steps)
    torch.cuda.synchronize()
    return ref.tiles_view().detach().clone(), ref.dt


def _hip(nl, N, t, lim, block, dtype=torch.float64, integ="ssprk3", dt=None):
    return Engine(_phys(nl, lim), TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=dtype, device="cuda",
                  backend="hip", integrator=integ, block=block, dt=dt)


def _check(nl, N, t, lim, block, dtype=torch.float64, integ="ssprk3", steps=4):
    a, dt = _reference(nl, N, t, lim, integ, steps)
    hip = _hip(nl, N, t, lim, block, dtype, integ, dt)
    assert hip.compute.phys_id == 4 and (hip.compute.bx, hip.compute.by) == block
    hip.step(steps)
    torch.cuda.synchronize()
    F = a.shape[0]
    b = hip.tiles_view().double()
    assert bool(torch.isfinite(b).all()), f"{int((~torch.isfinite(b)).sum())} non-finite values in the hip state"
    a, b = a.reshape(F, -1), b.reshape(F, -1)
    err = ((a - b).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).max().item()
    print(f"L={nl} C{N} t={t} lim={lim} block={block} {dtype} {integ}: rel err {err:.3e}")
    assert err < (FP64_BOUND if dtype == torch.float64 else FP32_BOUND)


def test_lds_rule_and_layer_ceiling():
    for block in BLOCKS:
        for dtype, es in ((torch.float64, 8), (torch.float32, 4)):
            sizes = {layers_stream_lds_bytes(*block, es, nl) for nl in range(3, 9)}
            assert len(sizes) == 1 and sizes.pop() <= LAYER_LDS_MAX
            _hip(3, 24, 1, 2, block, dtype)        # HipCompute asserts the library's export equals the rule
    assert layers_stream_lds_bytes(16, 16, 8) == 50384 and layers_stream_lds_bytes(16, 8, 8) == 30800
    with pytest.raises(ValueError, match="2 to 8 layers, not 9"):
        Engine(layer_physics(2, case="rest", depths=[500.0] * 9), TileLayout(24, 1, 1, ng=2), grid=_grid(24),
               device="cuda", backend="hip")


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("nl", [3, 4, 8])
def test_kernel_matches_twin(nl, t, lim, block):
    _check(nl, 24, t, lim, block)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("N,t", [(17, 1), (34, 2), (20, 1)])
def test_partial_blocks_and_one_cell_wide_last_block(N, t, block):
    _check(3, N, t, 2, block)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_integrators(integ):
    _check(3, 24, 2, 2, (16, 16), integ=integ)


@pytest.mark.parametrize("block", BLOCKS)
def test_fp32(block):
    _check(3, 24, 2, 2, block, dtype=torch.float32)


@pytest.mark.parametrize("cls", ["rough", "plateau"])
def test_rough_start(cls):
    """Every layer rough, independently (layer_states): the increment of one
    step, for every limiter and both blocks."""
    N = 16
    L = TileLayout(N, 1, 1, ng=2)
    for lim in (0, 1, 2, 3):
        mk = lambda backend, **kw: Engine(_phys(3, lim), L, grid=_grid(N), dtype=torch.float64, device="cuda",   # noqa: E731
                                          backend=backend, **kw)
        ref = mk("torch")
        G = make_state(ref, cls)
        for block in BLOCKS:
            r, hip = mk("torch", dt=ref.dt), mk("hip", block=block, dt=ref.dt)
            q0 = install(r, G)
            install(hip, G)
            r.step(1)
            hip.step(1)
            torch.cuda.synchronize()
            errs = increment_error(r, hip, q0, bound=FP64_BOUND, block=block, what=f"{cls} lim {lim} block {block}")
            print(f"{cls} lim={lim} block={block}: increment errors {['%.2e' % e for e in errs]}")


@pytest.mark.parametrize("ranks", [2, 8])
def test_remote_ghosts_virtual_ranks(ranks):
    """Several virtual ranks on one GPU against one rank: receive-buffer rows
    of 12 values and the interior / boundary block lists."""
    N = 24
    mk = lambda: _phys(3)   # noqa: E731
    single = Engine(mk(), TileLayout(N, 2, 1, ng=2), grid=_grid(N), device="cuda", backend="hip")
    vc = VirtualCluster(mk, TileLayout(N, 2, ranks, ng=2), grid=_grid(N), device="cuda", backend="hip", dt=single.dt)
    single.step(5)
    vc.step(5)
    torch.cuda.synchronize()
    for f in range(12):
        a, b = single.global_field(f), vc.global_field(f)
        assert abs(a - b).max() <= 1e-12 * max(1.0, abs(a).max()), f


def test_uniform_layers_stay_at_rest():
    """The kernel's face and cell accumulators go through the same operations:
    uniform layers give a coupling gradient of exactly zero."""
    ph = _phys(3, case="rest", depths=[1000.0] * 3)
    e = Engine(ph, TileLayout(24, 2, 1, ng=2), grid=_grid(24), device="cuda", backend="hip")
    e.step(10)
    torch.cuda.synchronize()
    v = e.tiles_view()
    H = 3000.0
    m = max(float(v[4 * k + 1:4 * k + 4].abs().max()) for k in range(3))
    print(f"rest, three layers, 10 steps on the device: max |M| {m:.3e}")
    assert m <= 10 * 1e-13 * H * (ph.g * H) ** 0.5


def test_solver_run_metrics_and_derived(tmp_path):
    """``configs/c48_layers3_tc2_1gpu.yaml`` shortened to a few steps."""
    import stsphere as S
    from stsphere.utils.history import read_metrics
    with open(os.path.join(S.__path__[0], "configs", "c48_layers3_tc2_1gpu.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["time"] = {"integrator": "ssprk3", "nsteps": 4}
    cfg["io"] = {"output_dir": str(tmp_path / "run"), "metrics_interval": 2, "history_fields": ["h2", "eta2"]}
    s = S.Solver(cfg, verbose=False)
    s.run()
    hip = s.engines[0]
    assert hip.compute.phys_id == 4 and hip.compute._layers == 3 and s.fused is None and s.step_count == 4
    m = read_metrics(str(tmp_path / "run" / "metrics.jsonl"))
    for rec in m:
        for k in ("mass0", "mass1", "mass2"):
            assert abs(rec[k] - m[0][k]) <= 1e-13 * m[0][k]
        assert np.isfinite(rec["energy"])
    assert set(s.error_norms()) >= {"h0_l2", "h1_l2", "h2_l2"}
    ref = Engine(_phys(3, case="tc2", depths=[4000.0] * 3), hip.layout, grid=hip.grid, device="cuda", backend="torch",
                 dt=hip.dt)
    ref.set_state(hip.tiles_view().clone())
    a = assemble_global(hip.layout, {0: ref.derived(layer=2)[0][0].cpu().numpy()})
    b = s.derived_field("vorticity2")
    assert np.abs(a - b).max() < FP64_BOUND * np.abs(a).max()
    s.close()
