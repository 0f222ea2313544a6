"""Two-layer shallow water on the GPU: the stage kernel
``ops/csrc/swe_layer_stage.hip`` against its fp64 PyTorch twin
(``models/swe.py::LayeredShallowWater``), with the project's bounds: relative
error below 1e-11 for fp64 and below 1e-4 for fp32.  The case is ``tc5``: two
moving layers over the mountain, so grad b != 0 and the coupling gradient is
not zero either."""
import functools

import numpy as np
import pytest
import torch
import yaml

from stsphere.engine import Engine, VirtualCluster
from stsphere.models.geometry import CubedSphereGrid
from stsphere.ops.hip_compute import LAYER_LDS_MAX, choose_layer_block, layer_lds_bytes
from stsphere.parallel.layout import TileLayout

from layer_states import increment_error, install, layer_physics, make_state

pytestmark = pytest.mark.gpu

BLOCKS = [(16, 16), (16, 8)]
FP64_BOUND, FP32_BOUND = 1e-11, 1e-4


def _admitted(block, dtype=torch.float64):
    """The LDS rule: a launch stays inside 64 KiB."""
    return layer_lds_bytes(*block, torch.tensor([], dtype=dtype).element_size()) <= LAYER_LDS_MAX


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


@functools.lru_cache(maxsize=None)
def _reference(N, t, lim, integ, steps):
    """The twin's state after ``steps`` steps (fp64, computed once per case and
    shared by the block shapes and precisions), and its dt."""
    ref = Engine(layer_physics(lim), TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=torch.float64, device="cuda",
                 backend="torch", integrator=integ)
    ref.step(steps)
    torch.cuda.synchronize()
    return ref.tiles_view().detach().clone(), ref.dt


def _hip(N, t, lim, block, dtype=torch.float64, integ="ssprk3", dt=None):
    return Engine(layer_physics(lim), TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=dtype, device="cuda",
                  backend="hip", integrator=integ, block=block, dt=dt)


def _relerr(a, hip):
    F = a.shape[0]
    b = hip.tiles_view().double()
    assert bool(torch.isfinite(b).all()), f"{int((~torch.isfinite(b)).sum())} non-finite values in the hip state"
    a, b = a.reshape(F, -1), b.reshape(F, -1)
    return ((a - b).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).max().item()


def _check(N, t, lim, block, dtype=torch.float64, integ="ssprk3", steps=4):
    a, dt = _reference(N, t, lim, integ, steps)
    hip = _hip(N, t, lim, block, dtype, integ, dt)
    assert hip.compute.phys_id == 4 and (hip.compute.bx, hip.compute.by) == block
    hip.step(steps)
    torch.cuda.synchronize()
    err = _relerr(a, hip)
    print(f"C{N} t={t} lim={lim} block={block} {dtype} {integ}: rel err {err:.3e}")
    assert err < (FP64_BOUND if dtype == torch.float64 else FP32_BOUND)


def test_lds_rule():
    """The library's LDS byte count is the Python rule's (HipCompute asserts it
    at construction), 16x8 fp64 and both fp32 shapes fit, and 16x16 fp64 fits
    with the sound-speed row of the neighbour's raw cell recomputed."""
    assert layer_lds_bytes(16, 8, 8) == 40400 and layer_lds_bytes(16, 16, 4) == 32680
    assert layer_lds_bytes(16, 16, 8) == 65360 <= LAYER_LDS_MAX
    for block in BLOCKS:
        for dtype in (torch.float64, torch.float32):
            assert _admitted(block, dtype)
            _hip(24, 1, 2, block, dtype)
    assert choose_layer_block(48, 24, 256) == (16, 16) and choose_layer_block(180, 6, 256) == (16, 8)
    with pytest.raises(ValueError, match="two-layer shallow water runs blocks"):
        _hip(24, 1, 2, (8, 8))


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("t", [1, 2])
def test_kernel_matches_twin(t, lim, block):
    _check(24, t, lim, block)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_integrators(integ):
    _check(24, 2, 2, (16, 16), integ=integ)


@pytest.mark.parametrize("block", BLOCKS)
def test_fp32(block):
    _check(24, 2, 2, block, dtype=torch.float32)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("N,t", [(17, 1), (34, 2), (20, 1)])
def test_partial_blocks_and_one_cell_wide_last_block(N, t, block):
    """n = 17: the last block is one cell wide, so the last-but-one block's
    window reaches the ghost strip (block_sides); n = 20: a partial block."""
    _check(N, t, 2, block)


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("cls", ["rough", "plateau"])
def test_rough_start(cls, t):
    """Both layers rough, independently (layer_states): both signs of the depth
    flux and every slope arm in each layer, measured on the increment of one
    step, for every limiter."""
    N = 16
    L = TileLayout(N, t, 1, ng=2)
    for lim in (0, 1, 2, 3):
        ref = Engine(layer_physics(lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="torch")
        G = make_state(ref, cls)
        for block in BLOCKS:
            r = Engine(layer_physics(lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="torch",
                       dt=ref.dt)
            hip = Engine(layer_physics(lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="hip",
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
    gather (rows of 8 values) and the interior / boundary block lists."""
    N = 24
    mk = lambda: layer_physics(2)   # noqa: E731
    single = Engine(mk(), TileLayout(N, 2, 1, ng=2), grid=_grid(N), device="cuda", backend="hip")
    vc = VirtualCluster(mk, TileLayout(N, 2, ranks, ng=2), grid=_grid(N), device="cuda", backend="hip", dt=single.dt)
    single.step(5)
    vc.step(5)
    torch.cuda.synchronize()
    for f in range(8):
        a, b = single.global_field(f), vc.global_field(f)
        assert abs(a - b).max() <= 1e-12 * max(1.0, abs(a).max()), f


def test_uniform_layers_stay_at_rest():
    """``rest`` on the device: the coupling gradient of uniform layers is exactly
    zero in the kernel too, so the momenta stay at rounding level (the bound of
    the CPU test: ten times the floor 1e-13 H sqrt(g H))."""
    N = 24
    ph = layer_physics(2, case="rest", depths=[1000.0, 1000.0])
    e = Engine(ph, TileLayout(N, 2, 1, ng=2), grid=_grid(N), device="cuda", backend="hip")
    e.step(10)
    torch.cuda.synchronize()
    v = e.tiles_view()
    H = 2000.0
    m = max(float(v[1:4].abs().max()), float(v[5:8].abs().max()))
    print(f"rest, 10 steps on the device: max |M| {m:.3e}")
    assert m <= 10 * 1e-13 * H * (ph.g * H) ** 0.5


def test_layer_derived_fields():
    """vorticity, divergence and PV of each layer through the derived kernel
    (the layer's rows of the state; of the receive buffer on ranks with remote
    ghosts) against the twin's derived fields of the layer slice."""
    N = 24
    L = TileLayout(N, 2, 1, ng=2)
    hip = Engine(layer_physics(2), L, grid=_grid(N), device="cuda", backend="hip")
    ref = Engine(layer_physics(2), L, grid=_grid(N), device="cuda", backend="torch", dt=hip.dt)
    hip.step(3)
    ref.set_state(hip.tiles_view().clone())
    for k in (0, 1):
        a = ref.derived(layer=k)[0].clone()
        b = hip.derived(layer=k)[0].clone()
        torch.cuda.synchronize()
        for j, name in enumerate(("vorticity", "divergence", "pv")):
            err = float((a[j] - b[j]).abs().max() / a[j].abs().max())
            print(f"layer {k} {name}: rel err {err:.3e}")
            assert err < FP64_BOUND
    # the two layers differ (the bottom one feels the mountain)
    assert float((hip.derived(layer=0)[0].clone() - hip.derived(layer=1)[0]).abs().max()) > 0
    # eight virtual ranks: the receive buffer's layer columns
    mk = lambda: layer_physics(2)   # noqa: E731
    vc = VirtualCluster(mk, TileLayout(N, 2, 8, ng=2), grid=_grid(N), device="cuda", backend="hip", dt=hip.dt)
    vc.step(3)
    from rough_states import global_of
    from stsphere.engine import assemble_global
    one = assemble_global(L, {0: hip.derived(layer=1)[0][2].cpu().numpy()})
    ds = [e.derived_fields for e in vc.engines]
    for d in ds:
        d.set_layer(1)
        d.start()
    for d in ds:
        d.finish()
    many = assemble_global(vc.engines[0].layout, {e.rank: d.compute()[0][2].cpu().numpy()
                                                  for e, d in zip(vc.engines, ds)})
    assert global_of(vc.engines).shape[0] == 8
    assert np.abs(one - many).max() <= FP64_BOUND * np.abs(one).max()


def test_solver_run_history_metrics_restart(tmp_path):
    """``configs/c48_layers_tc2_1gpu.yaml`` shortened to a few steps: history
    with eta1 and pv0, metrics with mass0 / mass1, a checkpoint, and a restart
    onto the same trajectory."""
    import os
    import stsphere as S
    from stsphere.utils import checkpoint as ckpt
    from stsphere.utils.history import read_history, read_metrics
    path = os.path.join(S.__path__[0], "configs", "c48_layers_tc2_1gpu.yaml")
    with open(path) as f:
        cfg = yaml.safe_load(f)
    cfg["time"] = dict(cfg.get("time", {}), nsteps=6)
    cfg["time"].pop("days", None)
    cfg["io"] = {"output_dir": str(tmp_path / "run"), "history_interval": 3, "metrics_interval": 2,
                 "checkpoint_interval": 3, "history_fields": ["h0", "h1", "eta1", "pv0"]}
    s = S.Solver(cfg, verbose=False)
    s.run()
    assert s.engines[0].compute.phys_id == 4 and s.fused is None and s.step_count == 6
    g = s.gather_global()
    assert g.shape == (8, 6, 48, 48)
    hist = str(tmp_path / "run" / "history.zarr")
    assert np.array_equal(read_history(hist, "eta1")[-1], g[4])          # b = 0 in tc2
    assert np.array_equal(read_history(hist, "pv0")[-1], s.derived_field("pv0"))
    m = read_metrics(str(tmp_path / "run" / "metrics.jsonl"))
    assert len(m) == 3
    for rec in m:
        for k in ("mass0", "mass1"):
            assert abs(rec[k] - m[0][k]) <= 1e-13 * m[0][k]
        assert np.isfinite(rec["energy"])
    norms = s.error_norms()
    assert set(norms) >= {"h0_l2", "h1_l2"} and norms["h0_l2"] < 1e-3
    with pytest.raises(ValueError, match="layer"):
        s.invariants()
    root = str(tmp_path / "run" / "checkpoints")
    assert ckpt.list_checkpoints(root) == [0, 3, 6]      # 0: the watchdog of the config can roll back to the start
    cfg["io"] = {"output_dir": str(tmp_path / "run2"), "restore": ckpt.step_dir(root, 3)}
    s2 = S.Solver(cfg, verbose=False)
    s2.initialize()
    assert s2.step_count == 3
    s2.step(3)
    assert np.array_equal(s2.gather_global(), g)
    for x in (s, s2):
        x.close()
