"""Every limiter and flux branch of the stencil kernels (GPU): the block stage
kernel in all shapes, the streaming stage, the pipelined streaming step and
the fused step against the fp64 PyTorch oracle, started from the rough states
of tests/rough_states.py and measured on the increment (state - start), not
on the carried state.

Unless stated otherwise a case runs two SSP-RK3 steps with the oracle's dt and
asserts ``increment_error`` per field below 1e-11 (fp64; two fp64 renderings
of the algorithm agree to 7e-15 on these states, tests/test_rough_states.py).
Every case prints its measured errors; profiles/rough/README.md records them."""
import functools

import pytest
import torch

from rough_states import (TopographySWE, fp32_twin_bound, global_of, grid_of, increment_error, install,
                          make_state)
from stsphere.engine import Engine, VirtualCluster
from stsphere.models.advection import Advection
from stsphere.models.diffusion import Diffusion
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

BOUND = 1e-11
STEPS = 2


def _physics(kind, lim):
    if kind == "adv":
        return Advection(limiter=lim)
    if kind == "diff":
        return Diffusion()
    if kind == "topo":                  # tc5 over topography in every cell (tests/test_topography_kernels.py)
        return TopographySWE("tc5", limiter=lim)
    return ShallowWater(kind, limiter=lim)


@functools.lru_cache(maxsize=None)
def _global(kind, N, cls):
    """The global start state of a class: a function of the case and the grid
    alone (not of the limiter, the layout or the precision)."""
    phys = _physics(kind, 2)
    return make_state(Engine(phys, TileLayout(N, 1, 1, ng=phys.halo), grid=grid_of(N)), cls)


def _engine(kind, N, t, lim, cls, backend="torch", dtype=torch.float64, integ="ssprk3", block=None, dt=None,
            rounded=False):
    """(engine on the GPU with the class's state installed, q0).  ``rounded``:
    the state rounded to fp32 first (the start of the fp32 comparisons)."""
    phys = _physics(kind, lim)
    e = Engine(phys, TileLayout(N, t, 1, ng=phys.halo), grid=grid_of(N), dtype=dtype, device="cuda",
               backend=backend, integrator=integ, block=block, dt=dt)
    G = _global(kind, N, cls)
    return e, install(e, G.float().double() if rounded else G)


@functools.lru_cache(maxsize=None)
def _reference(kind, N, t, lim, cls, integ="ssprk3", steps=STEPS, rounded=False):
    """(oracle engine after ``steps`` steps, q0): computed once per case and
    shared by every kernel shape that runs it; never stepped again."""
    ref, q0 = _engine(kind, N, t, lim, cls, integ=integ, rounded=rounded)
    ref.step(steps)
    torch.cuda.synchronize()
    return ref, q0


def _check(ref, hip, q0, block, what, bound=BOUND):
    torch.cuda.synchronize()
    errs = increment_error(ref, hip, q0, block=block, what=what)      # raises on a NaN
    print(f"ROUGH {what}: " + " ".join(f"{x:.2e}" for x in errs))
    increment_error(ref, hip, q0, bound=bound, block=block, what=what)
    return errs


def _block_case(kind, N, t, lim, cls, block, integ="ssprk3", steps=STEPS):
    ref, q0 = _reference(kind, N, t, lim, cls, integ, steps)
    hip, _ = _engine(kind, N, t, lim, cls, backend="hip", integ=integ, block=block, dt=ref.dt)
    hip.step(steps)
    _check(ref, hip, q0, block, f"{kind} {cls} limiter {lim} C{N} t={t} block {block[0]}x{block[1]} {integ}")


# ---- block stage kernel -------------------------------------------------------------------
@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("N,t,block", [
    (48, 1, (16, 16)),       # full ten-wave blocks, border-wave fix-up, one interior block per panel, cube corners
    (20, 1, (16, 16)),       # partial blocks, block-wide fix-up
    (24, 2, (16, 8)), (24, 2, (8, 16)), (24, 2, (32, 8)), (24, 2, (8, 8)),   # tile corners with carried ghosts
])
def test_block_kernel_rough(N, t, block, lim):
    _block_case("tc5", N, t, lim, "rough", block)


@pytest.mark.parametrize("N,block", [(25, (8, 8)), (33, (16, 16))])
def test_block_kernel_rough_block_ends_one_cell_from_the_panel_edge(N, block):
    _block_case("tc5", N, 1, 2, "rough", block)


@pytest.mark.parametrize("N,t,block", [(48, 1, (16, 16)), (24, 2, (16, 8)), (34, 1, (16, 16))])
def test_block_kernel_rough_ppm(N, t, block):
    _block_case("tc5", N, t, 4, "rough", block)


# PPM is not built for 8x8 blocks
@pytest.mark.parametrize("cls", ["plateau", "zero_mom"])
@pytest.mark.parametrize("lim,block", [(lim, b) for b in ((16, 16), (8, 8)) for lim in (1, 2, 3, 4)
                                       if (lim, b) != (4, (8, 8))])
def test_block_kernel_exact_zero_differences(lim, block, cls):
    _block_case("tc5", 24, 2, lim, cls, block)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_block_kernel_rough_integrators(integ):
    """One step: with euler a single RHS evaluation, the sharpest comparison."""
    _block_case("tc5", 16, 1, 2, "rough", (16, 16), integ=integ, steps=1)


@pytest.mark.parametrize("N,t,block,kind,lim", [
    (N, t, b, kind, lim) for N, t, b in ((24, 2, (16, 16)), (20, 1, (8, 8)))
    for kind, lim in (("adv", 1), ("adv", 2), ("adv", 3), ("adv", 4), ("diff", 0)) if (lim, b) != (4, (8, 8))])
def test_block_kernel_scalar_class(N, t, block, kind, lim):
    _block_case(kind, N, t, lim, "scalar", block)


# ---- streaming stage (64, R) ---------------------------------------------------------------
@pytest.mark.parametrize("lim", [0, 1, 2, 3])
def test_march_rough_limiters(lim):
    """C24: both halo lanes of the one wave are panel-edge ghosts."""
    _block_case("tc5", 24, 1, lim, "rough", (64, 8))


@pytest.mark.parametrize("N,t,R", [(72, 1, 16), (25, 1, 8), (50, 2, 4)])
def test_march_rough_shapes(N, t, R):
    """Two strips with a partial last strip; an odd tile; four rows per wave."""
    _block_case("tc5", N, t, 2, "rough", (64, R))


@pytest.mark.parametrize("cls", ["plateau", "zero_mom"])
@pytest.mark.parametrize("lim", [1, 2, 3])
def test_march_exact_zero_differences(lim, cls):
    _block_case("tc5", 24, 1, lim, cls, (64, 8))


def test_march_agrees_with_block_kernel_on_rough():
    """The streaming stage and the 8x8 block kernel within 1e-12 of the increment."""
    a, q0 = _engine("tc5", 48, 1, 2, "rough", backend="hip", block=(8, 8))
    b, _ = _engine("tc5", 48, 1, 2, "rough", backend="hip", block=(64, 16), dt=a.dt)
    a.step(STEPS)
    b.step(STEPS)
    _check(a, b, q0, (64, 16), "march (64, 16) against block 8x8, rough limiter 2 C48 t=1", bound=1e-12)


# ---- pipelined streaming step ----------------------------------------------------------------
def _march3_case(N, t, lim, cls, R):
    from stsphere.ops.march3 import March3Step
    ref, q0 = _reference("tc5", N, t, lim, cls)
    hip, _ = _engine("tc5", N, t, lim, cls, backend="hip", dt=ref.dt)
    m3 = March3Step(hip, rows=R)
    m3.step(STEPS)
    _check(ref, hip, q0, (64, R), f"march3 {cls} limiter {lim} C{N} t={t} rows {R}")


@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("N,R", [(48, 16), (50, 32)])
def test_march3_rough(N, R, lim):
    """March and band launches together, as March3Step issues a step."""
    _march3_case(N, 1, lim, "rough", R)


def test_march3_plateau():
    _march3_case(48, 1, 2, "plateau", 16)


# ---- fused step --------------------------------------------------------------------------------
FUSED_SHAPES = [(12, 1, 6), (36, 2, 6), (32, 2, 8), (48, 4, 12), (96, 2, 16), (54, 1, 18), (60, 3, 20)]


def _fused_case(N, t, B, lim, cls):
    from stsphere.ops.fused import FusedKernel
    ref, q0 = _reference("tc5", N, t, lim, cls)
    hip, _ = _engine("tc5", N, t, lim, cls, backend="hip", dt=ref.dt)
    fk = FusedKernel(hip, B=B)
    for _ in range(STEPS):
        fk.step(1)
    torch.cuda.synchronize()
    fk.check()
    _check(ref, hip, q0, (B, B), f"fused {cls} limiter {lim} C{N} t={t} B={B}")


@pytest.mark.parametrize("lim", [1, 2, 3])
@pytest.mark.parametrize("N,t,B", FUSED_SHAPES)
def test_fused_rough(N, t, B, lim):
    """One launch per step, one shape per block size."""
    _fused_case(N, t, B, lim, "rough")


def test_fused_rough_unlimited():
    _fused_case(32, 2, 8, 0, "rough")


@pytest.mark.parametrize("cls", ["plateau", "zero_mom"])
@pytest.mark.parametrize("lim", [2, 3])
@pytest.mark.parametrize("N,t,B", [(32, 2, 8), (12, 1, 6)])
def test_fused_exact_zero_differences(N, t, B, lim, cls):
    _fused_case(N, t, B, lim, cls)


@pytest.mark.parametrize("handoff", ["tag", "epoch"])
def test_fused_four_step_launch_on_rough(monkeypatch, handoff):
    """Four steps in one launch equal four single-step launches bit for bit
    (both in-launch hand-off forms), and the oracle on the increment."""
    from stsphere.ops.fused import FusedKernel
    monkeypatch.setenv("STSP_FUSED_HANDOFF", handoff)
    ref, q0 = _reference("tc5", 32, 2, 2, "rough", steps=4)
    a, _ = _engine("tc5", 32, 2, 2, "rough", backend="hip", dt=ref.dt)
    b, _ = _engine("tc5", 32, 2, 2, "rough", backend="hip", dt=ref.dt)
    FusedKernel(a).step(4)
    fk = FusedKernel(b)
    assert fk.handoff == handoff
    fk.launch(0, nsteps=4)
    torch.cuda.synchronize()
    fk.check()
    assert torch.equal(a.pool[0], b.pool[0])
    _check(ref, b, q0, (fk.plan.B,) * 2, f"fused four-step launch ({handoff}) rough limiter 2 C32 t=2")


# ---- remote-ghost path ------------------------------------------------------------------------
@pytest.mark.parametrize("ranks", [2, 8])
def test_remote_ghost_path_on_rough(ranks):
    """Virtual ranks (receive-buffer gather, interior / boundary block split)
    against the one-rank HIP engine, within 1e-12 of the field maximum."""
    N, t = 24, 2
    single, _ = _engine("tc5", N, t, 2, "rough", backend="hip")
    vc = VirtualCluster(lambda: ShallowWater("tc5"), TileLayout(N, t, ranks, ng=2), grid=grid_of(N), device="cuda",
                        backend="hip", dt=single.dt)
    for e in vc.engines:
        install(e, _global("tc5", N, "rough"))
    single.step(STEPS)
    vc.step(STEPS)
    torch.cuda.synchronize()
    a, b = global_of(single), global_of(vc.engines)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    for f in range(4):
        d = float((a[f] - b[f]).abs().max())
        print(f"ROUGH remote ghosts {ranks} ranks field {f}: {d / float(a[f].abs().max()):.2e} of the field maximum")
        assert d <= 1e-12 * max(1.0, float(a[f].abs().max())), f


# ---- fp32 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,t", [("block", 24, 2), ("march", 24, 1), ("march3", 48, 1), ("fused", 32, 2)])
def test_fp32_rough(family, N, t):
    ref, q0, twin, _ = fp32_twin_bound("tc5", N, t, 2, "rough", "ssprk3", STEPS)
    block = {"block": (16, 16), "march": (64, 8)}.get(family)
    hip, _ = _engine("tc5", N, t, 2, "rough", backend="hip", dtype=torch.float32, block=block, dt=ref.dt,
                     rounded=True)
    if family == "march3":
        from stsphere.ops.march3 import March3Step
        March3Step(hip, rows=16).step(STEPS)
        block = (64, 16)
    elif family == "fused":
        from stsphere.ops.fused import FusedKernel
        fk = FusedKernel(hip)
        fk.step(STEPS)
        torch.cuda.synchronize()
        fk.check()
        block = (fk.plan.B,) * 2
    else:
        hip.step(STEPS)
    print(f"ROUGH fp32 twin C{N} t={t}: " + " ".join(f"{x:.2e}" for x in twin))
    _check(ref, hip, q0, block, f"fp32 {family} rough limiter 2 C{N} t={t}", bound=[4.0 * x for x in twin])
