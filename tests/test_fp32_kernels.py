"""The float instantiation of every stepping kernel (GPU) on the increment
metric: the block stage kernel in all shapes and for every physics, the
streaming stage, the pipelined streaming step, the fused step, the tracer
stage kernel and the remote-ghost path, each limiter and state class, against
the fp64 PyTorch oracle started from the fp32-rounded state.

The fp32 state tests (``< 1e-4`` on the carried state of a smooth run) cannot
see a relative error of 1e-4 in g, let alone a wrong limiter arm; the
increment metric with the bound used here sees both
(tests/test_fp32_states.py).  The bound is ``max(4 x twin, 4 eps32)`` per
field, the twin being the PyTorch backend run in fp32 from the same state
(``fp32_twin_bound`` of tests/rough_states.py and tests/tracer_states.py): the
reference measured against the reference, nothing taken from the kernels.

Unless stated otherwise a case runs two SSP-RK3 steps with the oracle's dt.
Every case prints its measured error, its bound and the ratio of the kernel's
error to the twin's; profiles/fp32/README.md records them."""
import pytest
import torch

import tracer_states
from rough_states import (engine_of, fp32_twin_bound, global_of, global_state, grid_of, increment_error, install,
                          physics_of)
from stsphere.engine import VirtualCluster
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

STEPS = 2
F32 = torch.float32


def _fmt(xs):
    return " ".join(f"{x:.2e}" for x in xs)


def _check(r, hip, block, what):
    """``r``: the case's ``Fp32Reference``.  Prints, then asserts the bound
    (the failure names the worst cell)."""
    torch.cuda.synchronize()
    errs = increment_error(r.ref, hip, r.q0, block=block, what=what)      # raises on a NaN
    print(f"FP32 {what}: err {_fmt(errs)} | bound {_fmt(r.bound)} | err / twin "
          + " ".join(f"{e / max(x, 1e-300):.2f}" for e, x in zip(errs, r.twin)))
    increment_error(r.ref, hip, r.q0, bound=r.bound, block=block, what=what)
    return errs


def _hip(r, kind, N, t, lim, cls, block=None, integ="ssprk3"):
    """The fp32 HIP engine of a case, from the rounded state the reference
    started from, with the oracle's dt."""
    hip, q0 = engine_of(kind, N, t, lim, cls, backend="hip", dtype=F32, integ=integ, block=block, dt=r.ref.dt,
                        rounded=True)
    assert hip.pool[0].dtype == F32 and torch.equal(q0, r.q0)
    if block is not None:
        assert (hip.compute.bx, hip.compute.by) == block and hip.compute.march == (block[0] == 64)
    return hip


def _block_case(kind, N, t, lim, cls, block, integ="ssprk3", steps=STEPS):
    r = fp32_twin_bound(kind, N, t, lim, cls, integ, steps)
    hip = _hip(r, kind, N, t, lim, cls, block, integ)
    hip.step(steps)
    _check(r, hip, block, f"{kind} {cls} limiter {lim} C{N} t={t} block {block[0]}x{block[1]} {integ}")


# ---- block stage kernel, shallow water ------------------------------------------------------
@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("block", [(16, 16), (16, 8)], ids=["16x16", "16x8"])
def test_block_kernel_limiters(block, lim):
    """16x8 is the block fp32 runs in production."""
    _block_case("tc5", 24, 2, lim, "rough", block)


@pytest.mark.parametrize("block", [(8, 16), (32, 8), (8, 8)], ids=["8x16", "32x8", "8x8"])
def test_block_kernel_shapes(block):
    """Tile corners with carried ghosts."""
    _block_case("tc5", 24, 2, 2, "rough", block)


@pytest.mark.parametrize("N,lim,block", [(20, 2, (16, 16)), (17, 3, (16, 8))], ids=["C20-16x16", "C17-16x8"])
def test_block_kernel_partial_blocks(N, lim, block):
    """C20: partial blocks, block-wide fix-up; C17: the last block one cell wide."""
    _block_case("tc5", N, 1, lim, "rough", block)


@pytest.mark.parametrize("N,block", [(25, (8, 8)), (33, (16, 16))], ids=["C25-8x8", "C33-16x16"])
def test_block_kernel_block_ends_one_cell_from_the_panel_edge(N, block):
    _block_case("tc5", N, 1, 2, "rough", block)


@pytest.mark.parametrize("N,t,block", [(24, 2, (16, 16)), (24, 2, (16, 8)), (34, 1, (16, 16))],
                         ids=["C24-16x16", "C24-16x8", "C34-16x16"])
def test_block_kernel_ppm(N, t, block):
    """C34: the third window layer decides."""
    _block_case("tc5", N, t, 4, "rough", block)


@pytest.mark.parametrize("cls", ["plateau", "zero_mom"])
@pytest.mark.parametrize("lim", [1, 3, 4])
def test_block_kernel_exact_zero_differences(lim, cls):
    _block_case("tc5", 24, 2, lim, cls, (16, 8))


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_block_kernel_integrators(integ):
    """One step; rk4 reads and writes the fp32 accumulator rows."""
    _block_case("tc5", 16, 1, 2, "rough", (16, 16), integ=integ, steps=1)


# ---- block stage kernel, other physics ------------------------------------------------------
# PPM is not built for 8x8 blocks
@pytest.mark.parametrize("N,t,block,kind,lim", [
    (N, t, b, kind, lim) for N, t, b in ((24, 2, (16, 16)), (20, 1, (8, 8)))
    for kind, lim in (("adv", 1), ("adv", 2), ("adv", 3), ("adv", 4), ("diff", 0)) if (lim, b) != (4, (8, 8))])
def test_block_kernel_scalar_class(N, t, block, kind, lim):
    _block_case(kind, N, t, lim, "scalar", block)


def test_block_kernel_topography_van_leer():
    """tests/test_topography_kernels.py::test_fp32 runs limiter 2 only."""
    _block_case("topo", 24, 2, 3, "rough", (16, 8))


# ---- streaming stage (64, R) -------------------------------------------------------------------
@pytest.mark.parametrize("N,t,R,lim", [(24, 1, 4, 0), (24, 1, 4, 1), (24, 1, 4, 3), (50, 2, 4, 2), (72, 1, 16, 2)],
                         ids=["C24-R4-lim0", "C24-R4-lim1", "C24-R4-lim3", "C50-t2-R4", "C72-R16"])
def test_march(monkeypatch, N, t, R, lim):
    """Four rows per wave is what fp32 runs at C720; C72: two strips with a
    partial last one.  The geometry path is the fp32 default (cell records)."""
    monkeypatch.delenv("STSP_MARCH_COMPACT", raising=False)
    r = fp32_twin_bound("tc5", N, t, lim, "rough", "ssprk3", STEPS)
    hip = _hip(r, "tc5", N, t, lim, "rough", (64, R))
    assert hip.compute.march_geometry == "records"
    hip.step(STEPS)
    _check(r, hip, (64, R), f"march rough limiter {lim} C{N} t={t} rows {R}")


# ---- pipelined streaming step ----------------------------------------------------------------
@pytest.mark.parametrize("lim", [1, 3])
def test_march3(lim):
    from stsphere.ops.march3 import March3Step
    r = fp32_twin_bound("tc5", 48, 1, lim, "rough", "ssprk3", STEPS)
    hip = _hip(r, "tc5", 48, 1, lim, "rough")
    March3Step(hip, rows=16).step(STEPS)
    _check(r, hip, (64, 16), f"march3 rough limiter {lim} C48 t=1 rows 16")


# ---- fused step, single-step launches ------------------------------------------------------------
@pytest.mark.parametrize("N,t,B,lim", [(12, 1, 6, 2), (16, 1, 8, 2), (24, 2, 12, 2), (32, 2, 16, 2), (36, 2, 18, 2),
                                       (32, 2, 16, 1), (32, 2, 16, 3)])
def test_fused(N, t, B, lim):
    """One launch per step, every block size.  Multi-step launches equal
    single steps bit for bit in fp32 (tests/test_fused.py,
    tests/test_fused_handoff_rt.py)."""
    from stsphere.ops.fused import FusedKernel
    r = fp32_twin_bound("tc5", N, t, lim, "rough", "ssprk3", STEPS)
    hip = _hip(r, "tc5", N, t, lim, "rough")
    fk = FusedKernel(hip, B=B)
    assert fk.plan.B == B
    for _ in range(STEPS):
        fk.step(1)
    torch.cuda.synchronize()
    fk.check()
    _check(r, hip, (B, B), f"fused rough limiter {lim} C{N} t={t} B={B}")


# ---- tracer stage kernel -----------------------------------------------------------------------------
def _tracer_case(nq, N, t, lim, block):
    r = tracer_states.fp32_twin_bound(nq, N, t, lim, "rough", "ssprk3", 1)
    hip, q0 = tracer_states.engine_of(nq, N, t, lim, "rough", backend="hip", dtype=F32, block=block, dt=r.ref.dt,
                                      rounded=True)
    assert hip.compute.phys_id == 3 and (hip.compute.bx, hip.compute.by) == block and torch.equal(q0, r.q0)
    hip.step(1)
    _check(r, hip, block, f"tracers nq {nq} rough limiter {lim} C{N} t={t} block {block[0]}x{block[1]}")


@pytest.mark.parametrize("block", [(16, 16), (16, 8)], ids=["16x16", "16x8"])
@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("nq", [1, 2, 4])
def test_tracer_kernel(nq, lim, block):
    """Rough state and rough mixing ratios, one step (as
    tests/test_tracers_gpu.py::test_rough_start in fp64)."""
    _tracer_case(nq, 16, 2, lim, block)


def test_tracer_kernel_one_cell_wide_last_block():
    _tracer_case(2, 17, 1, 2, (16, 8))


# ---- remote-ghost path ---------------------------------------------------------------------------------
def _global_increment_errors(ref, G, G0):
    """``increment_error`` on global fields [F, 6, N, N] (the interior cells of
    all tiles are the global field)."""
    a = global_of(ref)
    F = a.shape[0]
    da, db = (a - G0).reshape(F, -1), (G - G0).reshape(F, -1)
    return ((db - da).abs().amax(1) / da.abs().amax(1)).tolist()


@pytest.mark.parametrize("ranks", [2, 8])
@pytest.mark.parametrize("what", ["mc", "ppm", "tracers"])
def test_remote_ghosts(what, ranks):
    """Virtual ranks (receive-buffer gather, interior / boundary block lists)
    on C24 t=2: the ranks' state against the oracle with the bound of the
    one-rank case, and the one-rank engine likewise.  The difference between
    the two is printed, not bounded."""
    N, t = 24, 2
    if what == "tracers":
        r = tracer_states.fp32_twin_bound(2, N, t, 2, "rough", "ssprk3", STEPS)
        G0, ng, block = tracer_states.global_state(2, N, "rough").float().double(), 2, (16, 8)
        make = lambda: tracer_states.tracer_physics(2, 2)   # noqa: E731
        single, _ = tracer_states.engine_of(2, N, t, 2, "rough", backend="hip", dtype=F32, block=block, dt=r.ref.dt,
                                            rounded=True)
    else:
        lim, block = (2, (16, 8)) if what == "mc" else (4, (16, 16))
        r = fp32_twin_bound("tc5", N, t, lim, "rough", "ssprk3", STEPS)
        G0 = global_state("tc5", N, "rough").float().double()
        make = lambda: physics_of("tc5", lim)   # noqa: E731
        ng = make().halo
        single = _hip(r, "tc5", N, t, lim, "rough", block)
    vc = VirtualCluster(make, TileLayout(N, t, ranks, ng=ng), grid=grid_of(N), device="cuda", backend="hip", dtype=F32,
                        block=block, dt=r.ref.dt)
    for e in vc.engines:
        assert e.compute.remote and (e.compute.bx, e.compute.by) == block and e.pool[0].dtype == F32
        install(e, G0)
    single.step(STEPS)
    vc.step(STEPS)
    torch.cuda.synchronize()
    name = f"remote ghosts {what} {ranks} ranks C{N} t={t} block {block[0]}x{block[1]}"
    _check(r, single, block, name + ", the one-rank engine")
    a, b = global_of(single), global_of(vc.engines)
    assert torch.isfinite(b).all()
    errs = _global_increment_errors(r.ref, b, G0)
    diff = max(float((a[f] - b[f]).abs().max() / a[f].abs().max()) for f in range(a.shape[0]))
    print(f"FP32 {name}: err {_fmt(errs)} | bound {_fmt(r.bound)} | err / twin "
          + " ".join(f"{e / x:.2f}" for e, x in zip(errs, r.twin))
          + f" | ranks against one rank {diff:.2e} of the field maximum, bitwise {bool(torch.equal(a, b))}")
    for f, (e, bd) in enumerate(zip(errs, r.bound)):
        assert e <= bd, (name, f, errs, r.bound)
