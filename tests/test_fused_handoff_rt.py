"""The fused step's in-launch hand-off where its cell-to-thread mapping and its
waits change with the block size (ops/csrc/fused_step.hip: tail cells on the
threads that own a block cell, fused_wait, ring-first polls).

Every case runs one multi-step launch (plus a trailing single step for an odd
count) and compares it bitwise with the same number of single-step launches,
which never wait inside the kernel; fp64 cases also against the stage-by-stage
PyTorch oracle at the 1e-11 of test_fused.py.  Each under both in-launch
hand-offs (tagged granules, epoch counters).

Shapes: B = 16 has 16 tail cells (784 window cells, 768 threads), N = 32, t = 2
is the smallest grid with them (24 blocks, all on cube corners), N = 48, t = 1
adds an interior block per panel; B = 18 has 132 tail cells, one per carrying
thread (two before); B = 6 and 8 have none and take the other side of the
ring-first choice.  The loopback layout brings tail cells from the xGMI ring.
"""
import pytest
import torch

from stsphere.engine import Engine
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32

# (N, t, B, steps, dtype)
CASES = [
    pytest.param(32, 2, 16, 7, F64, id="C32-t2-B16-fp64"),
    pytest.param(32, 2, 16, 7, F32, id="C32-t2-B16-fp32"),
    pytest.param(48, 1, 16, 5, F64, id="C48-t1-B16-fp64"),
    pytest.param(36, 2, 18, 4, F64, id="C36-t2-B18-fp64"),
    pytest.param(12, 1, 6, 5, F64, id="C12-t1-B6-fp64"),
    pytest.param(16, 1, 8, 5, F64, id="C16-t1-B8-fp64"),
]

_singles = {}     # (N, t, B, steps, dtype) -> (tiles, pool[0], dt) after `steps` single-step launches
_oracle = {}      # (N, t, steps) -> tiles of the PyTorch oracle


def _engine(N, t, dtype, backend="hip", dt=None, loopback=False):
    L = TileLayout(N, t, 1, ng=2, loopback=loopback)
    return Engine(ShallowWater("tc5", limiter=2), L, grid=CubedSphereGrid(N), dtype=dtype if backend == "hip" else F64,
                  device="cuda", backend=backend, dt=dt)


def _oracle_tiles(N, t, steps):
    key = (N, t, steps)
    if key not in _oracle:
        ref = _engine(N, t, F64, backend="torch")
        ref.step(steps)
        torch.cuda.synchronize()
        _oracle[key] = (ref.tiles_view().clone(), ref.dt)
    return _oracle[key]


def _single_steps(N, t, B, steps, dtype):
    from stsphere.ops.fused import FusedKernel
    key = (N, t, B, steps, dtype)
    if key not in _singles:
        dt = _oracle_tiles(N, t, steps)[1]
        a = _engine(N, t, dtype, dt=dt)
        fk = FusedKernel(a, B=B)
        assert fk.plan.B == B
        fk.step(steps)
        torch.cuda.synchronize()
        _singles[key] = (a.tiles_view().clone(), a.pool[0].clone(), dt)
    return _singles[key]


def _relerr(a, b):
    a, b = a.reshape(4, -1).double(), b.reshape(4, -1).double()
    return ((a - b).abs().amax(1) / a.abs().amax(1)).max().item()


def _multi_then_single(fk, steps):
    """`steps` steps as one even multi-step launch and, for an odd count, one
    single-step launch after it; the state ends in the engine's pool[0]."""
    fk.launch(0, nsteps=steps - steps % 2)
    if steps % 2:
        fk.step(1)
    torch.cuda.synchronize()
    fk.check()


@pytest.mark.parametrize("handoff", ["tag", "epoch"])
@pytest.mark.parametrize("N,t,B,steps,dtype", CASES)
def test_multi_step_launch_equals_single_steps(monkeypatch, N, t, B, steps, dtype, handoff):
    from stsphere.ops.fused import FusedKernel
    monkeypatch.setenv("STSP_FUSED_HANDOFF", handoff)
    monkeypatch.delenv("STSP_FUSED_POLL", raising=False)
    tiles, pool0, dt = _single_steps(N, t, B, steps, dtype)
    b = _engine(N, t, dtype, dt=dt)
    fk = FusedKernel(b, B=B)
    assert fk.handoff == handoff and fk.plan.B == B
    _multi_then_single(fk, steps)
    assert torch.equal(tiles, b.tiles_view())
    assert torch.equal(pool0, b.pool[0])          # the ghost slots pushed after the last step too
    if dtype == F64:
        err = _relerr(_oracle_tiles(N, t, steps)[0], b.tiles_view())
        print(f"C{N} t={t} B={B} {handoff}: max rel diff vs oracle after {steps} steps {err:.3e}")
        assert err < 1e-11


@pytest.mark.parametrize("handoff", ["tag", "epoch"])
def test_loopback_tail_cells_equal_one_rank(monkeypatch, handoff):
    """N = 32, t = 2, B = 16 with every other tile's window cells through the
    rank's own xGMI ring (tail cells among them): bitwise equal to one rank."""
    from stsphere.ops.fused import FusedKernel
    monkeypatch.setenv("STSP_FUSED_HANDOFF", handoff)
    monkeypatch.delenv("STSP_FUSED_POLL", raising=False)
    N, t, B, steps = 32, 2, 16, 7
    tiles, _, dt = _single_steps(N, t, B, steps, F64)
    b = _engine(N, t, F64, dt=dt, loopback=True)
    fk = FusedKernel(b, B=B)
    try:
        assert fk.mem is not None and fk.handoff == handoff
        assert (fk.plan.src <= -2).any()
        _multi_then_single(fk, steps)
        assert torch.equal(tiles, b.tiles_view())
        err = _relerr(_oracle_tiles(N, t, steps)[0], b.tiles_view())
        print(f"C{N} loopback {handoff}: max rel diff vs oracle after {steps} steps {err:.3e}")
        assert err < 1e-11
    finally:
        fk.close()
