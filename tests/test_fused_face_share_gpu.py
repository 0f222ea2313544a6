"""The fused step's shared face passes (each cell's limited slope computed once
per face line and handed to the neighbouring lane) against the same binary with
STSP_FUSED_SHARE=0 (every face computes both slopes, the order of
stage_face_coords): bit for bit, from rough states that take every limiter
branch, on interior, panel-edge and cube-corner blocks."""
import pytest
import torch

from rough_states import global_state, grid_of, install
from stsphere.engine import Engine
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32


def _kernel(monkeypatch, share, N, t, B, dtype, lim, loopback=False, dt=None):
    from stsphere.ops.fused import FusedKernel
    monkeypatch.setenv("STSP_FUSED_SHARE", "1" if share else "0")
    e = Engine(ShallowWater("tc5", limiter=lim), TileLayout(N, t, 1, ng=2, loopback=loopback), grid=grid_of(N),
               dtype=dtype, device="cuda", backend="hip", dt=dt)
    install(e, global_state("tc5", N, "rough"))
    fk = FusedKernel(e, B=B)
    assert fk.plan.B == B and fk.pfn
    return e, fk


def _run(e, fk):
    for _ in range(3):
        fk.step(1)
    fk.launch(0, nsteps=4)
    torch.cuda.synchronize()
    fk.check()
    assert torch.isfinite(e.pool[0]).all()


@pytest.mark.parametrize("N,t,B,dtype,lim,loopback", [
    pytest.param(24, 1, 6, F64, 2, False, id="C24-B6-fp64"),
    pytest.param(24, 1, 8, F64, 2, False, id="C24-B8-fp64"),
    pytest.param(48, 1, 16, F64, 2, False, id="C48-B16-fp64"),
    pytest.param(48, 1, 16, F32, 2, False, id="C48-B16-fp32"),
    pytest.param(24, 1, 8, F64, 1, False, id="C24-B8-fp64-lim1"),
    pytest.param(24, 1, 8, F64, 3, False, id="C24-B8-fp64-lim3"),
    pytest.param(24, 2, 6, F64, 2, True, id="C24-t2-B6-fp64-loopback"),
])
def test_shared_faces_equal_full_faces(monkeypatch, N, t, B, dtype, lim, loopback):
    a, fa = _kernel(monkeypatch, True, N, t, B, dtype, lim, loopback)
    b, fb = _kernel(monkeypatch, False, N, t, B, dtype, lim, loopback, dt=a.dt)
    try:
        assert (fa.tens["sched"][:, :, 17] != 0).any() and not (fb.tens["sched"][:, :, 17] != 0).any()
        assert (fa.mem is not None) == loopback
        q0 = a.pool[0].clone()
        _run(a, fa)
        _run(b, fb)
        assert not torch.equal(q0, a.pool[0])
        assert torch.equal(a.pool[0], b.pool[0])          # the full state, ghost slots too
        assert torch.equal(a.tiles_view(), b.tiles_view())
    finally:
        fa.close()
        fb.close()
