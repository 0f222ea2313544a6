"""The gfx950 derived-field kernel (ops/csrc/derived_kernel.hip) against its
PyTorch twin (models/derived.py), and its plumbing through the solver."""
import functools

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine, assemble_global
from stsphere.models import derived as md
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout
from stsphere.utils.history import read_history

pytestmark = pytest.mark.gpu

# (N, tiles per edge): a ragged single block; tile edges inside panels with carried
# corner ghosts as interpolation sources; an interior tile with no panel edge;
# 3 x 3 blocks with an 8-wide remainder
SHAPES = [(12, 1), (24, 2), (36, 3), (40, 1)]
CASES = ["tc5", "tc6"]
EPS32 = float(np.finfo(np.float32).eps)


@functools.lru_cache(maxsize=None)
def _state(N, t, case):
    """CPU fp64 engine two steps into the case (the shared reference state)."""
    e = Engine(ShallowWater(case), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N))
    e.step(2)
    return e


@functools.lru_cache(maxsize=None)
def _twin(N, t, case, rounded=False):
    """(fields, inv) of the fp64 twin on the reference state (``rounded``: on
    the state rounded to fp32)."""
    e = _state(N, t, case)
    if not rounded:
        f, inv = e.derived()
        return f.clone(), inv.clone()
    e2 = Engine(ShallowWater(case), e.layout, grid=e.grid, dt=e.dt)
    e2.set_state(e.tiles_view().float().double())
    f, inv = e2.derived()
    return f.clone(), inv.clone()


def _engine(N, t, case, dtype, device, backend):
    ref = _state(N, t, case)
    e = Engine(ShallowWater(case), ref.layout, grid=ref.grid, dtype=dtype, device=device, backend=backend, dt=ref.dt)
    e.set_state(ref.tiles_view().to(dtype))
    return e


def _field_diff(f, ref):
    """max |f - ref| / max |ref| per field."""
    f, ref = f.double().cpu(), ref.double().cpu()
    return [float((f[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in range(3)]


def _inv_diff(inv, ref):
    """Relative differences of the invariants; circulation over abs_circulation."""
    a, b = dict(zip(md.INVARIANTS, inv.cpu().tolist())), dict(zip(md.INVARIANTS, ref.cpu().tolist()))
    out = {k: abs(a[k] - b[k]) / abs(b[k]) for k in md.INVARIANTS if k != "circulation"}
    out["circulation"] = abs(a["circulation"] - b["circulation"]) / b["abs_circulation"]
    return out


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_twin_fp64(N, t, case):
    """Per field max |kernel - twin| <= 1e-12 max |twin|; positive sums within
    1e-12 relative, circulation within 1e-12 abs_circulation, max_courant within
    1e-14 relative.  Measured on an MI355X: see profiles/derived/README.md."""
    fr, ir = _twin(N, t, case)
    e = _engine(N, t, case, torch.float64, "cuda:0", "hip")
    f, inv = e.derived()
    torch.cuda.synchronize()
    fd, idf = _field_diff(f, fr), _inv_diff(inv, ir)
    print(f"fp64 C{N} t={t} {case}: fields {fd} inv {idf}")
    assert torch.isfinite(f).all() and float(inv[6]) == 0.0 and float(inv[7]) == 0.0
    for k in range(3):
        assert fd[k] <= 1e-12, (md.FIELDS[k], fd[k])
    for k in ("mass", "energy", "potential_enstrophy", "abs_circulation", "circulation"):
        assert idf[k] <= 1e-12, (k, idf[k])
    assert idf["max_courant"] <= 1e-14


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_twin_fp32(N, t, case):
    """No tolerance is fixed in advance: the twin run in fp32 is measured
    against the twin run in fp64 on the same fp32-rounded state (on the CPU,
    per field and shape), and the kernel gets 4x that against the fp64 twin,
    since its operation order differs (floor: 4 fp32 eps).

    Measured twin fp32 vs fp64, max |diff| / max |field| (vorticity,
    divergence, pv), tc5 / tc6:
      C12 t=1  (8.8e-7, 1.6e-6, 1.3e-7) / (3.9e-7, 5.4e-6, 1.5e-7)
      C24 t=2  (1.9e-6, 2.6e-6, 1.7e-7) / (9.1e-7, 4.1e-5, 3.4e-7)
      C36 t=3  (3.8e-6, 5.8e-6, 1.7e-7) / (1.0e-6, 1.4e-4, 4.0e-7)
      C40 t=1  (3.4e-6, 5.8e-6, 2.2e-7) / (1.2e-6, 1.3e-4, 4.6e-7)
    (the four circulation terms cancel by a factor that grows with N, and the
    divergence of the nearly non-divergent TC6 flow is itself a small
    remainder); invariants at most 9.8e-8 relative (potential enstrophy), the
    sums of mass and energy 4e-10 to 3e-9."""
    fr, ir = _twin(N, t, case, rounded=True)
    cpu = _engine(N, t, case, torch.float32, "cpu", "torch")
    fc, ic = cpu.derived()
    ftol = [max(4.0 * d, 4.0 * EPS32) for d in _field_diff(fc, fr)]
    itol = {k: max(4.0 * d, 4.0 * EPS32) for k, d in _inv_diff(ic, ir).items()}
    e = _engine(N, t, case, torch.float32, "cuda:0", "hip")
    f, inv = e.derived()
    torch.cuda.synchronize()
    fd, idf = _field_diff(f, fr), _inv_diff(inv, ir)
    print(f"fp32 C{N} t={t} {case}: fields {fd} (tol {ftol}) inv {idf} (tol {itol})")
    assert f.dtype == torch.float32 and inv.dtype == torch.float64 and torch.isfinite(f).all()
    for k in range(3):
        assert fd[k] <= ftol[k], (md.FIELDS[k], fd[k], ftol[k])
    for k in md.INVARIANTS:
        assert idf[k] <= itol[k], (k, idf[k], itol[k])


def _global(e, f):
    f = f.double().cpu().numpy()
    return np.stack([assemble_global(e.layout, {0: f[k]}) for k in range(3)])


def test_reproducible_and_decomposition_independent():
    e1 = _engine(24, 1, "tc5", torch.float64, "cuda:0", "hip")
    e2 = _engine(24, 2, "tc5", torch.float64, "cuda:0", "hip")
    e2.set_state(torch.as_tensor(np.stack([e2.geo.gather_global(assemble_global(e1.layout, {0: v}))
                                           for v in e1.tiles_view().cpu().numpy()])))
    f, inv = e2.derived()
    fa, ia = f.clone(), inv.clone()
    f, inv = e2.derived()
    assert torch.equal(fa, f) and torch.equal(ia, inv)
    f1, _ = e1.derived()
    assert np.array_equal(_global(e1, f1), _global(e2, fa))


def _gpu_cfg(out, **io):
    return {"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": "gpu"},
            "grid": {"N": 24}, "physics": {"model": "swe", "case": "tc5"}, "time": {"nsteps": 12},
            "runtime": {"fused": "on"}, "io": dict({"output_dir": str(out)}, **io)}


def _twin_of_global(state, dt):
    """Twin fields [3, 6, N, N] of a global state [4, 6, N, N] (one tile per panel)."""
    N = state.shape[-1]
    e = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), dt=dt)
    e.set_state(torch.as_tensor(state))
    return _global(e, e.derived()[0])


def test_after_fused_stepping(tmp_path):
    """The ghost slots of the padded state are not current after a fused
    launch: the kernel must pull its ring through the ghost map."""
    s = S.Solver(_gpu_cfg(tmp_path), verbose=False)
    s.initialize()
    s.step(5)
    assert s.fused is not None
    ref = _twin_of_global(s.gather_global(), s.dt)
    for k, name in enumerate(md.FIELDS):
        got = s.derived_field(name)
        assert np.abs(got - ref[k]).max() <= 1e-12 * np.abs(ref[k]).max(), name
    s.close()


def test_history_on_the_stepping_stream(tmp_path):
    """Every frame's pv equals the twin on that frame's prognostic state
    (recorded by a second run with the four prognostic fields)."""
    a = S.Solver(_gpu_cfg(tmp_path / "a", history_interval=4, history_fields=["h", "pv"]), verbose=False)
    a.run()
    a.close()
    b = S.Solver(_gpu_cfg(tmp_path / "b", history_interval=4), verbose=False)
    b.run()
    b.close()
    ha, hb = str(tmp_path / "a" / "history.zarr"), str(tmp_path / "b" / "history.zarr")
    pv, h = read_history(ha, "pv"), read_history(ha, "h")
    prog = np.stack([read_history(hb, f) for f in ("h", "mx", "my", "mz")], 1)      # [frames, 4, 6, N, N]
    assert pv.shape == (4, 6, 24, 24) and np.array_equal(h, prog[:, 0])
    for k in range(4):
        ref = _twin_of_global(prog[k], a.dt)[2]
        assert np.abs(pv[k] - ref).max() <= 1e-12 * np.abs(ref).max(), k
