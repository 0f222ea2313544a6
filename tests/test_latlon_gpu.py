"""The gfx950 lat-lon kernel (ops/csrc/latlon_kernel.hip) against its PyTorch
twin (models/latlon.py), and its plumbing through the solver."""
import functools
import math

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine
from stsphere.models import latlon as ml
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout
from stsphere.utils import zarr_lite
from stsphere.utils.history import read_history

pytestmark = pytest.mark.gpu

# the derived tests' shapes: (N, tiles per edge)
SHAPES = [(12, 1), (24, 2), (36, 3), (40, 1)]
CASES = ["tc5", "tc6"]
EPS = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)
PROG = ("h", "mx", "my", "mz")
DER = ("vorticity", "divergence", "pv")
WIND = ("u", "v")
# 684 points: a ragged last workgroup, nlon < 64; nlon = 100: a full wave and a
# partial one in the row sum; nlon = 300 > 256: a second pass of the row loop; the
# rows lat = -pi/2, +pi/2 and the column lon = 0 (nlon = 70)
GRIDS = {"19x36": lambda: ml.default_grid(19, 36), "7x100": lambda: ml.default_grid(7, 100),
         "5x300": lambda: ml.default_grid(5, 300),
         "poles": lambda: (np.linspace(-0.5 * math.pi, 0.5 * math.pi, 9),
                           np.linspace(0.0, 2.0 * math.pi, 70, endpoint=False))}


@functools.lru_cache(maxsize=None)
def _state(N, t, case):
    """CPU fp64 engine two steps into the case (the shared reference state)."""
    e = Engine(ShallowWater(case), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N))
    e.step(2)
    return e


def _engine(N, t, case, dtype, device, backend, rounded=False):
    ref = _state(N, t, case)
    e = Engine(ShallowWater(case), ref.layout, grid=ref.grid, dtype=dtype, device=device, backend=backend, dt=ref.dt)
    v = ref.tiles_view()
    e.set_state((v.float().double() if rounded else v).to(dtype))
    return e


def _outputs(e, grid, der=None):
    """{name: (array [nlat, nlon], zonal mean [nlat])} of every channel of an
    engine, as float64 CPU tensors; ``der``: the unpadded [3, T, n, n] input of the
    derived channels (default: the engine's own derived fields)."""
    ll = e.latlon(*GRIDS[grid]())
    der = e.derived()[0] if der is None else der.to(device=e.device, dtype=e.dtype)
    out = {}
    for names, (a, z) in ((PROG, ll.fields()), (DER, ll.tiles(der)), (WIND, ll.winds())):
        assert z.dtype == torch.float64 and a.dtype == e.dtype and a.shape == (len(names), ll.nlat, ll.nlon)
        for k, n in enumerate(names):
            out[n] = (a[k].double().cpu(), z[k].cpu())
    if e.device.type == "cuda":
        torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def _twin(N, t, case, grid):
    return _outputs(_state(N, t, case), grid)


def _diffs(got, ref):
    """{name: (field diff, zonal-mean diff)} over max |ref field|."""
    return {n: (float((got[n][0] - ref[n][0]).abs().max() / ref[n][0].abs().max()),
                float((got[n][1] - ref[n][1]).abs().max() / ref[n][0].abs().max())) for n in ref}


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_twin_fp64(N, t, case):
    """Per channel max |kernel - twin| <= 1e-12 max |twin|, the project's fp64
    bound: prognostic fields from the padded layout, the derived fields from the
    unpadded one, u, v, and the zonal mean of each.  Measured on an MI355X: see
    profiles/latlon/README.md."""
    e = _engine(N, t, case, torch.float64, "cuda:0", "hip")
    assert e.latlon(nlat=19, nlon=36).hip
    for grid in GRIDS:
        d = _diffs(_outputs(e, grid), _twin(N, t, case, grid))
        print(f"fp64 C{N} t={t} {case} {grid}: " + " ".join(f"{n} {a:.1e}/{z:.1e}" for n, (a, z) in d.items()))
        for n, (a, z) in d.items():
            assert a <= 1e-12 and z <= 1e-12, (grid, n, a, z)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_twin_fp32(N, t, case):
    """No tolerance is fixed in advance: the twin run in fp32 is measured
    against the twin run in fp64 on the same fp32-rounded state (on the CPU, per
    shape, grid and channel), and the kernel gets 4x that against the fp64 twin
    (floor: 4 fp32 eps).  The derived channels regrid one input, the fp32 twin's
    derived fields, in all three runs, so that the figure is the regridding's own.

    Measured twin fp32 vs fp64, max |diff| / max |field| over the shapes, cases
    and the four grids: prognostic 2.0e-08 to 1.6e-07 (zonal means 4.2e-11 to
    3.8e-08), derived 4.7e-08 to 1.6e-07 (3.4e-10 to 5.4e-08), u and v 6.0e-08 to
    6.3e-06 (1.7e-09 to 2.7e-07; each relative to its own maximum, and the
    meridional wind is a small remainder beside u).  On an MI355X the kernel's
    fp32 arrays came out bitwise equal to the fp32 twin's in all 32 cases
    (printed below, not asserted)."""
    c32 = _engine(N, t, case, torch.float32, "cpu", "torch", rounded=True)
    c64 = _engine(N, t, case, torch.float64, "cpu", "torch", rounded=True)
    der = c32.derived()[0]
    e = _engine(N, t, case, torch.float32, "cuda:0", "hip", rounded=True)
    for grid in GRIDS:
        ref = _outputs(c64, grid, der)
        tw, ke = _outputs(c32, grid, der), _outputs(e, grid, der)
        meas, got = _diffs(tw, ref), _diffs(ke, ref)
        print(f"fp32 C{N} t={t} {case} {grid}: arrays bitwise equal to the fp32 twin: "
              f"{all(torch.equal(ke[n][0], tw[n][0]) for n in ref)}")
        print(f"fp32 C{N} t={t} {case} {grid}: " + " ".join(f"{n} {got[n][0]:.1e}/{got[n][1]:.1e} "
                                                             f"(twin {meas[n][0]:.1e}/{meas[n][1]:.1e})" for n in ref))
        for n in ref:
            for k in range(2):
                assert got[n][k] <= max(4.0 * meas[n][k], 4.0 * EPS32), (grid, n, k, got[n][k], meas[n][k])


def test_repeatable():
    e = _engine(24, 2, "tc5", torch.float64, "cuda:0", "hip")
    for grid in GRIDS:
        a, b = _outputs(e, grid), _outputs(e, grid)
        for n in a:
            assert torch.equal(a[n][0], b[n][0]) and torch.equal(a[n][1], b[n][1]), (grid, n)


def test_terms_mode_folds_to_the_direct_result():
    """The several-rank route on one rank (the gather stores the four terms, the
    finish launch folds them) is the direct result bit for bit."""
    e = _engine(36, 3, "tc5", torch.float64, "cuda:0", "hip")
    der = e.derived()[0]
    for grid in GRIDS:
        ll = e.latlon(*GRIDS[grid]())
        pairs = ((ll.fields(), ll.finish(ll.partial_fields(terms=True))),
                 (ll.tiles(der), ll.finish(ll.partial_tiles(der, terms=True))),
                 (ll.winds(), ll.finish(ll.partial_velocity(terms=True), project=True)))
        torch.cuda.synchronize()
        for (a, za), (b, zb) in pairs:
            assert a.shape == b.shape and torch.equal(a, b) and torch.equal(za, zb), grid


def test_ghost_poison_on_the_device():
    """NaN in the whole ghost ring of the padded state: bitwise the same."""
    e = _engine(24, 2, "tc6", torch.float64, "cuda:0", "hip")
    ll = e.latlon(nlat=19, nlon=36)
    before = [x.clone() for x in (*ll.fields(), *ll.winds())]
    keep = e.tiles_view().clone()
    e.state.fill_(float("nan"))
    e.tiles_view().copy_(keep)
    assert int(torch.isnan(e.state).sum()) == 4 * (e.plan.S - e.plan.T * e.plan.n ** 2)
    after = [*ll.fields(), *ll.winds()]
    torch.cuda.synchronize()
    for a, b in zip(before, after):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def _gpu_cfg(out, nd=1, t=2, **io):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "gpu"},
            "grid": {"N": 24}, "physics": {"model": "swe", "case": "tc5"}, "time": {"nsteps": 12},
            "runtime": {"fused": "on" if nd == 1 else "auto"}, "io": dict({"output_dir": str(out)}, **io)}


def _twin_of_global(state, dt, names, nlat=19, nlon=36):
    """{name: (array, zonal mean)} of the CPU twin on a global state [4, 6, N, N]."""
    N = state.shape[-1]
    e = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), dt=dt)
    e.set_state(torch.as_tensor(state))
    ll = e.latlon(nlat=nlat, nlon=nlon)
    out = {}
    for group, (a, z) in ((PROG, ll.fields()), (DER, ll.tiles(e.derived()[0])), (WIND, ll.winds())):
        out.update({n: (a[k].numpy(), z[k].numpy()) for k, n in enumerate(group) if n in names})
    return out


NAMES = ("h", "mx", "vorticity", "pv", "u", "v")


def test_after_fused_stepping(tmp_path):
    """The ghost slots of the padded state are not current after a fused
    multi-step launch: the regridding reads none."""
    s = S.Solver(_gpu_cfg(tmp_path), verbose=False)
    s.initialize()
    s.step(6)
    assert s.fused is not None
    ref = _twin_of_global(s.gather_global(), s.dt, NAMES)
    for n in NAMES:
        a, z = s.latlon_field(n, 19, 36), s.zonal_mean(n, 19, 36)
        scale = np.abs(ref[n][0]).max()
        assert np.abs(a - ref[n][0]).max() <= 1e-12 * scale and np.abs(z - ref[n][1]).max() <= 1e-12 * scale, n
    s.close()


@pytest.mark.parametrize("nd", [2, 6])
def test_virtual_ranks_on_one_gpu(tmp_path, nd):
    """Two and six virtual ranks (term arrays added on the device in rank
    order) equal one rank within 8 eps max|field|; the channels that read the
    state alone bit for bit."""
    one = S.Solver(_gpu_cfg(tmp_path / "one", t=1), verbose=False)
    one.initialize()
    one.step(2)
    state = one.gather_global()
    many = S.Solver(_gpu_cfg(tmp_path / "many", nd=nd, t=1), verbose=False)
    many.initialize()
    assert many.mode == "virtual" and len(many.engines) == nd
    for e in many.engines:
        e.set_state(torch.as_tensor(np.stack([e.geo.gather_global(v) for v in state])))
    for n in NAMES:
        ra, rz = one.latlon_field(n, 19, 36), one.zonal_mean(n, 19, 36)
        a, z = many.latlon_field(n, 19, 36), many.zonal_mean(n, 19, 36)
        scale = np.abs(ra).max()
        assert np.abs(a - ra).max() <= 8 * EPS * scale and np.abs(z - rz).max() <= 8 * EPS * scale, n
        if n not in DER:
            assert np.array_equal(a, ra) and np.array_equal(z, rz), n
    one.close()
    many.close()


def test_history_on_the_stepping_stream(tmp_path):
    """The frames of history_latlon.zarr: the last one is ``latlon_field`` at
    the end of the run bit for bit, every one equals the twin on that frame's
    prognostic state (the cube history of the same run) within the fp64 bound."""
    a = S.Solver(_gpu_cfg(tmp_path / "a", history_interval=4, latlon=[19, 36]), verbose=False)
    a.run()
    hl, hc = str(tmp_path / "a" / "history_latlon.zarr"), str(tmp_path / "a" / "history.zarr")
    assert sorted(zarr_lite.list_arrays(hl)) == sorted(PROG + WIND + ("lat", "lon", "time", "step"))
    assert list(zarr_lite.read_array(hl, "step")) == [0, 4, 8, 12]
    frames = {n: zarr_lite.read_array(hl, n) for n in PROG + WIND}
    for n in PROG + WIND:
        assert frames[n].shape == (4, 19, 36) and np.array_equal(frames[n][-1], a.latlon_field(n, 19, 36)), n
    a.close()
    prog = np.stack([read_history(hc, f) for f in PROG], 1)                   # [frames, 4, 6, N, N]
    for k in range(4):
        ref = _twin_of_global(prog[k], a.dt, PROG + WIND)
        for n in PROG + WIND:
            assert np.abs(frames[n][k] - ref[n][0]).max() <= 1e-12 * np.abs(ref[n][0]).max(), (k, n)
