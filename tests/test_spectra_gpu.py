"""The gfx950 spectra kernel (ops/csrc/spectra_kernel.hip) against its PyTorch
twin (models/spectra.py), and its plumbing through the solver."""
import functools

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine
from stsphere.models import spectra as ms
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout
from stsphere.utils import zarr_lite
from stsphere.utils.history import read_history

pytestmark = pytest.mark.gpu

# the derived and lat-lon tests' shapes: (N, tiles per edge).  864 and 7776 cells
# per rank are no multiple of the 128-cell batch (ragged last batch); 3456 and
# 9600 are; all four split into several slabs
SHAPES = [(12, 1), (24, 2), (36, 3), (40, 1)]
CASES = ["tc5", "tc6"]
# 15, 16, 17 straddle a 16-row tile of degrees, 31, 32, 33 the 32-degree group
# (where N allows); 2N - 1 at N = 12 and 24 is the cap.  lmax = 0 has tests of its own
LMAXES = {12: (1, 15, 16, 17, 23), 24: (1, 15, 16, 17, 31, 32, 33, 47), 36: (1, 15, 16, 17, 33),
          40: (1, 15, 16, 17)}
PROG = ("h", "mx", "my", "mz")
DER = ("vorticity", "divergence", "pv")


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


def _coeffs(e, lmax, der):
    """Coefficients [7, 2, L+1, L+1] (float64, on the CPU) of the four
    prognostic channels (padded source) and of ``der`` [3, T, n, n] (unpadded)."""
    sp = e.spectra(lmax)
    a, b = sp.partial_fields(), sp.partial_tiles(der.to(device=e.device, dtype=e.dtype))
    assert a.dtype == torch.float64 and a.shape == (4, 2, lmax + 1, lmax + 1) and b.shape == (3, 2, lmax + 1, lmax + 1)
    return torch.cat([a, b]).cpu()


def _worst(got, ref):
    """Per channel (coefficient diff / max |coefficient|, power diff / max power)."""
    pg, pr = ms.power(got), ms.power(ref)
    return [(float((got[k] - ref[k]).abs().max() / ref[k].abs().max()),
             float((pg[k] - pr[k]).abs().max() / pr[k].max())) for k in range(ref.shape[0])]


def _check(tag, e, twin, der, lmaxes):
    """Every figure is printed before anything is asserted."""
    assert e.spectra(1).hip
    bad = []
    for L in lmaxes:
        got, ref = _coeffs(e, L, der), _coeffs(twin, L, der)
        d = _worst(got, ref)
        print(f"{tag} lmax {L}: " + " ".join(f"{n} {a:.1e}/{p:.1e}" for n, (a, p) in zip(PROG + DER, d)))
        assert bool((torch.triu(got, 1) == 0).all()) and bool((got[:, 1, :, 0] == 0).all())
        bad += [(L, n, a, p) for n, (a, p) in zip(PROG + DER, d) if not (a <= 1e-12 and p <= 1e-12)]
    assert not bad, bad


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_twin_fp64(N, t, case):
    """Per channel max |kernel - twin| <= 1e-12 max |twin|, the project's fp64
    bound, over all coefficients and over the power per degree (scaled by its
    own maximum): the prognostic fields from the padded layout, the derived
    fields from the unpadded one.  Measured on an MI355X: see
    profiles/spectra/README.md."""
    twin = _state(N, t, case)
    der = twin.derived()[0]
    _check(f"fp64 C{N} t={t} {case}", _engine(N, t, case, torch.float64, "cuda:0", "hip"), twin, der, LMAXES[N])


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_twin_fp32(N, t, case):
    """An fp32 state on the device against the fp64 twin on the same
    fp32-rounded values: all arithmetic is double after the load, so the bound
    is the same 1e-12."""
    c32 = _engine(N, t, case, torch.float32, "cpu", "torch", rounded=True)
    c64 = _engine(N, t, case, torch.float64, "cpu", "torch", rounded=True)
    der = c32.derived()[0]
    assert der.dtype == torch.float32
    _check(f"fp32 C{N} t={t} {case}", _engine(N, t, case, torch.float32, "cuda:0", "hip", rounded=True), c64,
           der, LMAXES[N])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_twin_lmax0(N, t, case, dtype):
    """lmax = 0, the same per-channel bound: the one coefficient is the area
    mean, so max |twin| is the mean itself.  For mx, my, mz, the vorticity and pv
    that mean vanishes analytically (the four-fold symmetry of the TC6 wave; no
    net circulation on a closed surface) and a plain sum leaves the rounding
    residue of its own summation order (kernel and twin then differed by 8.8e-13
    to 15 of the twin's value, 3.6e-15 of sum |w f|).  Kernel and twin both sum
    this coefficient error-free, to an ulp of the sum of the products w f, which
    are the same numbers on both sides."""
    rounded = dtype == torch.float32
    twin = _engine(N, t, case, torch.float64, "cpu", "torch", rounded=rounded)
    der = _engine(N, t, case, dtype, "cpu", "torch", rounded=rounded).derived()[0]
    e = _engine(N, t, case, dtype, "cuda:0", "hip", rounded=rounded)
    x = torch.cat([twin.tiles_view().reshape(4, -1), der.double().reshape(3, -1)])
    scale = (twin.spectra(0).tab.cell[:, 3] * x.abs()).sum(1)
    d = (_coeffs(e, 0, der) - _coeffs(twin, 0, der))[:, 0, 0, 0].abs() / scale
    print(f"lmax0 {dtype} C{N} t={t} {case} against sum |w f|: " + " ".join(f"{v:.1e}" for v in d.tolist()))
    _check(f"lmax0 {dtype} C{N} t={t} {case}", e, twin, der, (0,))


def test_repeatable():
    e = _engine(24, 2, "tc5", torch.float64, "cuda:0", "hip")
    der = e.derived()[0].clone()
    for L in (17, 47):
        a, b = _coeffs(e, L, der), _coeffs(e, L, der)
        assert torch.equal(a, b), L


def test_ghost_poison_on_the_device():
    """NaN in the whole ghost ring of the padded state: bitwise the same."""
    e = _engine(24, 2, "tc6", torch.float64, "cuda:0", "hip")
    sp = e.spectra(33)
    before = sp.partial_fields().clone()
    keep = e.tiles_view().clone()
    e.state.fill_(float("nan"))
    e.tiles_view().copy_(keep)
    assert int(torch.isnan(e.state).sum()) == 4 * (e.plan.S - e.plan.T * e.plan.n ** 2)
    after = sp.partial_fields()
    torch.cuda.synchronize()
    assert torch.isfinite(after).all() and torch.equal(before, after)


def _gpu_cfg(out, nd=1, t=2, **io):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "gpu"},
            "grid": {"N": 24}, "physics": {"model": "swe", "case": "tc5"}, "time": {"nsteps": 12},
            "runtime": {"fused": "on" if nd == 1 else "auto"}, "io": dict({"output_dir": str(out)}, **io)}


def _twin_of_global(state, dt, lmax):
    """({name: power [L+1]}, ke [L+1]) of the CPU twin on a global state [4, 6, N, N]."""
    N = state.shape[-1]
    e = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), dt=dt)
    e.set_state(torch.as_tensor(state))
    sp = e.spectra(lmax)
    a, b = sp.partial_fields(), sp.partial_tiles(e.derived()[0])
    out = {n: ms.power(a)[k].numpy() for k, n in enumerate(PROG)}
    out.update({n: ms.power(b)[k].numpy() for k, n in enumerate(DER)})
    return out, ms.ke_spectrum(b[0], b[1], e.grid.radius).numpy()


NAMES = ("h", "mx", "vorticity", "divergence", "pv")
LS = 20


def test_after_fused_stepping(tmp_path):
    """The ghost slots of the padded state are not current after a fused
    multi-step launch: the analysis reads none."""
    s = S.Solver(_gpu_cfg(tmp_path), verbose=False)
    s.initialize()
    s.step(6)
    assert s.fused is not None
    ref, ke = _twin_of_global(s.gather_global(), s.dt, LS)
    for n in NAMES:
        a = s.spectrum(n, LS)
        assert a.shape == (LS + 1,) and np.abs(a - ref[n]).max() <= 1e-12 * ref[n].max(), n
    assert np.abs(s.ke_spectrum(LS) - ke).max() <= 1e-12 * ke.max()
    s.close()


@pytest.mark.parametrize("nd", [2, 6])
def test_virtual_ranks_on_one_gpu(tmp_path, nd):
    """Two and six virtual ranks (partial sums added on the device in rank
    order) equal one rank within 1e-12 of the largest coefficient."""
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
        ra, a = one.sh_coefficients(n, LS), many.sh_coefficients(n, LS)
        assert ra.shape == (2, LS + 1, LS + 1) and np.abs(a - ra).max() <= 1e-12 * np.abs(ra).max(), n
    rk, k = one.ke_spectrum(LS), many.ke_spectrum(LS)
    assert np.abs(k - rk).max() <= 1e-12 * rk.max()
    one.close()
    many.close()


def test_history_on_the_stepping_stream(tmp_path):
    """The frames of history_spectra.zarr: the last one is ``Solver.spectrum``
    at the end of the run bit for bit, every one equals the twin on that frame's
    prognostic state (the cube history of the same run) within the fp64 bound."""
    a = S.Solver(_gpu_cfg(tmp_path / "a", history_interval=4, spectra=LS), verbose=False)
    a.run()
    hs, hc = str(tmp_path / "a" / "history_spectra.zarr"), str(tmp_path / "a" / "history.zarr")
    assert sorted(zarr_lite.list_arrays(hs)) == sorted(PROG + ("ke", "degree", "time", "step"))
    assert list(zarr_lite.read_array(hs, "step")) == [0, 4, 8, 12]
    frames = {n: zarr_lite.read_array(hs, n) for n in PROG + ("ke",)}
    for n in PROG:
        assert frames[n].shape == (4, LS + 1) and np.array_equal(frames[n][-1], a.spectrum(n, LS)), n
    assert np.array_equal(frames["ke"][-1], a.ke_spectrum(LS))
    a.close()
    prog = np.stack([read_history(hc, f) for f in PROG], 1)                   # [frames, 4, 6, N, N]
    for k in range(4):
        ref, ke = _twin_of_global(prog[k], a.dt, LS)
        for n in PROG:
            assert np.abs(frames[n][k] - ref[n]).max() <= 1e-12 * ref[n].max(), (k, n)
        assert np.abs(frames["ke"][k] - ke).max() <= 1e-12 * ke.max(), k
