"""The gfx950 synthesis kernel (ops/csrc/synth_kernel.hip) against its PyTorch
twin (models/spectra.py::synthesise), and its plumbing through the solver.

The bound is the project's fp64 bound: per channel max |kernel - twin| <= 1e-12
max |twin|; both sides get the same coefficient tensor.  Every figure is
printed before anything is asserted."""
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

pytestmark = pytest.mark.gpu

# (N, tiles per edge).  (9, 1): odd N, a cell centre on each pole, 486 cells (ragged
# last batch, as the 864 of (12, 1) and the 7776 of (36, 3)); 3456 and 9600 are whole batches
SHAPES = [(9, 1), (12, 1), (24, 2), (36, 3), (40, 1)]
CASES = ["tc5", "tc6"]
# 15, 16, 17 straddle a 16-degree tile, 31, 32, 33 the 32-degree group (where N allows);
# the last is 2N - 1.  lmax = 0 has a test of its own
LMAXES = {9: (1, 15, 16, 17), 12: (1, 15, 16, 17, 23), 24: (1, 15, 16, 17, 31, 32, 33, 47),
          36: (1, 15, 16, 17, 31, 32, 33, 71), 40: (1, 15, 16, 17, 31, 32, 33, 79)}
NAMES7 = ("h", "mx", "my", "mz", "vorticity", "divergence", "pv")
BOUND = 1e-12


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


@functools.lru_cache(maxsize=None)
def _gpu(N, t, dtype=torch.float64):
    return _engine(N, t, "tc5", dtype, "cuda:0", "hip", rounded=dtype == torch.float32)


def _seven(twin, der, L):
    """The twin's coefficients [7, 2, L+1, L+1] of the state and of ``der`` [3, T, n, n]."""
    sp = twin.spectra(L)
    return torch.cat([sp.partial_fields(), sp.partial_tiles(der.double())])


def _random(C, L, seed):
    """Seeded lower-triangular coefficients, scaled by (l+1)^-2."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn((C, 2, L + 1, L + 1), dtype=torch.float64, generator=g)
    c = c * torch.tril(torch.ones(L + 1, L + 1, dtype=torch.float64))
    c[:, 1, :, 0] = 0.0
    return c / (torch.arange(L + 1, dtype=torch.float64)[:, None] + 1.0) ** 2


def _garbage(c, value=1e300):
    L = c.shape[-1] - 1
    bad = c.clone()
    bad[..., torch.triu(torch.ones(L + 1, L + 1, dtype=torch.bool), 1)] = value
    bad[:, 1, :, 0] = value
    return bad


def _diff(got, ref):
    """Per channel max |got - ref| / max |ref|."""
    got, ref = got.reshape(ref.shape[0], -1).cpu(), ref.reshape(ref.shape[0], -1)
    return ((got - ref).abs().amax(1) / ref.abs().amax(1)).tolist()


def _check(tag, e, twin, coeffs_of, lmaxes, names):
    assert e.spectra(1).hip and not twin.spectra(1).hip
    bad = []
    for L in lmaxes:
        c = coeffs_of(L)
        got = e.spectra(L).synthesise(c.to(e.device))
        assert got.dtype == torch.float64 and got.shape == (c.shape[0], e.plan.T, e.plan.n, e.plan.n)
        d = _diff(got, ms.synthesise(c, twin.spectra(L).tab))
        print(f"{tag} lmax {L} chunks {e.spectra(L).default_chunks()}: " +
              " ".join(f"{n} {v:.1e}" for n, v in zip(names, d)))
        bad += [(L, n, v) for n, v in zip(names, d) if not v <= BOUND]
    assert not bad, bad


# ---- 1. seven channels of a state ------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_seven_channels(N, t, case):
    """The twin's coefficients of h, mx, my, mz, vorticity, divergence and pv two
    steps in.  Measured on an MI355X: see profiles/synthesis/README.md."""
    twin = _state(N, t, case)
    der = twin.derived()[0]
    _check(f"seven C{N} t={t} {case}", _gpu(N, t), twin, lambda L: _seven(twin, der, L), LMAXES[N], NAMES7)


# ---- 2. seeded random coefficients: column predication ----------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 8])
@pytest.mark.parametrize("N,t", SHAPES)
def test_random_coefficients(N, t, C):
    _check(f"random C{N} t={t} C={C}", _gpu(N, t), _state(N, t, "tc5"), lambda L: _random(C, L, 100 * C + L),
           LMAXES[N], [f"ch{k}" for k in range(C)])


# ---- 3. lmax = 0 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,t", SHAPES)
def test_lmax_zero(N, t):
    """P_00 = 1, cos 0 = 1: every cell is C_00 bit for bit."""
    e = _gpu(N, t)
    c = torch.tensor([1.0 / 3.0, -2.5e7, 1e-300], dtype=torch.float64).reshape(3, 1, 1, 1).repeat(1, 2, 1, 1)
    got = e.spectra(0).synthesise(c.to(e.device)).cpu()
    print(f"lmax0 C{N} t={t}: " + " ".join(f"{float((got[k] - c[k, 0, 0, 0]).abs().max()):.1e}" for k in range(3)))
    for k in range(3):
        assert torch.equal(got[k], torch.full_like(got[k], float(c[k, 0, 0, 0])))
    _check(f"lmax0 C{N} t={t}", e, _state(N, t, "tc5"), lambda L: _random(2, L, 1), (0,), ("ch0", "ch1"))


# ---- 4. order chunks: the record-and-fold path ------------------------------------------------------
@pytest.mark.parametrize("chunks", [1, 2, 3, 34])
def test_chunks(chunks):
    e, twin, L = _gpu(24, 2), _state(24, 2, "tc5"), 33
    sp = e.spectra(L)
    c = _seven(twin, twin.derived()[0], L)
    ref = ms.synthesise(c, twin.spectra(L).tab)
    a = sp.synthesise(c.to(e.device), chunks=chunks)
    b = sp.synthesise(c.to(e.device), chunks=chunks)
    torch.cuda.synchronize()
    d = _diff(a, ref)
    print(f"chunks {chunks} bounds {ms.chunk_bounds(L, chunks)}: " + " ".join(f"{v:.1e}" for v in d))
    assert max(d) <= BOUND
    assert torch.equal(a, b)


def test_default_chunks_fill_the_device():
    """The fewest chunks that make the grid at least twice the compute units:
    small shapes take the fold path by default."""
    e = _gpu(24, 2)
    sp = e.spectra(33)
    cus = torch.cuda.get_device_properties(e.device).multi_processor_count
    k = sp.default_chunks()
    print(f"C24: {sp.cells} cells, {cus} compute units, default chunks {k}")
    assert 1 <= k <= 34 and k == max(1, min(34, -(-2 * cus // 27)))


# ---- 5. the upper triangle and S_l0 are never read ---------------------------------------------------
@pytest.mark.parametrize("chunks", [1, 3])
def test_upper_triangle_is_not_read(chunks):
    e = _gpu(12, 1)
    sp = e.spectra(17)
    c = _random(3, 17, 9)
    a = sp.synthesise(c.to(e.device), chunks=chunks)
    b = sp.synthesise(_garbage(c).to(e.device), chunks=chunks)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


def test_pole_cells_on_the_device():
    """C9: the cells whose centres are the poles (cos phi = 0 exactly) against
    sum_l (+-1)^l C_l0 sqrt(2l + 1), bound 1e-12 of sum_l |C_l0| sqrt(2l + 1)."""
    e, L = _gpu(9, 1), 17
    sp = e.spectra(L)
    cell = sp.tab.cell.cpu()
    at = torch.nonzero(cell[:, 1] == 0.0).reshape(-1)
    assert at.numel() == 2
    c = _random(2, L, 4)
    f = sp.synthesise(c.to(e.device)).reshape(2, -1).cpu()
    root = torch.sqrt(2.0 * torch.arange(L + 1, dtype=torch.float64) + 1.0)
    for k in at.tolist():
        sign = torch.sign(cell[k, 0]) ** torch.arange(L + 1, dtype=torch.float64)
        want, scale = (c[:, 0, :, 0] * root * sign).sum(1), (c[:, 0, :, 0].abs() * root).sum(1)
        d = (f[:, k] - want).abs() / scale
        print(f"pole cell mu = {float(cell[k, 0]):+.0f}: " + " ".join(f"{v:.1e}" for v in d.tolist()))
        assert float(d.max()) <= 1e-12


# ---- 6. / 7. the solver after fused stepping, fp64 and fp32 -------------------------------------------
def _gpu_cfg(out, nd=1, t=2, dtype="float64", **io):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "gpu"},
            "grid": {"N": 24, "dtype": dtype}, "physics": {"model": "swe", "case": "tc5"}, "time": {"nsteps": 12},
            "runtime": {"fused": "on" if nd == 1 else "auto"}, "io": dict({"output_dir": str(out)}, **io)}


LS = 20


def _twin_products(state, dt, zd=None):
    """psi, chi (lmax = LS) and band_field('h', 20, 2, 10) of the CPU twin on a
    global state [4, 6, N, N]; ``zd``: vorticity and divergence [2, 6, N, N]
    when they are given rather than the derived-field twin's."""
    N = state.shape[-1]
    e = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), dt=dt)
    e.set_state(torch.as_tensor(state))
    sp = e.spectra(LS)
    zd = e.derived()[0][:2] if zd is None else torch.as_tensor(zd)
    c = sp.partial_tiles(zd)
    psi, chi = ms.helmholtz(c[0], c[1], e.grid.radius)
    hb = ms.scale_degrees(sp.partial_fields()[:1], ms.band_factors(LS, 2, 10))
    f = ms.synthesise(torch.cat([psi[None], chi[None], hb]), sp.tab).reshape(3, 6, N, N).numpy()
    return {"psi": f[0], "chi": f[1], "band": f[2]}


def _solver_products(s):
    return {"psi": s.streamfunction(LS), "chi": s.velocity_potential(LS), "band": s.band_field("h", LS, 2, 10)}


def _compare(tag, got, ref):
    d = {n: float(np.abs(got[n] - ref[n]).max() / np.abs(ref[n]).max()) for n in ref}
    print(f"{tag}: " + " ".join(f"{n} {v:.1e}" for n, v in d.items()))
    for n in ref:
        assert got[n].shape == ref[n].shape and got[n].dtype == np.float64 and d[n] <= BOUND, n


def test_solver_after_fused_stepping(tmp_path):
    """The ghost slots of the padded state are not current after a fused
    multi-step launch; neither transform reads one."""
    s = S.Solver(_gpu_cfg(tmp_path), verbose=False)
    s.initialize()
    s.step(6)
    assert s.fused is not None
    _compare("fused fp64", _solver_products(s), _twin_products(s.gather_global(), s.dt))
    s.close()


def test_solver_after_fused_stepping_fp32(tmp_path):
    """An fp32 engine against the fp64 twin on the fp32-rounded state (what
    ``gather_global`` returns): both transforms compute in double after the load.
    The vorticity and the divergence of an fp32 engine are fp32 fields of the
    derived-field kernel, whose own rounding (tests/test_derived_gpu.py) is not
    the subject here: the twin gets those fields as the solver returns them."""
    s = S.Solver(_gpu_cfg(tmp_path, dtype="float32"), verbose=False)
    s.initialize()
    s.step(6)
    assert s.fused is not None and s.engines[0].dtype == torch.float32
    zd = np.stack([s.derived_field("vorticity"), s.derived_field("divergence")])
    _compare("fused fp32", _solver_products(s), _twin_products(s.gather_global(), s.dt, zd))
    s.close()


def test_fp32_engine_seven_channels():
    """The kernel's arithmetic is double whatever the engine's state type."""
    c32 = _engine(24, 2, "tc6", torch.float32, "cpu", "torch", rounded=True)
    c64 = _engine(24, 2, "tc6", torch.float64, "cpu", "torch", rounded=True)
    der = c32.derived()[0]
    assert der.dtype == torch.float32
    _check("seven fp32 C24 t=2 tc6", _gpu(24, 2, torch.float32), c64, lambda L: _seven(c64, der, L), LMAXES[24], NAMES7)


# ---- 8. virtual ranks --------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [2, 6])
def test_virtual_ranks_on_one_gpu(tmp_path, nd):
    one = S.Solver(_gpu_cfg(tmp_path / "one", t=1), verbose=False)
    one.initialize()
    one.step(2)
    state = one.gather_global()
    many = S.Solver(_gpu_cfg(tmp_path / "many", nd=nd, t=1), verbose=False)
    many.initialize()
    assert many.mode == "virtual" and len(many.engines) == nd
    for e in many.engines:
        e.set_state(torch.as_tensor(np.stack([e.geo.gather_global(v) for v in state])))
    _compare(f"{nd} virtual ranks", _solver_products(many), _solver_products(one))
    one.close()
    many.close()
