"""Gradient synthesis (models/spectra.py::gradient / winds, the solver's
``gradient`` / ``rotational_wind`` / ``divergent_wind`` / ``band_wind``) with the
PyTorch twin on the CPU.  Every figure is printed before anything is asserted."""
import math

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine
from stsphere.models import spectra as ms
from stsphere.models.geometry import DAY, EARTH_RADIUS, CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout


def _solver(tmp, N=12, nd=1, case="tc5", model="swe", nsteps=12, **io):
    s = S.Solver({"parallelization": {"tiles_per_edge": 1, "num_devices": nd, "device_type": "cpu"},
                  "grid": {"N": N}, "physics": {"model": model, "case": case}, "time": {"nsteps": nsteps, "cfl": 0.9},
                  "io": dict({"output_dir": str(tmp)}, **io)}, verbose=False)
    s.initialize()
    return s


def _random_coeffs(C, L, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn((C, 2, L + 1, L + 1), dtype=torch.float64, generator=g)
    c = c * torch.tril(torch.ones(L + 1, L + 1, dtype=torch.float64))
    c[:, 1, :, 0] = 0.0
    return c


def test_against_central_differences():
    """C9 (a cell centre on each pole), lmax 12, random coefficients: the
    difference quotient of ``synthesise`` over a Cartesian displacement h = 1e-5
    along e_east and e_north of every cell's table longitude, poles included.
    Measured 1.8e-9 of max |grad|; bound 1e-6 (the quotient's own rounding)."""
    grid, L, R, h = CubedSphereGrid(9), 12, 3.0, 1e-5
    tb = ms.grid_tables(grid, L)
    c = _random_coeffs(2, L, 11)
    got = ms.gradient(c, tb, R)
    mu, cphi, lam = (tb.cell[:, k].numpy() for k in range(3))
    assert int((cphi == 0.0).sum()) == 2
    p = np.stack([cphi * np.cos(lam), cphi * np.sin(lam), mu], 1)
    frame = [np.stack([-np.sin(lam), np.cos(lam), 0.0 * lam], 1),
             np.stack([-mu * np.cos(lam), -mu * np.sin(lam), cphi], 1)]
    area = np.ones(p.shape[0])
    for k, e in enumerate(frame):
        side = []
        for sgn in (1.0, -1.0):
            x = p + sgn * h * e
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            side.append(ms.synthesise(c, ms.make_tables(x, area, 1.0, L)))
        fd = (side[0] - side[1]) / (2.0 * h * R)
        d = float((got[:, k] - fd).abs().max() / got.abs().max())
        print(f"{'east' if k == 0 else 'north'}: max |twin - difference quotient| / max |grad| = {d:.2e}")
        assert d <= 1e-6


def test_closed_form_solid_body():
    """psi = -R u0 sin phi is the one coefficient (1, 0) = -R u0 / sqrt(3):
    u = u0 cos phi, v = 0, a one-term sum."""
    R, u0, L = EARTH_RADIUS, 38.6, 5
    tb = ms.grid_tables(CubedSphereGrid(9, R), L)
    psi = torch.zeros((2, L + 1, L + 1), dtype=torch.float64)
    psi[0, 1, 0] = -R * u0 / math.sqrt(3.0)
    rot, div = ms.winds(psi, torch.zeros_like(psi), tb, R)
    du = float((rot[0] - u0 * tb.cell[:, 1]).abs().max() / u0)
    print(f"solid body: |u - u0 cos phi| / u0 {du:.1e}, |v| / u0 {float(rot[1].abs().max() / u0):.1e}")
    assert du <= 1e-13 and float(rot[1].abs().max()) == 0.0 and float(div.abs().max()) == 0.0


def _tc2_winds(tmp, N):
    s = _solver(tmp, N=N, case="tc2")
    u0 = 2.0 * math.pi * s.grid.radius / (12.0 * DAY)
    rot, div = s.rotational_wind(8), s.divergent_wind(8)
    assert rot.shape == div.shape == (2, 6, N, N) and rot.dtype == np.float64
    exact = u0 * ms.grid_tables(s.grid, 8).cell[:, 1].numpy().reshape(6, N, N)
    err = max(np.abs(rot[0] - exact).max(), np.abs(rot[1]).max()) / u0
    both = s.band_wind(8)
    assert np.array_equal(both, rot + div)
    return float(err), float(np.abs(div).max() / u0)


def test_tc2_rotational_wind_converges(tmp_path):
    """TC2 through the solver: the rotational wind to degree 8 against
    u0 cos phi, second order in the cell width.  Measured with the twin: error
    9.29e-4 at C24, 2.32e-4 at C48 (ratio 4.01); divergent wind over u0 1.034e-4 at
    C24 and 2.42e-5 at C48, asserted at twice that."""
    (e24, d24), (e48, d48) = _tc2_winds(tmp_path / "a", 24), _tc2_winds(tmp_path / "b", 48)
    print(f"tc2 rotational wind error / u0: C24 {e24:.3e} C48 {e48:.3e} ratio {e24 / e48:.3f}; "
          f"divergent wind / u0: C24 {d24:.3e} C48 {d48:.3e}")
    assert e24 / e48 >= 3.0
    assert d24 <= 2 * 1.034e-4 and d48 <= 2 * 2.42e-5


def test_contracts(tmp_path):
    e = Engine(ShallowWater("tc5"), TileLayout(12, 2, 1, ng=2), grid=CubedSphereGrid(12))
    # lmax = 0: zeros
    z = e.spectra(0).gradient(torch.full((3, 2, 1, 1), 7.0, dtype=torch.float64))
    assert z.shape == (3, 2, e.plan.T, e.plan.n, e.plan.n) and float(z.abs().max()) == 0.0
    assert float(ms.gradient(torch.ones(1, 2, 1, 1, dtype=torch.float64), e.spectra(0).tab, 1.0).abs().max()) == 0.0
    # finite garbage at m > l and in S_l0 changes no bit; any C >= 1
    sp, c = e.spectra(9), _random_coeffs(3, 9, 5)
    bad = c.clone()
    bad[..., torch.triu(torch.ones(10, 10, dtype=torch.bool), 1)] = 1e300
    bad[:, 1, :, 0] = 1e300
    a, b = sp.gradient(c), sp.gradient(bad)
    assert a.shape == (3, 2, e.plan.T, e.plan.n, e.plan.n) and a.dtype == torch.float64
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    assert torch.equal(sp.gradient(c, chunks=9), a)
    for L, k in ((1, 1), (9, 1), (9, 4), (9, 9), (47, 7)):
        bd = ms.grad_chunk_bounds(L, k)
        assert bd[0] == 1 and bd[-1] == L + 1 and len(bd) == k + 1 and all(x < y for x, y in zip(bd, bd[1:]))
    # refusals
    ok = torch.zeros(2, 2, 10, 10, dtype=torch.float64)
    for call in (lambda: sp.gradient(ok[0]), lambda: sp.gradient(ok[:, :1]), lambda: sp.gradient(ok[..., :9]),
                 lambda: sp.gradient(ok.float()), lambda: sp.gradient(ok[:0]), lambda: sp.gradient(ok[:, :, :9, :9]),
                 lambda: sp.gradient(ok, chunks=0), lambda: sp.gradient(ok, chunks=10)):
        with pytest.raises(ValueError):
            call()
    s = _solver(tmp_path / "a")
    assert s.gradient(np.zeros((2, 6, 6))).shape == (2, 6, 12, 12)
    assert s.gradient(np.zeros((3, 2, 6, 6))).shape == (3, 2, 6, 12, 12)
    for call in (lambda: s.gradient(np.zeros((2, 6, 5))), lambda: s.gradient(np.zeros((2, 25, 25))),
                 lambda: s.rotational_wind(24), lambda: s.band_wind(5, 4, 3)):
        with pytest.raises(ValueError):
            call()
    d = _solver(tmp_path / "b", model="diffusion", case="lima_flag")
    for call in (d.rotational_wind, d.divergent_wind, d.band_wind):
        with pytest.raises(ValueError, match="shallow-water"):
            call(5)


def test_six_virtual_ranks_and_the_cli(tmp_path):
    """Every rank its own cells, tiles gathered: six virtual ranks equal one;
    the ``synth`` command writes u, v of the same winds from a history."""
    from stsphere.__main__ import main as cli
    one, six = _solver(tmp_path / "a"), _solver(tmp_path / "b", nd=6)
    assert six.mode == "virtual" and len(six.engines) == 6
    for name in ("rotational_wind", "divergent_wind"):
        a, b = getattr(one, name)(9), getattr(six, name)(9)
        d = float(np.abs(a - b).max() / np.abs(a).max())
        print(f"{name}: six ranks against one {d:.1e}")
        assert d <= 1e-12
    s = _solver(tmp_path / "run", nsteps=2, history_interval=2)
    s.run()
    out = tmp_path / "w.npz"
    assert cli(["synth", str(tmp_path / "run" / "history.zarr"), "rotational_wind", "9", str(out)]) == 0
    r = np.load(out)
    want = s.rotational_wind(9)
    assert r["u"].shape[1:] == (6, 12, 12) and r["v"].shape == r["u"].shape
    d = float(max(np.abs(r["u"][-1] - want[0]).max(), np.abs(r["v"][-1] - want[1]).max()) / np.abs(want).max())
    print(f"cli rotational_wind against the solver {d:.1e}")
    assert d <= 1e-12
