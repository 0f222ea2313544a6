"""Grid transfer between C_N grids (models/transfer.py, the twin) through
``Solver.set_from_cubed`` / ``resampled_state`` on the CPU."""
import math

import numpy as np
import pytest

from stsphere.__main__ import main
from stsphere.driver import Solver
from stsphere.models import transfer as mt
from stsphere.models.geometry import EARTH_RADIUS, CubedSphereGrid

EPS = float(np.finfo(np.float64).eps)
SWE = {"model": "swe", "case": "tc2", "tracers": ["constant", "cosine_bell"]}


def config(N, t=1, physics=SWE, device="cpu", dtype="float64"):
    return {"parallelization": {"num_devices": 6 if t > 1 else 1, "tiles_per_edge": t, "device_type": device},
            "grid": {"N": N, "dtype": dtype}, "physics": physics}


def solver(N, t=1, physics=SWE, **kw):
    s = Solver(config(N, t, physics, **kw), verbose=False)
    s.initialize()
    return s


def mass(q, N):
    """fsum(q A) and fsum(|q A|) per row of [F, 6, N, N]."""
    A = CubedSphereGrid(N, EARTH_RADIUS).areas()
    return [(math.fsum((q[f] * A).ravel()), math.fsum(np.abs(q[f] * A).ravel())) for f in range(len(q))]


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("Ns", [4, 6])
@pytest.mark.parametrize("r", [2, 4])
def test_conservation_and_round_trip(r, Ns, t):
    """sum(q A) of h and the tracer masses (rows 0, 4, 5) against math.fsum, both
    directions, and refine-then-coarsen against the source.  Measured with the twin
    over these cases: the sums differ by at most 0.0022 eps cells of sum |q A| (cells =
    6 N^2 of the fine grid), the round trip by 2.1 eps of max |q|; bounds 10 x that."""
    coarse, fine = solver(Ns, t if Ns // t >= 4 else 1), solver(r * Ns, t)      # a tile holds two halo widths
    src = coarse.gather_global()
    fine.set_from_cubed(src)
    up = fine.gather_global()
    coarse.set_from_cubed(up)
    back = coarse.gather_global()
    assert fine.step_count == 0 and np.array_equal(fine.resampled_state(Ns), back)
    cells = 6 * (r * Ns) ** 2
    ms, mu, mb = mass(src, Ns), mass(up, r * Ns), mass(back, Ns)
    for f in (0, 4, 5):
        drift = max(abs(mu[f][0] - ms[f][0]), abs(mb[f][0] - mu[f][0])) / ms[f][1]
        trip = np.abs(back[f] - src[f]).max() / np.abs(src[f]).max()
        print(f"row {f}: drift {drift / (EPS * cells):.3g} eps cells, round trip {trip / EPS:.3g} eps")
        assert drift <= 0.022 * EPS * cells and trip <= 21 * EPS


@pytest.mark.parametrize("r", [2, 4])
def test_limiter_keeps_a_cap_in_bounds(r):
    s = solver(6 * r, 1, {"model": "advection"})
    cap = (CubedSphereGrid(6).centers()[..., 2] > 0.3).astype(np.float64)[None]
    s.set_from_cubed(cap)
    q = s.gather_global()
    assert q.min() == 0.0 and q.max() == 1.0 and 0.0 < q.mean() < 1.0
    s.set_from_cubed(cap, limiter="none")
    q = s.gather_global()
    assert q.min() < 0.0 and q.max() > 1.0


def test_second_order():
    """l2 error of refining z (x^2 - y^2) from Ns = 8, 16, 32 by 2: measured
    4.03e-3, 8.16e-4, 1.96e-4 (ratios 4.94, 4.17)."""
    class Scalar:
        F, name = 1, "advection"
    f = lambda g: g.centers()[..., 2] * (g.centers()[..., 0] ** 2 - g.centers()[..., 1] ** 2)
    err = []
    for Ns in (8, 16, 32):
        gs, gt = CubedSphereGrid(Ns), CubedSphereGrid(2 * Ns)
        out = mt.transfer(f(gs)[None], Scalar, 2 * Ns, gs.radius)[0].numpy()
        err.append(math.sqrt(((out - f(gt)) ** 2 * gt.areas()).sum() / gt.areas().sum()))
    print(err, err[0] / err[1], err[1] / err[2])
    assert err[0] / err[1] >= 3.5 and err[1] / err[2] >= 3.5


@pytest.mark.parametrize("r", [2, 8])
def test_swe_momentum_tangent_and_constant_tracer(r):
    fine = solver(4 * r)
    fine.set_from_cubed(solver(4).gather_global())
    q = fine.gather_global()
    c = np.moveaxis(fine.grid.centers(), -1, 0)
    Mn = np.sqrt((q[1:4] ** 2).sum(0))
    assert (np.abs((q[1:4] * c).sum(0)) <= 4 * EPS * Mn.max()).all() and Mn.max() > 0
    assert np.abs(q[4] / q[0] - 1.0).max() <= 8 * EPS


def test_refusals_and_cli_round_trip(tmp_path):
    s = solver(6)
    for bad in (np.zeros((6, 6, 2, 2)), np.zeros((6, 6, 18, 18)), np.zeros((4, 6, 12, 12)), np.zeros((6, 6, 12, 6))):
        with pytest.raises(ValueError, match="grid transfer"):
            s.set_from_cubed(bad)
    with pytest.raises(ValueError, match="limiter"):
        s.set_from_cubed(np.ones((6, 6, 3, 3)), limiter="minmod")
    import yaml
    cfg = {k: dict(v) for k, v in config(12).items()}
    (tmp_path / "c12.yaml").write_text(yaml.safe_dump(cfg))
    s._initial_condition_stage(str(tmp_path / "c6.zarr"))
    assert main(["resample", str(tmp_path / "c6.zarr"), "0", str(tmp_path / "c12.yaml"), str(tmp_path / "c12.zarr")]) == 0
    cfg["io"] = {"initial_condition": str(tmp_path / "c12.zarr")}
    t = Solver(cfg, verbose=False)
    t.initialize()
    want = mt.transfer(s.gather_global(), s.physics, 12, s.grid.radius).numpy()
    assert np.array_equal(t.gather_global(), want)
    t.step(1)
    assert t.all_finite()
