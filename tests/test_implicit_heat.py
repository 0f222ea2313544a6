"""Implicit consistent diffusion on the CPU: the twin of the BiCGStab Helmholtz solve
(models/diffusion.py::helmholtz_bicgstab through ops/heat.py::HeatOperator.solve) against
a dense solve, conservation, the order of Crank-Nicolson, and the refusals.  Every figure is
printed before it is asserted."""
import functools

import numpy as np
import pytest
import torch

import rough_states as rs
from stsphere import driver as S
from stsphere.engine import Engine, VirtualCluster
from stsphere.models.diffusion import ConsistentDiffusion
from stsphere.parallel.layout import TileLayout

TOL = 1e-10
EPS = 2.0 ** -52


def engine(N, t, device="cpu", dtype=torch.float64, case="harmonic"):
    # C6 in two tiles per edge has 3 x 3 tiles: one ghost layer (the operator reads no ghost slot)
    return Engine(ConsistentDiffusion(case=case), TileLayout(N, t, 1, ng=1 if N // t < 4 else 2), grid=rs.grid_of(N),
                  dtype=dtype, device=device, backend="torch" if device == "cpu" else "hip")


@functools.lru_cache(maxsize=None)
def dense_laplacian(N, t):
    """L as a dense float64 matrix in the rank's cell order: column j is the twin's
    Laplacian of unit vector j."""
    op = engine(N, t).heat_operator()
    op._setup_solver()
    m = op.T * op.n * op.n
    L, u = np.zeros((m, m)), torch.zeros((op.T, op.n, op.n), dtype=torch.float64)
    for j in range(m):
        u.view(-1)[j] = 1.0
        L[:, j] = op._twin_laplacian(u).reshape(-1).numpy()
        u.view(-1)[j] = 0.0
    return L


@functools.lru_cache(maxsize=None)
def dense_system(N, t, c):
    """(tau, A, cond(A), b): A = I - tau L with tau lam = c; b a rough right-hand side [T, n, n]."""
    L = dense_laplacian(N, t)
    tau = c / ConsistentDiffusion.lam(rs.grid_of(N))
    A = np.eye(len(L)) - tau * L
    n = N // t
    b = torch.rand((6 * t * t, n, n), generator=torch.Generator().manual_seed(N + t), dtype=torch.float64) - 0.5
    return tau, A, float(np.linalg.cond(A)), b


def relative_error(x, A, b):
    ref = np.linalg.solve(A, b.reshape(-1).double().numpy())
    return float(np.linalg.norm(x.detach().cpu().double().reshape(-1).numpy() - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("c", [1.0, 50.0])
@pytest.mark.parametrize("t", [1, 2])
def test_solve_matches_dense_solve(t, c):
    tau, A, cond, b = dense_system(6, t, c)
    x, rec = engine(6, t).heat_operator().solve(b, tau, tol=TOL)
    err = relative_error(x, A, b)
    print(f"C6 t={t} tau lam={c:g}: {rec}, error {err:.2e}, cond {cond:.1f}, bound {10 * cond * TOL:.2e}")
    assert rec["flag"] == 1 and rec["residual"] <= TOL and err <= 10 * cond * TOL


def test_backward_euler_conserves():
    e = engine(12, 2)
    dt, A = 50.0 * e.physics.max_dt(e.grid, 1.0), torch.as_tensor(e.geo.area)
    m0, scale = float((e.tiles_view()[0] * A).sum()), float((e.tiles_view()[0].abs() * A).sum())
    T0 = e.tiles_view().clone()
    rec = e.heat_operator().implicit_step(dt, e.physics.kappa, 1.0, tol=TOL)
    drift = abs(float((e.tiles_view()[0] * A).sum()) - m0) / scale
    print(f"backward Euler C12 at 50 x the explicit bound: {rec}, drift {drift:.2e}")
    # each iteration rounds x twice per cell
    assert drift <= 4 * EPS * rec["iterations"] and not torch.equal(T0, e.tiles_view()) and e.step_count == 1


def test_crank_nicolson_is_second_order(tmp_path):
    """C96 ``harmonic`` to t = R^2 / (20 kappa) = 1014811.1 s (one e-folding time) in 1, 2 and 4
    steps: dt = 1014811.1, 507405.6 and 253702.8 s, 2232, 1116 and 558 times the explicit bound.
    The twin's ``err_linf`` are 9.35e-2, 2.11e-2 and 4.92e-3: ratios 4.43 and 4.28.  The
    Crank-Nicolson factor ((1 - z / 2) / (1 + z / 2))^k against exp(-1) at z = 1 / k alone gives
    4.38 and 4.09; the spatial error (1.3e-4 here, of the other sign) adds the rest."""
    errs = []
    for ns in (1, 2, 4):
        c = {"parallelization": {"num_devices": 1}, "grid": {"N": 96},
             "physics": {"model": "diffusion", "case": "harmonic", "operator": "consistent",
                         "implicit": {"theta": 0.5}},
             "time": {"dt": rs.grid_of(96).radius ** 2 / (20 * 2.0e6) / ns, "integrator": "rk4"},
             "io": {"output_dir": str(tmp_path / str(ns))}}
        s = S.Solver(c, verbose=False)
        out = s.run(nsteps=ns)
        errs.append(out["err_linf"])
        assert out["implicit_iterations"]["max"] >= out["implicit_iterations"]["mean"] > 1 and s.step_count == ns
    print(f"Crank-Nicolson C96: errors {errs}, ratios {errs[0] / errs[1]:.2f}, {errs[1] / errs[2]:.2f}")
    assert errs[0] / errs[1] >= 3.5 and errs[1] / errs[2] >= 3.5


def solver_helmholtz_error(out, device_type, N, t):
    """``Solver.helmholtz`` at tau lam = 50 through the global cell order [6, N, N] and back:
    (relative error against the dense solve, 10 cond(A) tol, the solver)."""
    c = {"parallelization": {"num_devices": 1, "tiles_per_edge": t, "device_type": device_type},
         "grid": {"N": N, "halo": 1 if N // t < 4 else 2}, "io": {"output_dir": str(out)},
         "physics": {"model": "diffusion", "operator": "consistent"}}
    s = S.Solver(c, verbose=False)
    s.initialize()
    tau, A, cond, b = dense_system(N, t, 50.0)
    x = s.helmholtz(s._gather_tiles({0: b.numpy()}), tau)
    assert x.shape == (6, N, N) and s.helmholtz_record["flag"] == 1
    return relative_error(torch.as_tensor(s.engines[0].geo.gather_global(x)), A, b), 10 * cond * TOL, s


def test_solver_helmholtz(tmp_path):
    err, bound, _ = solver_helmholtz_error(tmp_path, "cpu", 6, 2)
    print(f"Solver.helmholtz C6 t=2: error {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    c = {"parallelization": {"num_devices": 1}, "grid": {"N": 6}, "io": {"output_dir": str(tmp_path)},
         "physics": {"model": "swe", "case": "tc2"}}
    s = S.Solver(c, verbose=False)
    s.initialize()
    with pytest.raises(ValueError, match="one scalar field"):
        s.helmholtz(np.zeros((6, 6, 6)), 1.0)


@pytest.mark.parametrize("phys,nd,match", [
    ({"model": "diffusion", "operator": "consistent", "implicit": {"theta": 0.7}}, 1, "theta"),
    ({"model": "diffusion", "operator": "two_point", "implicit": {"theta": 1.0}}, 1, "physics.implicit"),
    ({"model": "swe", "case": "tc2", "implicit": {"theta": 1.0}}, 1, "physics.implicit"),
    ({"model": "diffusion", "operator": "consistent", "implicit": {"theta": 1.0}}, 6, "virtual ranks"),
])
def test_config_refusals(tmp_path, phys, nd, match):
    c = {"parallelization": {"num_devices": nd}, "grid": {"N": 8}, "physics": phys,
         "io": {"output_dir": str(tmp_path)}}
    with pytest.raises(ValueError, match=match):
        S.Solver(c, verbose=False).initialize()


def test_solve_refusals():
    vc = VirtualCluster(lambda: ConsistentDiffusion(), TileLayout(8, 1, 6, ng=2), grid=rs.grid_of(8))
    op = vc.engines[0].heat_operator()
    with pytest.raises(ValueError, match="remote ghosts"):
        op.solve(torch.zeros((op.T, op.n, op.n), dtype=torch.float64), 1.0)
    tau, _, _, b = dense_system(6, 1, 50.0)
    with pytest.raises(RuntimeError, match="no convergence") as err:
        engine(6, 1).heat_operator().solve(b, tau, maxiter=1)
    assert err.value.record["iterations"] == 1 and err.value.record["flag"] == 0
