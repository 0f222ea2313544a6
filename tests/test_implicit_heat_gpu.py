"""The gfx950 BiCGStab Helmholtz solve (ops/csrc/helmholtz_kernel.hip) through
ops/heat.py::HeatOperator.solve: against a dense float64 solve, against the twin's iterates,
reproducibility, the flag and no-op rule (a chunk launched with a flag set, convergence inside
a chunk), ``Solver.helmholtz`` and the entry point's checks.  Measured values:
profiles/implicit_heat/README.md."""
import ctypes

import pytest
import torch

from stsphere.ops import heat
from test_implicit_heat import TOL, dense_system, engine, relative_error, solver_helmholtz_error

pytestmark = pytest.mark.gpu

# (N, tiles per edge): one ragged block per tile; 3 x 3 tiles; 16 + a block one cell wide; 24 tiles of 9 x 9
# (17 is odd: C18 stands in for the two-tiles-per-edge case of C17)
SHAPES = [(6, 1), (6, 2), (17, 1), (18, 2)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("c", [1.0, 50.0])
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_matches_dense_solve(N, t, c, dtype):
    tau, A, cond, b = dense_system(N, t, c)
    op = engine(N, t, "cuda:0", dtype).heat_operator()
    assert op.hip
    b = b.to(dtype)                     # the reference solves for the rounded right-hand side
    x, rec = op.solve(b.cuda(), tau, tol=TOL)
    err = relative_error(x, A, b)
    bound = 10 * cond * TOL + (2.0 ** -23 if dtype == torch.float32 else 0.0)
    print(f"C{N} t={t} tau lam={c:g} {dtype}: {rec}, error {err:.2e}, cond {cond:.1f}, bound {bound:.2e}")
    assert x.dtype == dtype and rec["flag"] == 1 and rec["residual"] <= TOL and err <= bound


def test_iterates_match_twin():
    tau, _, _, b = dense_system(17, 1, 50.0)
    xs = []
    for device in ("cpu", "cuda:0"):
        op = engine(17, 1, device).heat_operator()
        with pytest.raises(RuntimeError, match="no convergence") as err:
            op.solve(b.to(device), tau, tol=0.0, maxiter=8, chunk=8)
        assert err.value.record["iterations"] == 8
        xs.append(op._row(heat.RX).cpu().clone())
    diff = float((xs[0] - xs[1]).abs().max() / xs[0].abs().max())
    print(f"C17 tau lam=50, x after one chunk of 8 iterations: kernel against twin {diff:.2e}")
    assert float(xs[0].abs().max()) > 0 and diff <= 1e-11


def test_reproducible_and_converged_start_is_untouched():
    tau, _, _, b = dense_system(17, 1, 50.0)
    op = engine(17, 1, "cuda:0").heat_operator()
    x1, r1 = op.solve(b.cuda(), tau, tol=1e-12)
    x2, r2 = op.solve(b.cuda(), tau, tol=1e-12)
    assert torch.equal(x1, x2) and r1 == r2 and r1["iterations"] > 8
    # x1 passes the looser test in the set-up, so solve launches no chunk at all
    x3, r3 = op.solve(b.cuda(), tau, x0=x1, tol=TOL, chunk=8)
    print(f"two solves: {r1}; from the converged x: {r3}")
    assert r3["iterations"] == 0 and r3["flag"] == 1 and torch.equal(x3, x1)
    assert torch.equal(op._row(heat.RX), x1)


@pytest.mark.parametrize("flag", [1, 2])
def test_chunk_after_a_flag_is_a_no_op(flag):
    """A chunk of 8 iterations launched with CONVERGED (1) or BREAKDOWN (2) set: every work
    row and the scalar block keep their bits.  alpha, omega and beta are set to 0.5 first
    (the set-up leaves them 0, with which s, x, r and p would not move anyway)."""
    tau, _, _, b = dense_system(17, 1, 50.0)
    op = engine(17, 1, "cuda:0").heat_operator()
    x1, _ = op.solve(b.cuda(), tau, tol=1e-12)          # rows v, s, t hold a finished solve's vectors
    if flag == 2:
        b = b.clone()
        b[0, 0, 0] = float("nan")                       # (b, b) is not finite: the set-up flags a breakdown
    op._row(heat.RB).copy_(b)
    op._row(heat.RX).copy_(x1)
    rec0 = op._launch_solver(0, 0, tau, TOL)
    op.block[1:4] = 0.5
    bits = lambda: (op.work.view(torch.int64).clone(), op.block.view(torch.int64).clone())
    w0, k0 = bits()
    rec1 = op._launch_solver(1, 8, tau, TOL)
    w1, k1 = bits()
    print(f"flag {flag}: after the set-up {rec0}, after a chunk of 8 {rec1}")
    assert rec0["flag"] == flag and (rec1["flag"], rec1["iterations"]) == (flag, 0)
    assert bool(op._row(heat.RP).isnan().any() if flag == 2 else (op._row(heat.RP) != 0).any())
    assert torch.equal(w0, w1) and torch.equal(k0, k1)


def test_convergence_inside_a_chunk_matches_twin():
    """tau lam = 1 converges at iteration 11, inside the second chunk of 8: iterations
    12 .. 16 are launched and must leave x and the count alone."""
    tau, _, _, b = dense_system(17, 1, 1.0)
    x0, r0 = engine(17, 1).heat_operator().solve(b, tau, tol=TOL)
    x1, r1 = engine(17, 1, "cuda:0").heat_operator().solve(b.cuda(), tau, tol=TOL, chunk=8)
    diff = float((x0 - x1.cpu()).abs().max() / x0.abs().max())
    print(f"twin {r0}, kernel {r1}: final x differs by {diff:.2e}")
    assert r0["iterations"] == r1["iterations"] and 8 < r1["iterations"] < 16 and diff <= 1e-11


def test_solver_helmholtz_two_tiles_per_edge(tmp_path):
    err, bound, s = solver_helmholtz_error(tmp_path, "gpu", 18, 2)
    print(f"Solver.helmholtz C18 t=2 on the GPU: error {err:.2e}, bound {bound:.2e}")
    assert s.engines[0].heat_operator().hip and err <= bound


def test_entry_point_rejects_bad_descriptors():
    op = engine(17, 1, "cuda:0").heat_operator()
    op._setup_solver()
    assert op.lib.stsp_helmholtz_desc_size() == ctypes.sizeof(heat.HelmDesc)

    def rc(**kw):
        d = heat.HelmDesc()
        ctypes.memmove(ctypes.byref(d), ctypes.byref(op.hdesc), ctypes.sizeof(d))
        d.op, d.iters, d.tau, d.tol = 1, 8, 1.0, TOL
        for k, v in kw.items():
            setattr(d, k, v)
        return op.lib.stsp_helmholtz_launch(d, 0)
    assert rc(n=0) == 1 and rc(S=op.S + 1) == 1 and rc(nblocks=op.nblocks + 1) == 1 and rc(pw=op.n) == 1
    assert rc(op=2) == 1 and rc(iters=0) == 1 and rc(iters=65) == 1 and rc(work=0) == 1 and rc(block=0) == 1
    assert rc(partials=0) == 1 and rc(tau=float("nan")) == 1 and rc(op=0, tol=-1.0) == 1
    torch.cuda.synchronize()
