"""Consistent thermal diffusion (models/diffusion.py::ConsistentDiffusion and its
PyTorch twin, ops/heat.py): convergence against the decaying harmonics,
conservation, the constant field, decomposition independence, the time-step
bound, the Lima flag's undershoot, configuration and the driver.  Every figure is
printed before it is asserted."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import rough_states as rs
from stsphere import driver as S
from stsphere.engine import Engine, VirtualCluster
from stsphere.models import diffusion as mh
from stsphere.models import initial_conditions as ic
from stsphere.models.diffusion import ConsistentDiffusion, Diffusion
from stsphere.ops import heat
from stsphere.parallel.layout import TileLayout
from stsphere.utils.history import read_history

DEGREE = {"harmonic": 4, "harmonic32": 3}


def _engine(N, t=1, case="lima_flag", cls=ConsistentDiffusion, integrator="ssprk3", **kw):
    return Engine(cls(case=case), TileLayout(N, t, 1, ng=2), grid=rs.grid_of(N), integrator=integrator, **kw)


def _cluster(N, t, nd, integrator="ssprk3", case="lima_flag"):
    return VirtualCluster(lambda: ConsistentDiffusion(case=case), TileLayout(N, t, nd, ng=2), grid=rs.grid_of(N),
                          integrator=integrator)


@functools.lru_cache(maxsize=None)
def _rough(N):
    """The ``scalar`` rough state [1, 6, N, N] on the Lima flag's scale."""
    return rs.make_state(_engine(N), "scalar")


# ---- 1., 2. convergence and conservation ---------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _decay_run(cls, case, N):
    """SSP-RK3 at the default cfl to t_end = 0.25 R^2 / (kappa l (l + 1)), dt shortened to
    land on it: (linf error / max |T(0)|, |sum(T A) - sum(T0 A)| / sum(|T0| A))."""
    e = _engine(N, case=case, cls=cls)
    g, ph, l = e.grid, e.physics, DEGREE[case]
    t_end = 0.25 * g.radius ** 2 / (ph.kappa * l * (l + 1))
    ns = int(math.ceil(t_end / e.dt))
    e.dt = t_end / ns
    T0 = rs.global_of(e)[0].numpy().copy()
    e.step(ns)
    T, A = rs.global_of(e)[0].numpy(), g.areas()
    err = np.abs(T - ph.exact(g, e.time)).max() / np.abs(T0).max()
    return float(err), float(abs((T * A).sum() - (T0 * A).sum()) / (np.abs(T0) * A).sum())


@pytest.mark.parametrize("case", ["harmonic", "harmonic32"])
def test_consistent_operator_converges(case):
    e24, m24 = _decay_run(ConsistentDiffusion, case, 24)
    e48, m48 = _decay_run(ConsistentDiffusion, case, 48)
    print(f"{case}: linf error / max |T0| C24 {e24:.3e} C48 {e48:.3e}, ratio {e24 / e48:.2f}; "
          f"conservation C24 {m24:.1e} C48 {m48:.1e}")
    assert e24 / e48 >= 3.0 and e48 <= 1e-3
    assert m24 <= 1e-14 and m48 <= 1e-14


def test_two_point_operator_does_not_converge():
    """Why the consistent operator exists; fails if the default is ever changed silently."""
    e24, _ = _decay_run(Diffusion, "harmonic", 24)
    e48, _ = _decay_run(Diffusion, "harmonic", 48)
    print(f"two_point harmonic: linf error / max |T0| C24 {e24:.4f} C48 {e48:.4f}")
    assert e48 >= e24 >= 0.03


# ---- 3. constant field ---------------------------------------------------------------------------

def test_constant_field_stays_constant():
    e = _engine(12, t=2)
    e.set_state(torch.full((1, e.plan.T, e.plan.n, e.plan.n), 287.0, dtype=torch.float64))
    e.step(10)
    dev = float((e.tiles_view() - 287.0).abs().max()) / 287.0
    print(f"constant field, 10 steps: relative deviation {dev:.2e}")
    assert dev <= 1e-13


# ---- 4. decomposition independence ---------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _one_rank_5_steps(integ, t):
    e = _engine(24, t=t, integrator=integ)
    rs.install(e, _rough(24))
    e.step(5)
    return rs.global_of(e).numpy()


@pytest.mark.parametrize("integ", ["ssprk3", "rk4"])
def test_tiling_independent(integ):
    a, b = _one_rank_5_steps(integ, 1), _one_rank_5_steps(integ, 2)
    print(f"{integ}: t = 1 against t = 2 after 5 steps, max difference {np.abs(a - b).max():.1e}")
    assert np.array_equal(a, b) and not np.array_equal(a, _rough(24).numpy())


@pytest.mark.parametrize("nd", [2, 8])
@pytest.mark.parametrize("integ", ["ssprk3", "rk4"])
def test_virtual_ranks_equal_one_rank(integ, nd):
    vc = _cluster(24, 2, nd, integ)
    for e in vc.engines:
        rs.install(e, _rough(24))
    vc.step(5)
    a, b = _one_rank_5_steps(integ, 2), rs.global_of(vc.engines).numpy()
    print(f"{integ}: {nd} virtual ranks against one after 5 steps, max difference {np.abs(a - b).max():.1e}")
    assert np.array_equal(a, b)
    for e in vc.engines:                       # the same-rank ghost slots equal their source cells
        q = e.state.clone()
        e.refresh_halos(q)
        assert torch.equal(q, e.state)


# ---- 5. max_dt -----------------------------------------------------------------------------------

def test_max_dt_is_the_global_bound():
    N, ph = 16, ConsistentDiffusion()
    grid = rs.grid_of(N)
    lams = []
    for t in (1, 2, 4):
        vc = _cluster(N, t, 6)
        lam = max(e.compute.op.lam_local for e in vc.engines)
        dts = {e.dt for e in vc.engines}
        print(f"C{N} t = {t}: lam {lam:.6e}, dt {sorted(dts)}")
        lams.append(lam)
        assert dts == {ph.max_dt(grid)}
    assert lams[0] == lams[1] == lams[2] == ph.lam(grid)
    assert ph.max_dt(grid) == 0.8 / (2.0 * ph.kappa * lams[0])
    assert ph.max_dt(grid, 0.4) == 0.4 / (2.0 * ph.kappa * lams[0])


@pytest.mark.parametrize("integ", ["euler", "ssprk2", "ssprk3", "rk4"])
def test_stable_at_the_default_cfl(integ):
    e = _engine(16, integrator=integ)
    rs.install(e, _rough(16))
    m0 = float(e.tiles_view().abs().max())
    e.step(200)
    m1 = float(e.tiles_view().abs().max())
    print(f"{integ} C16 rough state, 200 steps at cfl 0.8: max |T| {m0:.4f} -> {m1:.4f}")
    assert math.isfinite(m1) and m1 <= m0


# ---- 6. Lima flag: not monotone, but nearly -------------------------------------------------------

def test_lima_flag_undershoot_is_small():
    e = _engine(16, integrator="rk4")
    lo, hi = float(e.tiles_view().min()), float(e.tiles_view().max())
    worst = 0.0
    for _ in range(100):
        e.step()
        worst = max(worst, lo - float(e.tiles_view().min()))
    print(f"Lima flag C16, 100 RK4 steps: initial range [{lo}, {hi}], undershoot {worst:.4f} = "
          f"{worst / (hi - lo):.2e} of the range")
    assert worst <= 1e-3 * (hi - lo)


# ---- 7. solver ----------------------------------------------------------------------------------

def _cfg(out, nd=1, t=1, N=12, case="harmonic", operator="consistent", model="diffusion", nsteps=6, dt=None, **io):
    c = {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
         "grid": {"N": N}, "physics": {"model": model, "case": case},
         "time": {"nsteps": nsteps, "dt": dt}, "io": dict({"output_dir": str(out)}, **io)}
    if operator is not None:
        c["physics"]["operator"] = operator
    return c


def test_solver_virtual_ranks_equal_one_rank(tmp_path):
    a = S.Solver(_cfg(tmp_path / "a", nd=6, t=2), verbose=False)
    b = S.Solver(_cfg(tmp_path / "b"), verbose=False)
    sa, sb = a.run(), b.run()
    assert isinstance(a.physics, ConsistentDiffusion) and isinstance(a.engines[0].compute, heat.ConsistentCompute)
    assert np.array_equal(a.gather_global(), b.gather_global()) and a.step_count == 6
    assert sa["runtime"] == "eager" and sa["err_linf"] == sb["err_linf"] and "mass" in sa
    assert not np.array_equal(a.gather_global()[0], ic.harmonic_decay("harmonic", a.grid.centers(), 0.0, 2.0e6))


def test_solver_error_norms_fall(tmp_path):
    norms = {}
    for N in (12, 24):
        ph, g = ConsistentDiffusion(case="harmonic"), rs.grid_of(N)
        t_end = 0.25 * g.radius ** 2 / (ph.kappa * 20)
        ns = int(math.ceil(t_end / ph.max_dt(g)))
        s = S.Solver(_cfg(tmp_path / str(N), N=N, nsteps=ns, dt=t_end / ns), verbose=False)
        s.run()
        norms[N] = s.error_norms()
        print(f"C{N} harmonic, {ns} steps: {norms[N]}")
        assert norms[N] is not None and abs(s.time - t_end) < 1e-9 * t_end
    assert all(norms[24][k] < norms[12][k] for k in ("l1", "l2", "linf"))
    s = S.Solver(_cfg(tmp_path / "flag", case="lima_flag"), verbose=False)
    s.initialize()
    assert s.error_norms() is None


def test_solver_checkpoint_resume_and_history(tmp_path):
    a = S.Solver(_cfg(tmp_path / "a", history_interval=3), verbose=False)
    a.run()
    h = read_history(str(tmp_path / "a" / "history.zarr"), "T")
    assert h.shape == (3, 6, 12, 12) and np.array_equal(h[-1], a.global_field("T"))
    assert not np.array_equal(h[0], h[1])
    b = S.Solver(_cfg(tmp_path / "b", nsteps=3, checkpoint_interval=3), verbose=False)
    b.run()
    c = S.Solver(_cfg(tmp_path / "b", nsteps=3, restore="latest"), verbose=False)
    c.initialize()
    assert c.step_count == 3
    c.run()
    assert c.step_count == 6 and np.array_equal(c.gather_global(), a.gather_global())


def test_explicit_two_point_is_the_default(tmp_path):
    a = S.Solver(_cfg(tmp_path / "a", operator="two_point"), verbose=False)
    b = S.Solver(_cfg(tmp_path / "b", operator=None), verbose=False)
    a.run()
    b.run()
    assert type(a.physics) is Diffusion and type(b.physics) is Diffusion and a.physics.kernel_id == 1
    assert type(a.engines[0].compute).__name__ == "TorchCompute"
    assert np.array_equal(a.gather_global(), b.gather_global())
    c = S.Solver(_cfg(tmp_path / "c"), verbose=False)
    c.run()
    assert not np.array_equal(a.gather_global(), c.gather_global())


def _twin_laplacian(e):
    """L of a one-rank engine's state, by the twin's two passes."""
    op = heat.HeatOperator(e)
    assert not op.hip
    mh.heat_gradient_pass(e.state, None, e.gmap, op.tabs, op.T, op.n, op.ng, op.scratch)
    return mh.heat_flux_pass(op.scratch, None, e.gmap, op.tabs, op.T, op.n, op.ng)


def test_solver_laplacian(tmp_path):
    s = S.Solver(_cfg(tmp_path / "a", nd=6, t=2), verbose=False)
    s.initialize()
    one = S.Solver(_cfg(tmp_path / "b"), verbose=False)
    one.initialize()
    L = s.laplacian("T")
    assert L.shape == (6, 12, 12) and np.isfinite(L).all()
    assert np.array_equal(L, one.laplacian("T"))
    e = one.engines[0]
    assert np.array_equal(one.laplacian("T"), _twin_laplacian(e).numpy())
    # the two-point diffusion and the advection model: their prognostic field, same operator
    for kw, name in ((dict(operator=None), "T"), (dict(operator=None, model="advection", case="cosine_bell"), "q")):
        p = S.Solver(_cfg(tmp_path / "c", **kw), verbose=False)
        p.initialize()
        assert np.array_equal(p.laplacian(name), _twin_laplacian(p.engines[0]).numpy())
        with pytest.raises(ValueError, match="unknown laplacian field"):
            p.laplacian("h")
        with pytest.raises(ValueError):                      # physics.dissipation stays shallow water only
            p.dissipate()


def test_the_twin_shares_the_dissipation_arithmetic():
    """Row 0 of the dissipation's Laplacian of the same scalar: the same bits."""
    e = _engine(12, t=2)
    x = rs.local_of(e, _rough(12))
    e.set_state(x)
    from stsphere.models.swe import ShallowWater
    d = Engine(ShallowWater("tc2"), TileLayout(12, 2, 1, ng=2), grid=rs.grid_of(12)).dissipation()
    assert torch.equal(e.heat_operator().laplacian(), d.laplacian(x)[0])


@pytest.mark.parametrize("phys,match", [
    ({"model": "swe", "case": "tc2", "operator": "consistent"}, "physics.operator"),
    ({"model": "advection", "case": "cosine_bell", "operator": "consistent"}, "physics.operator"),
    ({"model": "diffusion", "operator": "five_point"}, "physics.operator"),
])
def test_config_rejections(tmp_path, phys, match):
    c = _cfg(tmp_path)
    c["physics"] = phys
    with pytest.raises(ValueError, match=match):
        S.Solver(c, verbose=False).initialize()


def test_spmd_is_refused(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "6")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="spmd"):
        S.Solver(_cfg(tmp_path, nd=6), verbose=False).initialize()


def test_rhs_is_refused_and_torch_compute_is_not_used():
    e = _engine(8)
    assert isinstance(e.compute, heat.ConsistentCompute) and e.physics.two_pass
    with pytest.raises(NotImplementedError):
        e.physics.rhs(None, None, e.tens, 8, 1)


def test_shipped_configs():
    from stsphere.utils.config import load_config
    here = os.path.join(os.path.dirname(S.__file__), "configs")
    a = load_config(os.path.join(here, "lima_flag_consistent.yaml"))
    b = load_config(os.path.join(here, "lima_flag_diffusion.yaml"))
    assert a.physics.operator == "consistent" and b.physics.operator == "two_point"
    assert (a.grid.N, a.physics.case, a.physics.kappa, a.time.days) == (b.grid.N, b.physics.case, b.physics.kappa,
                                                                        b.time.days)
    h = load_config(os.path.join(here, "heat_harmonic.yaml"))
    assert (h.grid.N, h.physics.case, h.physics.operator, h.parallelization.num_devices) == (48, "harmonic32",
                                                                                             "consistent", 1)
    assert isinstance(S.make_physics(h.physics), ConsistentDiffusion)
    # kappa: 2.0e6 reaches the model as a number (YAML reads it as a string), in the two-point config too
    assert [S.make_physics(c.physics).kappa for c in (a, b, h)] == [2.0e6] * 3
    b.physics.kappa = "warm"
    with pytest.raises(ValueError, match="physics.kappa"):
        S.make_physics(b.physics)
