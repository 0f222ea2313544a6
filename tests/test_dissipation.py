"""Scale-selective dissipation (models/dissipation.py, ops/dissipation.py, the
PyTorch twin): accuracy and spectrum of the consistent Laplacian, conservation,
fixed points, decomposition independence, order 2 and sub-steps, the Galewsky
jet, configuration and the driver."""
import functools
import math

import numpy as np
import pytest
import torch

import rough_states as rs
from stsphere import driver as S
from stsphere.engine import Engine, VirtualCluster
from stsphere.models import dissipation as md
from stsphere.models import initial_conditions as ic
from stsphere.models.geometry import EARTH_RADIUS, GRAVITY, OMEGA
from stsphere.models.swe import ShallowWater
from stsphere.ops.dissipation import apply_all, laplacian_all
from stsphere.parallel.layout import TileLayout


def _engine(N, t=1, case="tc5", dtype=torch.float64):
    return Engine(ShallowWater(case), TileLayout(N, t, 1, ng=2), grid=rs.grid_of(N), dtype=dtype)


def _cluster(N, t, nd, case="tc5"):
    return VirtualCluster(lambda: ShallowWater(case), TileLayout(N, t, nd, ng=2), grid=rs.grid_of(N))


def _global(engines, tiles):
    from stsphere.engine import assemble_global
    return assemble_global(engines[0].layout, {e.rank: x.detach().cpu().numpy() for e, x in zip(engines, tiles)})


@functools.lru_cache(maxsize=None)
def _l4_errors(N):
    """(border max error / max value, interior max error / max value) of L on
    35 z^4 - 30 z^2 + 3 against -20 / R^2 times it."""
    e = _engine(N)
    z = torch.as_tensor(e.geo.center[..., 2])
    f = 35 * z ** 4 - 30 * z ** 2 + 3
    exact = -20.0 / EARTH_RADIUS ** 2 * f
    err = (e.dissipation().laplacian(f[None])[0] - exact).abs() / exact.abs().max()
    j, i = np.mgrid[0:N, 0:N]
    dist = torch.as_tensor(np.minimum(np.minimum(i, N - 1 - i), np.minimum(j, N - 1 - j)))
    return float(err[:, dist == 0].max()), float(err[:, dist >= 2].max())


# ---- 1. accuracy -------------------------------------------------------------------------------

def test_accuracy_against_the_analytic_eigenvalue():
    b24, i24 = _l4_errors(24)
    b48, i48 = _l4_errors(48)
    print(f"l = 4: border C24 {b24:.4f} C48 {b48:.4f}; interior C24 {i24:.3e} C48 {i48:.3e}, ratio {i24 / i48:.2f}")
    assert b24 <= 0.08 and b48 <= 0.08
    assert i24 / i48 >= 3.5


# ---- 2. spectrum -------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _dense(N=8):
    e = _engine(N, case="rest")
    d = e.dissipation()
    cells = 6 * N * N
    M = np.zeros((cells, cells))
    for k0 in range(0, cells, 4):      # four unit vectors per application
        x = torch.zeros((4, cells), dtype=torch.float64)
        for c in range(4):
            x[c, k0 + c] = 1.0
        M[:, k0:k0 + 4] = d.laplacian(x.reshape(4, 6, N, N)).reshape(4, cells).numpy().T
    return M, d.lam, e.geo.area.reshape(-1)


def test_spectrum_at_c8():
    M, lam, _ = _dense()
    ev = np.linalg.eigvals(M)
    print(f"C8: max Re lambda / Lam {ev.real.max() / lam:.3e}, max |lambda| / Lam {np.abs(ev).max() / lam:.4f}")
    assert ev.real.max() <= 1e-9 * lam
    assert np.abs(ev).max() <= 2.0 * lam


# ---- 3. conservation ----------------------------------------------------------------------------

def _rough(e):
    return rs.make_state(e, "rough")


def test_flux_is_conservative_on_a_rough_field():
    e = _engine(24)
    q = rs.local_of(e, _rough(e))
    A = torch.as_tensor(e.geo.area)
    Lq = e.dissipation().laplacian(q)
    for c in range(4):
        assert abs(float((A * Lq[c]).sum())) <= 1e-13 * float((A * Lq[c].abs()).sum())


@pytest.mark.parametrize("order,nu", [(1, 1.0e5), (2, 1.0e15)])
def test_four_applications_conserve_mass(order, nu):
    e = _engine(24)
    rs.install(e, _rough(e))
    A = torch.as_tensor(e.geo.area)
    m0 = float((e.tiles_view()[0] * A).sum())
    d = e.dissipation(order, nu)
    q0 = e.tiles_view().clone()
    for _ in range(4):
        d.apply(600.0)
    assert not torch.equal(q0, e.tiles_view())
    assert abs(float((e.tiles_view()[0] * A).sum()) - m0) < 1e-13 * m0


# ---- 4. fixed points ----------------------------------------------------------------------------

def test_lake_at_rest_over_the_mountain_is_a_fixed_point():
    e = _engine(24)
    b = e.tens["b"]
    assert float(b.max()) > 1000.0
    q = torch.zeros((4,) + tuple(b.shape), dtype=torch.float64)
    q[0] = 5960.0 - b
    e.set_state(q)
    for order, nu in ((1, 1.0e5), (2, 1.0e15)):
        e.set_state(q)
        e.dissipation(order, nu).apply(600.0)
        out = e.tiles_view()
        assert float((out[0] - q[0]).abs().max()) <= 1e-12 * float(q[0].max())
        assert bool((out[1:4] == 0).all())


def test_laplacian_of_a_constant():
    e = _engine(24)
    d = e.dissipation()
    x = torch.full((1, 6, 24, 24), 7.5, dtype=torch.float64)
    assert float(d.laplacian(x).abs().max()) <= 1e-13 * d.lam * 7.5


# ---- 5. decomposition ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _applied(t, nd, order):
    """Global state after one application on the rough state, any layout."""
    if nd == 1:
        engines = [_engine(24, t)]
    else:
        engines = _cluster(24, t, nd).engines
    G = rs.swe_state(rs.global_of(engines), engines[0].grid.centers(), "rough")
    for e in engines:
        rs.install(e, G)
    nu = 1.0e5 if order == 1 else 1.0e15
    apply_all([e.dissipation(order, nu) for e in engines], 900.0)
    return rs.global_of(engines)


@pytest.mark.parametrize("order", [1, 2])
def test_tilings_and_virtual_ranks_are_bitwise_equal(order):
    ref = _applied(1, 1, order)
    assert torch.equal(_applied(2, 1, order), ref)
    assert torch.equal(_applied(4, 1, order), ref)
    assert torch.equal(_applied(2, 4, order), ref)


def test_laplacian_over_virtual_ranks():
    one = _engine(24, 2)
    G = _rough(one)
    ref = one.dissipation().laplacian(rs.local_of(one, G))
    vc = _cluster(24, 2, 4)
    ys = laplacian_all([e.dissipation() for e in vc.engines], [rs.local_of(e, G) for e in vc.engines])
    for c in range(4):
        assert np.array_equal(_global(vc.engines, [y[c] for y in ys]), _global([one], [ref[c]]))


# ---- 6. order 2 and sub-steps -------------------------------------------------------------------

def test_order_two_is_minus_l_of_l():
    e = _engine(24, case="tc2")                 # no topography: the inner field is L of (h, v) itself
    rs.install(e, _rough(e))
    q0 = e.tiles_view().clone()
    d = e.dissipation(2, 1.0e15)
    w = md.primitives(q0)
    inner = d.laplacian(w)
    LL = d.laplacian(inner)
    tau = 300.0
    assert d.substeps(tau) == 1
    d.apply(tau)
    want = q0.clone()
    md.update(want, LL, -tau * d.nu, d.tabs, True)
    assert torch.equal(e.tiles_view(), want)


def test_substep_rule_and_limit():
    e = _engine(12)
    lam = e.dissipation().lam
    tau = 1000.0
    # order 1: m = ceil(2 tau nu lam); 2 tau nu lam = 2.5 needs 3
    d = e.dissipation(1, 2.5 / (2.0 * tau * lam))
    assert d.substeps(tau) == 3
    assert e.dissipation(1, 0.99 / (2.0 * tau * lam)).substeps(tau) == 1
    d2 = e.dissipation(2, 2.5 / (tau * (2.0 * lam) ** 2))
    assert d2.substeps(tau) == 3
    # three sub-steps are three applications of tau / 3
    G = _rough(e)
    rs.install(e, G)
    assert d.apply(tau) == 3
    got = e.tiles_view().clone()
    rs.install(e, G)
    one = e.dissipation(1, d.nu / 3.0)          # same tau nu / 3 per application, m = 1
    for _ in range(3):
        assert one.apply(tau) == 1
    assert torch.allclose(e.tiles_view(), got, rtol=1e-13, atol=0)
    with pytest.raises(ValueError, match="largest admissible nu"):
        e.dissipation(1, 65.0 / (2.0 * tau * lam)).apply(tau)
    assert e.dissipation(1, 63.9 / (2.0 * tau * lam)).substeps(tau) == 64


# ---- 7. Galewsky --------------------------------------------------------------------------------

def test_galewsky_balance_depth_and_perturbation():
    a, g = EARTH_RADIUS, GRAVITY
    p0, p1 = ic.GALEWSKY_PHI0, ic.GALEWSKY_PHI1
    phi = np.linspace(p0, p1, 202)[1:-1]                     # 200 latitudes inside the jet
    u = ic.galewsky_wind(phi)
    assert abs(u.max() - 80.0) < 0.05 and ic.galewsky_wind(np.array([p0, p1, 0.0, 1.5])).max() == 0.0
    # gradient-wind balance by central differences of the host depth function.  With step d the
    # difference quotient errs by d^2 / 6 |h'''| + eps h / d.  h' = -(a / g) u (f + u tan / a) <=
    # 6.4e6 / 9.8 * 80 * 2.6e-4 ~ 1.4e4 m / rad and every derivative of the jet profile brings a
    # factor <= ~60 / rad (the width of its flanks), so |h'''| <= 1.4e4 * 60^2 ~ 5e7: at d = 1e-5
    # the truncation is <= 1e-3 and the rounding 1e-16 * 1e4 / 1e-5 = 1e-7 m / rad.  (g / a) times
    # that is 1.6e-9 m / s^2 against terms of 80 * 1.5e-4 = 1.2e-2: tolerance 1e-8 m / s^2.
    d = 1.0e-5
    dh = (ic.galewsky_depth(phi + d) - ic.galewsky_depth(phi - d)) / (2.0 * d)
    res = 2.0 * OMEGA * np.sin(phi) * u + u * u * np.tan(phi) / a + (g / a) * dh
    print(f"galewsky: max balance residual {np.abs(res).max():.3e} m/s^2")
    assert np.abs(res).max() <= 1.0e-8
    # quadrature: four times the nodes
    lat = np.linspace(-0.5 * math.pi, 0.5 * math.pi, 721)
    h = ic.galewsky_depth(lat)
    assert np.abs(h - ic.galewsky_depth(lat, nodes=4 * ic.GALEWSKY_NODES)).max() <= 1.0e-6
    # global mean depth 1/2 int h cos, by Gauss-Legendre on the three pieces (h is constant on the outer two)
    mean = 0.0
    jet = np.linspace(p0, p1, 129)
    pieces = [(-0.5 * math.pi, p0, 8), (p1, 0.5 * math.pi, 8)] + [(lo, hi, 32) for lo, hi in zip(jet[:-1], jet[1:])]
    for lo, hi, n in pieces:
        x, w = np.polynomial.legendre.leggauss(n)
        y = 0.5 * (hi + lo) + 0.5 * (hi - lo) * x
        mean += 0.5 * 0.5 * (hi - lo) * float((w * ic.galewsky_depth(y) * np.cos(y)).sum())
    assert abs(mean - 10000.0) <= 1.0e-6
    # the perturbation: 120 cos(pi / 4) at (0, pi / 4), the centre of both Gaussians.  The factor
    # cos(phi) moves the maximum south by d = tan(pi / 4) / (2 * 15^2) = 2.2e-3 rad and raises it by
    # the factor 1 + d / 2 = 1.0011 (first order in d); lambda = 0 stays the maximum in longitude
    peak = 120.0 * math.cos(0.25 * math.pi)
    assert abs(float(ic.galewsky_perturbation(0.0, 0.25 * math.pi)) - peak) < 1e-12
    lon, la = np.meshgrid(np.linspace(-math.pi, math.pi, 721), np.linspace(0.0, 0.5 * math.pi, 3601))
    pert = ic.galewsky_perturbation(lon, la)
    k = np.unravel_index(pert.argmax(), pert.shape)
    assert peak <= pert.max() <= 1.0012 * peak
    assert abs(lon[k]) < 1e-12 and 0.0 <= 0.25 * math.pi - la[k] < 3.0e-3
    assert np.allclose(ic.galewsky_perturbation(lon + 2.0 * math.pi, la), pert, rtol=0, atol=1e-9)
    assert ic.galewsky_perturbation(math.pi - 1e-3, 0.25 * math.pi) < 1e-30      # lambda in (-pi, pi]: no seam


def test_galewsky_cases_of_the_model():
    grid = rs.grid_of(12)
    from stsphere.models.geometry import xyz_to_lonlat
    lon, lat = xyz_to_lonlat(grid.centers())
    hb, wb, bb = ShallowWater("galewsky_balanced").global_fields(grid)
    hp, wp, _ = ShallowWater("galewsky").global_fields(grid)
    # balanced: no dependence on longitude: equal to the depth function of the latitude alone
    assert np.array_equal(hb, ic.galewsky_depth(lat)) and not bb.any()
    assert np.array_equal(wb, wp) and np.array_equal(hp - hb, (hb + ic.galewsky_perturbation(lon, lat)) - hb)
    assert np.abs(hp - hb).max() > 10.0
    assert np.abs((wb * grid.centers()).sum(-1)).max() < 1e-12      # tangent wind


# ---- 8. config and driver ------------------------------------------------------------------------

def _cfg(out, diss=None, nd=1, t=1, tracers=None, case="galewsky", model="swe", **io):
    c = {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
         "grid": {"N": 12}, "physics": {"model": model, "case": case, "limiter": "mc"},
         "time": {"nsteps": 4, "dt": 300.0}, "io": dict({"output_dir": str(out)}, **io)}
    if diss is not None:
        c["physics"]["dissipation"] = diss
    if tracers is not None:
        c["physics"]["tracers"] = tracers
    return c


@pytest.mark.parametrize("diss,kw,match", [
    ({"order": 1, "nu": 1e5, "strength": 2}, {}, "unknown key"),
    ({"order": 3, "nu": 1e5}, {}, "order"),
    ({"nu": 1e5}, {}, "order"),
    ({"order": 1, "nu": 0.0}, {}, "nu"),
    ({"order": 1, "nu": -1.0}, {}, "nu"),
    ({"order": 1, "nu": 1e5, "interval": 0}, {}, "interval"),
    ({"order": 1, "nu": 1e5}, {"model": "advection", "case": "cosine_bell"}, "shallow-water"),
    ({"order": 1, "nu": 1e5}, {"tracers": ["cap"], "case": "tc5"}, "depth: false"),
    ({"order": 1, "nu": 1e5, "depth": True}, {"tracers": ["cap"], "case": "tc5"}, "depth: false"),
    ({"order": 1, "nu": 1e5, "interval": 2}, {"checkpoint_interval": 3}, "checkpoint_interval"),
])
def test_config_rejections(tmp_path, diss, kw, match):
    with pytest.raises(ValueError, match=match):
        S.Solver(_cfg(tmp_path, diss, **kw), verbose=False).initialize()


def test_shipped_galewsky_config():
    """configs/c96_galewsky.yaml: six days, order 1, nu = 1e5 (which YAML reads as a string),
    vorticity in the history, a time step inside the model's own bound."""
    import os
    from stsphere.utils.config import load_config
    path = os.path.join(os.path.dirname(os.path.abspath(md.__file__)), "..", "configs", "c96_galewsky.yaml")
    c = load_config(path)
    assert S.dissipation_spec(c.physics) == {"order": 1, "nu": 1.0e5, "interval": 1, "depth": True}
    assert c.physics.case == "galewsky" and c.time.days == 6 and "vorticity" in c.io.history_fields
    assert c.io.checkpoint_interval % 1 == 0 and c.grid.N == 96
    assert c.time.dt <= ShallowWater("galewsky").max_dt(rs.grid_of(96))
    with pytest.raises(ValueError, match="nu"):
        S.dissipation_spec(load_config({"physics": {"dissipation": {"order": 1, "nu": "large"}}}).physics)


def test_spmd_is_refused(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "6")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(ValueError, match="spmd"):
        S.Solver(_cfg(tmp_path, {"order": 1, "nu": 1e5}, nd=6), verbose=False).initialize()


def test_run_without_the_key_is_unchanged(tmp_path):
    """No key: the driver steps exactly as an engine stepped by hand."""
    s = S.Solver(_cfg(tmp_path), verbose=False)
    s.run()
    e = _engine(12, case="galewsky")
    e.dt = 300.0
    e.step(4)
    assert np.array_equal(s.gather_global(), rs.global_of(e).numpy())
    with pytest.raises(ValueError, match="no dissipation"):
        s.dissipate()


@pytest.mark.parametrize("nd,t", [(1, 1), (6, 2)])
def test_run_equals_step_step_dissipate(tmp_path, nd, t):
    diss = {"order": 1, "nu": 1.0e5, "interval": 2}
    s = S.Solver(_cfg(tmp_path / "a", diss, nd=nd, t=t), verbose=False)
    s.run()
    h = S.Solver(_cfg(tmp_path / "b", nd=nd, t=t), verbose=False)
    h.initialize()
    for _ in range(2):                                # the operator by hand on a run without the key
        h.step(2)
        assert apply_all([e.dissipation(1, 1.0e5) for e in h.engines], 2 * 300.0) == 1
    assert np.array_equal(s.gather_global(), h.gather_global())
    plain = S.Solver(_cfg(tmp_path / "c", nd=nd, t=t), verbose=False)
    plain.run()
    assert not np.array_equal(s.gather_global(), plain.gather_global())
    s2 = S.Solver(_cfg(tmp_path / "d", diss, nd=nd, t=t), verbose=False)
    s2.initialize()
    with pytest.raises(ValueError, match="multiple"):
        s2.step(3)
    s2.step(4)
    assert np.array_equal(s2.gather_global(), s.gather_global())


def test_virtual_ranks_run_equals_one_rank(tmp_path):
    diss = {"order": 2, "nu": 1.0e15}
    a = S.Solver(_cfg(tmp_path / "a", diss, nd=1, t=2), verbose=False)
    b = S.Solver(_cfg(tmp_path / "b", diss, nd=6, t=2), verbose=False)
    a.run()
    b.run()
    assert np.array_equal(a.gather_global(), b.gather_global())


def test_tracers_without_depth_keep_h_and_hq(tmp_path):
    kw = dict(tracers=["cap", "gradient"], case="tc5")
    a = S.Solver(_cfg(tmp_path / "a", {"order": 1, "nu": 1.0e5, "depth": False}, **kw), verbose=False)
    a.initialize()
    b = S.Solver(_cfg(tmp_path / "b", **kw), verbose=False)
    b.initialize()
    a.dissipate()
    ga, gb = a.gather_global(), b.gather_global()
    assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[4:], gb[4:])
    assert not np.array_equal(ga[1:4], gb[1:4])


def test_solver_laplacian(tmp_path):
    s = S.Solver(_cfg(tmp_path, nd=6, t=2), verbose=False)
    s.initialize()
    one = S.Solver(_cfg(tmp_path, nd=1, t=1), verbose=False)
    one.initialize()
    for name in ("h", "vorticity", "u"):
        L = s.laplacian(name)
        assert L.shape == (6, 12, 12) and np.isfinite(L).all() and np.abs(L).max() > 0
        assert np.array_equal(L, one.laplacian(name))
    e = one.engines[0]
    assert np.array_equal(one.laplacian("h"), _global([e], [e.dissipation().laplacian(e.tiles_view()[0:1])[0]]))
    with pytest.raises(ValueError):
        s.laplacian("nope")
