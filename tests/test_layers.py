"""Two-layer (stacked, isopycnal) shallow water, the PyTorch twin on the CPU
(``models/swe.py::LayeredShallowWater``): one layer is the parent bit for bit,
the steady two-layer state converges at second order and conserves each layer's
mass, uniform layers stay at rest, the result does not depend on the
decomposition, and the plumbing from the config file to the Solver's products.

Bounds: the l2 depth error of the steady state must fall by a factor of at least
4 from C16 to C32 (second order; the prototype measured 5.6 and 5.5) and each
layer's mass may drift by 1e-12 relative (measured 1.5e-14)."""
import functools

import numpy as np
import pytest
import torch
import yaml

import stsphere as S
from stsphere.engine import Engine, VirtualCluster
from stsphere.models import initial_conditions as ic
from stsphere.models.base import extend
from stsphere.models.geometry import DAY, CubedSphereGrid, xyz_to_lonlat
from stsphere.models.swe import LayeredShallowWater, ShallowWater
from stsphere.parallel.layout import TileLayout
from stsphere.utils import checkpoint as ckpt
from stsphere.utils.history import read_history, read_metrics

from rough_states import global_of


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _engine(phys, N, t=1, **kw):
    return Engine(phys, TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=torch.float64, device="cpu", backend="torch",
                  **kw)


def _two(case="tc2", **kw):
    kw.setdefault("limiter", 2)
    if case == "tc2":
        kw.setdefault("depths", [4000.0, 4000.0])
        kw.setdefault("winds", [0.5, 0.4])
    else:
        kw.setdefault("depths", list(ic.LAYER_DEPTHS.get(case, (4000.0, 4000.0))))
    return LayeredShallowWater(case, density_ratio=0.9, **kw)


def test_one_layer_is_the_parent_bit_for_bit():
    a = _engine(LayeredShallowWater("tc2"), 12)
    b = _engine(ShallowWater("tc2"), 12)
    assert a.physics.kernel_id == 4 and a.physics.fields == ["h0", "mx0", "my0", "mz0"] and a.dt == b.dt
    a.step(3)
    b.step(3)
    assert torch.equal(a.tiles_view(), b.tiles_view())
    da, db = a.diagnostics(), b.diagnostics()
    assert da["energy"] == db["energy"] and da["mass0"] == db["mass"]


@functools.lru_cache(maxsize=None)
def _steady_day(N):
    """One day of the steady two-layer state at the default dt: per layer the
    l2 depth error against the initial state and the relative mass drift."""
    e = _engine(_two("tc2"), N)
    A = e.tens["area"]
    v0 = e.tiles_view().clone()
    e.step(int(np.ceil(DAY / e.dt)))
    v = e.tiles_view()
    l2 = [float(((((v[4 * k] - v0[4 * k]) ** 2) * A).sum() / ((v0[4 * k] ** 2) * A).sum()).sqrt()) for k in (0, 1)]
    drift = [abs(float(((v[4 * k] - v0[4 * k]) * A).sum() / (v0[4 * k] * A).sum())) for k in (0, 1)]
    return l2, drift


def test_steady_state_converges_at_second_order_and_conserves_mass():
    (c, dc), (f, df) = _steady_day(16), _steady_day(32)
    ratios = [c[k] / f[k] for k in (0, 1)]
    print(f"l2 depth error C16 {c[0]:.3e} / {c[1]:.3e}, C32 {f[0]:.3e} / {f[1]:.3e}, ratios "
          f"{ratios[0]:.2f} / {ratios[1]:.2f}; mass drift {max(dc + df):.2e}")
    assert min(ratios) >= 4.0
    assert max(dc + df) < 1e-12


def test_uniform_layers_stay_at_rest():
    """``rest`` at C12, ten steps: max |M_k| at most ten times the parent's
    single-layer figure after the same steps, with a floor of 1e-13 H sqrt(g H)
    (H = 1000 m, the depth of a layer and of the parent's lake); the coupling
    gradient alone is exactly zero."""
    a = _engine(_two("rest"), 12)
    b = _engine(ShallowWater("rest"), 12, dt=a.dt)
    p = a.plan
    qe = extend(a.state, None, a.gmap, p.T, p.n, 2, cmap=a.cmap)
    gc = a.physics.coupling_gradients(qe, a.tiles_view(), a.tens, p.n, 2)
    assert gc.shape == (2, 3, p.T, p.n, p.n) and float(gc.abs().max()) == 0.0
    a.step(10)
    b.step(10)
    va = a.tiles_view()
    mp = float(b.tiles_view()[1:4].abs().max())
    H = 1000.0
    bound = max(10.0 * mp, 1e-13 * H * (a.physics.g * H) ** 0.5)
    m = [float(va[4 * k + 1:4 * k + 4].abs().max()) for k in (0, 1)]
    print(f"rest: max |M| layers {m[0]:.3e} / {m[1]:.3e}, parent {mp:.3e}, bound {bound:.3e}")
    assert max(m) <= bound
    # and the gradient is not zero by construction: a tilted interface gives one
    c = _engine(_two("tc5"), 12)
    qe = extend(c.state, None, c.gmap, c.plan.T, c.plan.n, 2, cmap=c.cmap)
    assert float(c.physics.coupling_gradients(qe, c.tiles_view(), c.tens, c.plan.n, 2).abs().max()) > 0


def test_decomposition_independent():
    """t = 1, t = 2 and 4 virtual ranks after five steps at C12: bit-identical,
    as the parent's and the tracers' decomposition tests assert for the torch
    path (the panel-edge pairs are chosen on the whole edge)."""
    N = 12
    mk = lambda: _two("tc5")   # noqa: E731
    a = _engine(mk(), N, 1)
    b = _engine(mk(), N, 2, dt=a.dt)
    vc = VirtualCluster(mk, TileLayout(N, 2, 4, ng=2), grid=_grid(N), dtype=torch.float64, device="cpu",
                        backend="torch", dt=a.dt)
    for x in (a, b, vc):
        x.step(5)
    ga = global_of(a)
    assert torch.equal(ga, global_of(b))
    assert torch.equal(ga, global_of(vc.engines))


def test_layered_jet():
    """Thicknesses positive, bottom layer at rest, the balanced state zonally
    symmetric (and the perturbed one not), the ranges computed at C32, and 20
    steps at C24 stay finite."""
    p = _grid(32).centers()
    lon, lat = xyz_to_lonlat(p)
    hb, wb, b = ic.layered_fields("layered_jet_balanced", p)
    h, w, _ = ic.layered_fields("layered_jet", p)
    assert h.min() > 0 and hb.min() > 0 and not b.any()
    assert not w[1].any() and not wb[1].any()
    assert 2800 < h[0].min() < 2850 and 5350 < h[0].max() < 5400 and 4650 < h[1].min() < 4700 \
        and 6940 < h[1].max() < 6980
    assert 19.9 < np.linalg.norm(w[0], axis=-1).max() <= 20.0
    # r h_0 + h_1 is constant where the bottom layer rests
    assert np.ptp(0.9 * hb[0] + hb[1]) < 1e-9 * 9500
    # zonal symmetry: the balanced depths are a function of the latitude alone
    order = np.argsort(lat.ravel())
    for k in (0, 1):
        x = hb[k].ravel()[order]
        same = np.abs(np.diff(lat.ravel()[order])) < 1e-12
        assert np.abs(np.diff(x))[same].max() < 1e-8
    # the bump peaks at 120 cos(pi / 4) = 85 m; a C32 cell centre lies within half a cell
    # (0.025 rad) of the peak in each direction: at least 85 exp(-(0.025 * 15)^2 - (0.025 * 3)^2) = 73 m
    assert 73 < np.abs(h[0] - hb[0]).max() < 85 and np.array_equal(h[1], hb[1])
    e = _engine(_two("layered_jet"), 24)
    e.step(20)
    v = e.tiles_view()
    assert bool(torch.isfinite(v).all()) and float(v[0].min()) > 0 and float(v[4].min()) > 0


def test_tc2_and_tc5_states():
    """tc2: the two pressure relations of the steady state; exact() returns the
    initial depths.  tc5: h_0 = H_0 and the mountain under the bottom layer."""
    g = _grid(12)
    ph = _two("tc2")
    h, w, b = ph.global_fields(g)
    u0 = 2.0 * np.pi * g.radius / (12.0 * DAY)
    lon, lat = xyz_to_lonlat(g.centers())
    s2 = np.sin(lat) ** 2
    A = [g.radius * ph.omega * f * u0 + 0.5 * (f * u0) ** 2 for f in (0.5, 0.4)]
    assert np.allclose(h[0] + h[1], 8000.0 - A[0] * s2 / ph.g, rtol=1e-13)
    assert np.allclose(0.9 * h[0] + h[1], 0.9 * 4000.0 + 4000.0 - A[1] * s2 / ph.g, rtol=1e-13)
    assert np.array_equal(ph.exact(g, 3600.0), h) and h.shape == (2, 6, 12, 12)
    h5, w5, b5 = _two("tc5").global_fields(g)
    assert np.all(h5[0] == 2000.0) and b5.max() > 1000 and np.array_equal(w5[0], w5[1])
    assert _two("layered_jet").exact(g, 0.0) is None


def test_diagnostics_masses_and_energy():
    e = _engine(_two("tc5"), 12)
    v, A, b = e.tiles_view(), e.tens["area"], e.tens["b"]
    d = e.diagnostics()
    assert d["mass0"] == pytest.approx(float((v[0] * A).sum())) and d["mass1"] == pytest.approx(float((v[4] * A).sum()))
    gr = e.physics.g
    en = 0.9 * (0.5 * (v[1:4] ** 2).sum(0) / v[0] + gr * v[0] * (b + v[4] + 0.5 * v[0])) \
        + (0.5 * (v[5:8] ** 2).sum(0) / v[4] + gr * v[4] * (b + 0.5 * v[4]))
    assert d["energy"] == pytest.approx(float((en * A).sum()), rel=1e-14)


# ---- refusals ---------------------------------------------------------------------
def _cfg(out, layers=True, nd=1, t=1, case="tc2", **io):
    c = {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
         "grid": {"N": 12}, "physics": {"model": "swe", "case": case, "limiter": "mc"},
         "time": {"nsteps": 6, "dt": 400.0}, "io": dict({"output_dir": str(out)}, **io)}
    if layers:
        c["physics"]["layers"] = {"depths": [4000.0, 4000.0], "density_ratio": 0.9, "winds": [0.5, 0.4]}
    return c


def test_refuses_fused_streaming_and_march3():
    from stsphere.ops.fused import fused_supported_config
    from stsphere.ops.hip_compute import march_supported
    from stsphere.ops.march3 import march3_unsupported
    L = TileLayout(48, 1, 1, ng=2)
    assert fused_supported_config(ShallowWater("tc5"), "ssprk3", L) is None
    assert fused_supported_config(_two("tc5"), "ssprk3", L) == "fused step: no layers"
    assert march_supported(2, 2, False) and not march_supported(4, 2, False)

    class _Compute:
        phys_id = 4

    class _E:
        backend = "hip"
        compute = _Compute()
    assert march3_unsupported(_E()) is not None


def test_refuses_the_direct_xgmi_exchange():
    from stsphere.ops.xgmi import XgmiHalo
    with pytest.raises(RuntimeError, match="1 or 4 fields"):
        XgmiHalo(_engine(_two("tc5"), 12))
    c = _cfg("x")
    c["runtime"] = {"comm": "xgmi"}
    with pytest.raises(ValueError, match="xgmi with physics.layers"):
        S.Solver(c, verbose=False).initialize()


def test_refuses_tracers_with_layers():
    c = _cfg("x")
    c["physics"]["tracers"] = ["cap"]
    with pytest.raises(ValueError, match="physics.layers with physics.tracers"):
        S.Solver(c, verbose=False).initialize()


def test_refuses_dissipation_with_layers():
    c = _cfg("x")
    c["physics"]["dissipation"] = {"order": 1, "nu": 1.0e5}
    with pytest.raises(ValueError, match="physics.dissipation with physics.layers"):
        S.Solver(c, verbose=False).initialize()


def test_refuses_particles_on_a_layered_run(tmp_path):
    s = S.Solver(_cfg(tmp_path), verbose=False)
    s.initialize()
    with pytest.raises(ValueError, match="particles on a layered run"):
        s.add_particles(np.array([0.1]), np.array([0.2]))
    c = _cfg(tmp_path / "b")
    c["io"]["particles"] = {"count": 4}
    with pytest.raises(ValueError, match="particles on a layered run"):
        S.Solver(c, verbose=False).initialize()


def test_refuses_ppm():
    with pytest.raises(ValueError, match="PPM"):
        _two("tc2", limiter=4)
    c = _cfg("x")
    c["physics"]["limiter"] = "ppm"
    with pytest.raises(ValueError, match="PPM"):
        S.Solver(c, verbose=False).initialize()


def test_refuses_other_cases_and_bad_parameters():
    with pytest.raises(ValueError, match="unknown layered shallow-water case"):
        _two("tc6", depths=[4000.0, 4000.0])
    with pytest.raises(ValueError, match="unknown layered shallow-water case"):
        S.Solver(_cfg("x", case="galewsky"), verbose=False).initialize()
    # a thickness that would not be positive: the message carries the minimum
    with pytest.raises(ValueError, match=r"layer 0 is not positive \(minimum -"):
        LayeredShallowWater("tc2", depths=[100.0, 4000.0], density_ratio=0.99, winds=[1.0, 0.0]).global_fields(_grid(8))
    with pytest.raises(ValueError, match="density_ratio"):
        LayeredShallowWater("tc2", depths=[4000.0, 4000.0], density_ratio=1.2)
    c = _cfg("x")
    c["physics"]["layers"]["colour"] = 1
    with pytest.raises(ValueError, match="unknown key"):
        S.Solver(c, verbose=False).initialize()


def test_invariants_refused_and_names(tmp_path):
    s = S.Solver(_cfg(tmp_path), verbose=False)
    s.initialize()
    assert isinstance(s.physics, LayeredShallowWater) and s.physics.nl == 2
    assert s.fields == ["h0", "mx0", "my0", "mz0", "h1", "mx1", "my1", "mz1"]
    names = ["eta0", "eta1", "vorticity0", "divergence0", "pv0", "vorticity1", "divergence1", "pv1"]
    assert s.layer_names() == names
    assert s.latlon_names() == s.fields + names and s.spectrum_names() == s.fields + names
    with pytest.raises(ValueError, match="layered run"):
        s.invariants()
    with pytest.raises(ValueError, match="per layer"):
        s.latlon_field("vorticity", 6, 12)
    with pytest.raises(ValueError, match="per layer"):
        s.latlon_field("u", 6, 12)
    s.step(2)
    g = s.gather_global()
    assert np.array_equal(s.derived_field("eta0"), g[0] + g[4]) and np.array_equal(s.derived_field("eta1"), g[4])
    # the per-layer derived fields are the derived fields of a one-layer state holding that layer
    e = s.engines[0]
    for k in (0, 1):
        one = _engine(ShallowWater("tc2"), 12, dt=e.dt)
        one.set_state(e.tiles_view()[4 * k:4 * k + 4].clone())
        want = one.derived()[0]
        for j, nm in enumerate(("vorticity", "divergence", "pv")):
            got = s.derived_field(f"{nm}{k}")
            assert np.array_equal(got, global_of_field(one, want[j]))
    lat, lon = np.linspace(-1.2, 1.2, 5), np.linspace(0.1, 6.0, 5)
    assert s.latlon_field("eta1", 6, 12).shape == (6, 12) and s.zonal_mean("pv0", 6, 12).shape == (6,)
    assert s.sample(["h1", "eta0", "vorticity1"], lat, lon).shape == (3, 5)
    assert s.spectrum("eta0", 4).shape == (5,) and s.spectrum("pv1", 4).shape == (5,)


def global_of_field(engine, tiles):
    from stsphere.engine import assemble_global
    return assemble_global(engine.layout, {engine.rank: tiles.detach().double().cpu().numpy()})


def test_config_round_trip(tmp_path):
    """yaml -> Solver -> the physics the keywords describe; history with the
    layered names, metrics with mass0 / mass1 / energy, per-layer error norms,
    and a restart from a checkpoint on another tiling onto the same trajectory."""
    p = tmp_path / "c.yaml"
    cfg = _cfg(tmp_path / "run", history_interval=3, metrics_interval=2, checkpoint_interval=3,
               history_fields=["h0", "eta1", "pv0"])
    p.write_text(yaml.safe_dump(cfg))
    s = S.Solver(str(p), verbose=False)
    summary = s.run()
    ph = s.physics
    assert (ph.depths, ph.density_ratio, ph.winds, ph.case, ph.limiter) == ([4000.0, 4000.0], 0.9, [0.5, 0.4], "tc2", 2)
    assert s.cfg.physics.layers == cfg["physics"]["layers"] and s.step_count == 6
    g = s.gather_global()
    assert g.shape == (8, 6, 12, 12)
    hist = str(tmp_path / "run" / "history.zarr")
    assert np.array_equal(read_history(hist, "eta1")[-1], g[4]) and np.array_equal(read_history(hist, "h0")[-1], g[0])
    assert np.array_equal(read_history(hist, "pv0")[-1], s.derived_field("pv0"))
    m = read_metrics(str(tmp_path / "run" / "metrics.jsonl"))
    assert len(m) == 3
    for rec in m:
        assert abs(rec["mass0"] - m[0]["mass0"]) <= 1e-13 * m[0]["mass0"]
        assert abs(rec["mass1"] - m[0]["mass1"]) <= 1e-13 * m[0]["mass1"]
        assert np.isfinite(rec["energy"]) and "potential_enstrophy" not in rec
    norms = s.error_norms()
    assert set(norms) == {f"h{k}_{n}" for k in (0, 1) for n in ("l1", "l2", "linf")}
    assert 0 < norms["h0_l2"] < 1e-2 and summary["err_h1_l2"] == norms["h1_l2"]
    root = str(tmp_path / "run" / "checkpoints")
    assert ckpt.list_checkpoints(root) == [3, 6]
    c2 = _cfg(tmp_path / "run", nd=2, t=2, restore=ckpt.step_dir(root, 3))
    s2 = S.Solver(c2, verbose=False)
    s2.initialize()
    assert s2.step_count == 3
    s2.step(3)
    assert np.array_equal(s2.gather_global(), g)


def test_example_configs_load():
    import os
    from stsphere.driver import make_physics
    from stsphere.utils.config import load_config
    for name, case in (("c48_layers_tc2_1gpu.yaml", "tc2"), ("c96_layered_jet.yaml", "layered_jet")):
        c = load_config(os.path.join(S.__path__[0], "configs", name))
        ph = make_physics(c.physics)
        assert isinstance(ph, LayeredShallowWater) and ph.case == case and ph.nl == 2


def test_latlon_and_spectra_frames_on_two_virtual_ranks(tmp_path):
    """The frame outputs of ``run`` take the layered names; the per-layer derived
    fields of two virtual ranks (the layer's columns of the receive buffer) equal
    the one-rank fields bit for bit."""
    c = _cfg(tmp_path / "two", nd=2, case="tc5", history_interval=2, history_fields=["eta0", "pv1", "h1"],
             latlon=[6, 12], spectra=4)
    c["physics"]["layers"] = {"depths": [2000.0, 5960.0]}
    s = S.Solver(c, verbose=False)
    s.run()
    hist = str(tmp_path / "two" / "history.zarr")
    assert np.array_equal(read_history(hist, "pv1")[-1], s.derived_field("pv1"))
    c1 = _cfg(tmp_path / "one", case="tc5")
    c1["physics"]["layers"] = {"depths": [2000.0, 5960.0]}
    s1 = S.Solver(c1, verbose=False)
    s1.initialize()
    s1.step(6)
    for name in ("pv1", "vorticity0", "eta1"):
        assert np.array_equal(s.derived_field(name), s1.derived_field(name)), name
    assert not np.array_equal(s1.derived_field("pv0"), s1.derived_field("pv1"))


def test_spmd_gloo_ranks_state_restart_and_products(tmp_path):
    """The Solver on two SPMD gloo ranks (receive rows of 8 values): state,
    restart from the step-3 checkpoint, lat-lon fields, samples and the derived
    fields of both layers (each layer's columns of the receive rows) equal the
    one-rank run bit for bit, the spectra to 1e-12."""
    from rank_products import assert_equal, reference, spmd_run

    def cfg(out, nd):
        c = _cfg(out, nd=nd, t=1, case="tc5")
        c["physics"]["layers"] = {"depths": [2000.0, 5960.0], "density_ratio": 0.9}
        return c
    got = spmd_run(cfg(tmp_path / "ranks", 2), "layers", 2, tmp_path)
    state, prods = reference(cfg(tmp_path / "one", 1), "layers", 6)
    assert state.shape == (8, 6, 12, 12)
    assert_equal(got, state, prods, "layers, 2 gloo ranks")
    assert not np.array_equal(prods["latlon_h1"], prods["latlon_eta1"])      # tc5: b != 0 under the lower layer
