"""Shallow water with passive tracers, the PyTorch twin on the CPU
(``models/swe.py::ShallowWaterTracers``): what the scheme promises (SWE part
untouched, constancy, conservation, bounds under a limiter) and the plumbing
from the config file to the Solver's products.

Bounds: the figures measured when the scheme was prototyped (constancy 1.0e-15,
mass drift 2.2e-15, limited minima >= -2.1e-57) times 100 or more."""
import functools

import numpy as np
import pytest
import torch
import yaml

import stsphere as S
from stsphere.engine import Engine, VirtualCluster
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater, ShallowWaterTracers
from stsphere.parallel.layout import TileLayout
from stsphere.utils import checkpoint as ckpt
from stsphere.utils.history import read_history, read_metrics

from rough_states import global_of


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _engine(phys, N, t, **kw):
    return Engine(phys, TileLayout(N, t, 1, ng=2), grid=_grid(N), dtype=torch.float64, device="cpu", backend="torch",
                  **kw)


@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("t", [1, 2])
def test_swe_fields_untouched_and_constants_stay_constant(t, lim):
    """TC5 C12, 10 steps: (h, M) bit-identical to a plain ShallowWater run;
    q = 0.75 and q = 1 stay constant."""
    a = _engine(ShallowWaterTracers("tc5", tracers=[0.75, "constant"], limiter=lim), 12, t)
    b = _engine(ShallowWater("tc5", limiter=lim), 12, t, dt=a.dt)
    a.step(10)
    b.step(10)
    va = a.tiles_view()
    assert torch.equal(va[:4], b.tiles_view())
    for k, c in enumerate((0.75, 1.0)):
        dev = (va[4 + k] / va[0] - c).abs().max().item()
        print(f"t={t} lim={lim} q={c}: max deviation {dev:.2e}")
        assert dev < 1e-13


@pytest.mark.parametrize("lim", [1, 2, 3, 0])
@pytest.mark.parametrize("case,N", [("tc5", 12), ("tc6", 16)])
def test_cap_bounds_and_mass(case, N, lim):
    """A 0/1 cap, 40 steps: the limited schemes keep q in [0, 1], the unlimited
    slope must not (the test can fail); the tracer mass drifts by rounding."""
    e = _engine(ShallowWaterTracers(case, tracers=["cap"], limiter=lim), N, 1)
    A = e.tens["area"]
    m0 = (e.tiles_view()[4] * A).sum().item()
    e.step(40)
    v = e.tiles_view()
    q = v[4] / v[0]
    lo, hi = q.min().item(), q.max().item()
    drift = abs((v[4] * A).sum().item() - m0) / abs(m0)
    print(f"{case} C{N} lim={lim}: q min {lo:.3e} max {hi:.15g}; relative mass drift {drift:.2e}")
    assert drift < 1e-13
    if lim == 0:
        assert lo < -0.01 and hi > 1.01
    else:
        assert -1e-12 <= lo and hi <= 1.0 + 1e-12


def test_decomposition_independent():
    """t = 1, t = 2 and 4 virtual ranks after 20 steps: bit-identical, tracers
    included (the panel-edge pairs are chosen on the whole edge)."""
    N = 12
    mk = lambda: ShallowWaterTracers("tc5", tracers=["cap", "gradient"], limiter=2)   # noqa: E731
    a = _engine(mk(), N, 1)
    b = _engine(mk(), N, 2, dt=a.dt)
    vc = VirtualCluster(mk, TileLayout(N, 2, 4, ng=2), grid=_grid(N), dtype=torch.float64, device="cpu",
                        backend="torch", dt=a.dt)
    for x in (a, b, vc):
        x.step(20)
    ga = global_of(a)
    assert torch.equal(ga, global_of(b))
    assert torch.equal(ga, global_of(vc.engines))


def test_initial_conditions_and_diagnostics():
    e = _engine(ShallowWaterTracers("tc5", tracers=["constant", "cosine_bell", "cap", "gradient"]), 12, 1)
    assert e.physics.fields == ["h", "mx", "my", "mz", "hq0", "hq1", "hq2", "hq3"] and e.physics.kernel_id == 3
    v = e.tiles_view()
    q = v[4:] / v[0]
    assert torch.allclose(q[0], torch.ones_like(q[0]), rtol=0, atol=1e-15)
    assert 0.5 < q[1].max() <= 1 and q[1].min() == 0      # the TC1 bell, scaled to [0, 1] (C12: 0.82 at a centre)
    assert set(torch.unique(q[2]).tolist()) == {0.0, 1.0}
    assert q[3].min() > 0 and q[3].max() < 1
    d = e.diagnostics()
    for k in range(4):
        assert d[f"tracer_mass_{k}"] == pytest.approx(float((v[4 + k] * e.tens["area"]).sum()))
    assert d["tracer_mass_0"] == pytest.approx(d["mass"], rel=1e-14)


def test_rejections():
    from stsphere.ops.fused import fused_supported_config
    from stsphere.ops.hip_compute import march_supported
    from stsphere.ops.xgmi import XgmiHalo
    L = TileLayout(48, 1, 1, ng=2)
    assert fused_supported_config(ShallowWater("tc5"), "ssprk3", L) is None
    assert fused_supported_config(ShallowWaterTracers("tc5", tracers=["cap"]), "ssprk3", L) == "fused step: no tracers"
    assert march_supported(2, 2, False) and not march_supported(3, 2, False)
    with pytest.raises(ValueError, match="PPM"):
        ShallowWaterTracers("tc5", tracers=["cap"], limiter=4)
    with pytest.raises(ValueError, match="1 to 4"):
        ShallowWaterTracers("tc5", tracers=["cap"] * 5)
    with pytest.raises(ValueError, match="unknown tracer"):
        ShallowWaterTracers("tc5", tracers=["smoke"])
    # the direct xGMI exchange packs 1 or 4 fields: refused up front, so the
    # solver's transport chain moves on; asked for by name it is a config error
    e = _engine(ShallowWaterTracers("tc5", tracers=["cap"]), 12, 1)
    with pytest.raises(RuntimeError, match="1 or 4 fields"):
        XgmiHalo(e)
    c = _cfg("x", tracers=["cap"])
    c["runtime"] = {"comm": "xgmi"}
    with pytest.raises(ValueError, match="xgmi"):
        S.Solver(c, verbose=False).initialize()
    c = _cfg("x", tracers=["cap"])
    c["physics"]["limiter"] = "ppm"
    with pytest.raises(ValueError, match="PPM"):
        S.Solver(c, verbose=False).initialize()
    c = _cfg("x", tracers=["cap"] * 5)
    with pytest.raises(ValueError, match="physics.tracers"):
        S.Solver(c, verbose=False).initialize()


def test_march3_refuses_tracers():
    from stsphere.ops.march3 import march3_unsupported

    class _Compute:
        phys_id = 3

    class _E:
        backend = "hip"
        compute = _Compute()
    why = march3_unsupported(_E())
    assert why is not None


def _cfg(out, tracers=None, nd=1, t=1, **io):
    c = {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
         "grid": {"N": 12}, "physics": {"model": "swe", "case": "tc5", "limiter": "mc"},
         "time": {"nsteps": 6, "dt": 400.0}, "io": dict({"output_dir": str(out)}, **io)}
    if tracers is not None:
        c["physics"]["tracers"] = tracers
    return c


def test_empty_tracer_list_is_plain_shallow_water(tmp_path):
    s = S.Solver(_cfg(tmp_path, tracers=[]), verbose=False)
    s.initialize()
    assert type(s.physics) is ShallowWater and s.fields == ["h", "mx", "my", "mz"] and s.mix_names() == []


def test_yaml_run_history_metrics_checkpoint(tmp_path):
    p = tmp_path / "c.yaml"
    cfg = _cfg(tmp_path / "run", tracers=["cap", "cosine_bell"], history_interval=3, metrics_interval=2,
               checkpoint_interval=3, history_fields=["h", "hq0", "q0", "q1", "vorticity"])
    p.write_text(yaml.safe_dump(cfg))
    s = S.Solver(str(p), verbose=False)
    s.run()
    assert isinstance(s.physics, ShallowWaterTracers) and s.step_count == 6
    g = s.gather_global()
    assert g.shape == (6, 6, 12, 12)
    assert np.array_equal(s.tracer(0), g[4] / g[0]) and np.array_equal(s.tracer(1), g[5] / g[0])
    with pytest.raises(ValueError):
        s.tracer(2)
    hist = str(tmp_path / "run" / "history.zarr")
    assert np.array_equal(read_history(hist, "q0")[-1], s.tracer(0))
    assert np.array_equal(read_history(hist, "hq0")[-1], g[4])
    assert read_history(hist, "q1").shape == (3, 6, 12, 12)
    m = read_metrics(str(tmp_path / "run" / "metrics.jsonl"))
    assert len(m) == 3
    for rec in m:
        assert len(rec["tracer_mass"]) == len(rec["tracer_min"]) == len(rec["tracer_max"]) == 2
        assert abs(rec["tracer_mass"][0] - m[0]["tracer_mass"][0]) <= 1e-13 * m[0]["tracer_mass"][0]
        assert -1e-12 <= rec["tracer_min"][0] and rec["tracer_max"][0] <= 1 + 1e-12
    assert m[-1]["tracer_max"][1] == pytest.approx(float(s.tracer(1).max()))
    # restart from step 3 on another tiling: the same trajectory
    root = str(tmp_path / "run" / "checkpoints")
    assert ckpt.list_checkpoints(root) == [3, 6]
    c2 = _cfg(tmp_path / "run", tracers=["cap", "cosine_bell"], nd=2, t=2,
              restore=ckpt.step_dir(root, 3))
    s2 = S.Solver(c2, verbose=False)
    s2.initialize()
    assert s2.step_count == 3
    s2.step(3)
    assert np.array_equal(s2.gather_global(), g)


def test_swe_products_equal_the_plain_run(tmp_path):
    """Vorticity, invariants, winds and samples of a tracer run are those of
    the same run without tracers, exactly; the mixing ratios go through the
    same products."""
    lat, lon = np.linspace(-1.2, 1.2, 5), np.linspace(0.1, 6.0, 5)
    a = S.Solver(_cfg(tmp_path / "a"), verbose=False)
    b = S.Solver(_cfg(tmp_path / "b", tracers=["gradient", "cap"]), verbose=False)
    for s in (a, b):
        s.initialize()
        s.add_particles(lat, lon)
        s.step(4)
    assert np.array_equal(a.derived_field("vorticity"), b.derived_field("vorticity"))
    assert a.invariants() == b.invariants()
    assert np.array_equal(a.latlon_field("u", 6, 12), b.latlon_field("u", 6, 12))
    assert np.array_equal(a.sample(["h", "u"], lat, lon), b.sample(["h", "u"], lat, lon))
    assert np.array_equal(np.stack(a.particle_positions()), np.stack(b.particle_positions()))
    # q0 = (1 + sin lat) / 2 at the start, and smooth: its lat-lon image stays close to that
    q = b.latlon_field("q0", 6, 12)
    zm = b.zonal_mean("q0", 6, 12)
    assert q.shape == (6, 12) and zm.shape == (6,) and np.all(np.diff(zm) > 0)
    # sample("q0") interpolates the mixing ratio itself (not hq0 / h of the interpolated fields)
    from stsphere.models.points import lonlat_points
    e = b.engines[0]
    direct = e.points().tiles(lonlat_points(lat, lon), torch.stack([e.physics.mixing_ratio(e.tiles_view(), 0)]))
    assert np.array_equal(b.sample(["q0", "h"], lat, lon)[0], direct[0].numpy())
    assert b.spectrum("q1", 4).shape == (5,)
    assert "q0" in b.latlon_names() and "q1" in b.spectrum_names() and "q0" not in a.latlon_names()
    with pytest.raises(ValueError):
        a.latlon_field("q0", 6, 12)


@pytest.mark.parametrize("tlim", [None, "ppm"])
def test_spmd_gloo_ranks_state_restart_and_products(tlim, tmp_path):
    """The Solver on two SPMD gloo ranks (receive rows of 6 values, with PPM
    tracers three ghost layers): state, restart from the step-3 checkpoint,
    lat-lon fields, samples and the derived field (the SWE columns of the wider
    receive rows) equal the one-rank run bit for bit, the spectra to 1e-12."""
    from rank_products import assert_equal, reference, spmd_run

    def cfg(out, nd):
        c = _cfg(out, tracers=["gradient", "cap"], nd=nd, t=1)
        if tlim:
            c["physics"]["tracer_limiter"] = tlim
        return c
    got = spmd_run(cfg(tmp_path / "ranks", 2), "tracers", 2, tmp_path)
    state, prods = reference(cfg(tmp_path / "one", 1), "tracers", 6)
    assert state.shape == (6, 6, 12, 12)
    assert_equal(got, state, prods, f"tracers {tlim or 'mc'}, 2 gloo ranks")
