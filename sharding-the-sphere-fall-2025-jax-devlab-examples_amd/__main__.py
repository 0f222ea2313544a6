"""Command line:  python -m stsphere <command> ...

    run CONFIG.yaml [--days D | --nsteps K] [--plot] [--plot-field NAME]
                                                       run the solver (NAME: a prognostic field,
                                                       vorticity, divergence or pv)
    diag CONFIG.yaml [--restore PATH]                  print the invariants of the (restored) state
    info CONFIG.yaml                                   validate config, print sharding + halo plan
    schedule                                           print the reference 4-stage halo schedule
    roofline                                           slide-19 roofline / TT model for MI355X
    plot HISTORY.zarr FIELD OUTDIR [--log] [--products frames,band,six] [--every K] [--latlon NLAT NLON]
                                    [--spectrum LMAX] [--tracks]
                                                       sphere frames, equatorial band, six-panel;
                                                       --latlon: regridded image + zonal-mean profile;
                                                       --spectrum: log-log power per degree, first and last frame;
                                                       --tracks: history_particles.zarr (beside HISTORY.zarr)
                                                       over the last frame's lat-lon image
    sample HISTORY.zarr FIELD POINTS.npz OUT.npz       time series [frames, K] of a history field (or u, v) at
                                                       the lat, lon (radians) of POINTS.npz, on the CPU
    regrid HISTORY.zarr FIELD NLAT NLON OUT.npz        regrid a history field (or u, v of a shallow-water
                                                       history) to the cell-centred lat-lon grid, on the CPU
    spectrum HISTORY.zarr FIELD LMAX OUT.npz           power per degree 0 .. LMAX of a history field (``ke``:
                                                       the kinetic-energy spectrum of a shallow-water
                                                       history), on the CPU
    synth HISTORY.zarr FIELD LMAX OUT.npz [--band LMIN LCUT]
                                                       a history field analysed to degree LMAX and synthesised
                                                       back on the cells (--band: degrees LMIN .. LCUT only), or
                                                       the streamfunction / velocity_potential of a
                                                       shallow-water history, on the CPU
    ensemble CONFIG.yaml [--members M] [--amplitude A] [--days D | --nsteps K] [--batched]
                                                       perturbed members of one config on one device
                                                       (--batched: every member's stage in one launch)
    build                                              compile the gfx950 library
"""
import argparse
import json
import os
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(prog="stsphere")
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("config")
    r.add_argument("--days", type=float)
    r.add_argument("--nsteps", type=int)
    r.add_argument("--plot", action="store_true")
    r.add_argument("--plot-field", default=None,
                   help="field of the final plot: a prognostic name, vorticity, divergence or pv (default: the first)")
    dg = sub.add_parser("diag")
    dg.add_argument("config")
    dg.add_argument("--restore", default=None, help="checkpoint to read the state from")
    i = sub.add_parser("info")
    i.add_argument("config")
    sub.add_parser("schedule")
    sub.add_parser("roofline")
    p = sub.add_parser("plot")
    p.add_argument("history")
    p.add_argument("field")
    p.add_argument("outdir")
    p.add_argument("--log", action="store_true")
    p.add_argument("--products", default="frames,band,six")
    p.add_argument("--every", type=int, default=1)
    p.add_argument("--latlon", type=int, nargs=2, metavar=("NLAT", "NLON"), default=None,
                   help="also write the last frame regridded to NLAT x NLON with its zonal-mean profile")
    p.add_argument("--spectrum", type=int, metavar="LMAX", default=None,
                   help="also write the log-log power per degree 0 .. LMAX of the first and the last frame")
    p.add_argument("--tracks", action="store_true",
                   help="also draw the particle tracks of history_particles.zarr over the last frame")
    sa = sub.add_parser("sample")
    sa.add_argument("history")
    sa.add_argument("field")
    sa.add_argument("points")
    sa.add_argument("out")
    rg = sub.add_parser("regrid")
    rg.add_argument("history")
    rg.add_argument("field")
    rg.add_argument("nlat", type=int)
    rg.add_argument("nlon", type=int)
    rg.add_argument("out")
    sp = sub.add_parser("spectrum")
    sp.add_argument("history")
    sp.add_argument("field")
    sp.add_argument("lmax", type=int)
    sp.add_argument("out")
    sy = sub.add_parser("synth")
    sy.add_argument("history")
    sy.add_argument("field")
    sy.add_argument("lmax", type=int)
    sy.add_argument("out")
    sy.add_argument("--band", type=int, nargs=2, metavar=("LMIN", "LCUT"), default=None,
                    help="keep the degrees LMIN .. LCUT only")
    en = sub.add_parser("ensemble")
    en.add_argument("config")
    en.add_argument("--members", type=int, default=2)
    en.add_argument("--amplitude", type=float, default=1e-4)
    en.add_argument("--days", type=float)
    en.add_argument("--nsteps", type=int)
    en.add_argument("--batched", action="store_true",
                    help="batched storage: one stage launch steps every member (Ensemble mode='batched')")
    sub.add_parser("build")
    a = ap.parse_args(argv)

    if a.cmd == "build":
        from .ops import build
        for v in sorted(build.VARIANT_FLAGS):
            print(build.build(force=True, variant=v))
        return 0
    if a.cmd == "schedule":
        from .ops.halo import make_halo_exchange
        from .parallel.topology import create_communication_schedule
        make_halo_exchange(create_communication_schedule(), 4)
        return 0
    if a.cmd == "roofline":
        from .utils.roofline import report
        print(report())
        return 0
    if a.cmd == "plot":
        from .utils.viz import history_products
        for f in history_products(a.history, a.field, a.outdir, log=a.log, every=a.every,
                                  products=tuple(a.products.split(","))):
            print(f)
        if a.latlon:
            from .utils.viz import latlon_image
            r = regrid_history(a.history, a.field, a.latlon[0], a.latlon[1])
            os.makedirs(a.outdir, exist_ok=True)
            print(latlon_image(r["field"][-1], r["lat"], r["lon"], os.path.join(a.outdir, f"{a.field}_latlon.png"),
                               title=f"{a.field}, day {r['time'][-1] / 86400.0:.2f}", zonal=r["zonal_mean"][-1]))
        if a.spectrum is not None:
            from .utils.viz import spectrum_plot
            r = spectrum_history(a.history, a.field, a.spectrum)
            os.makedirs(a.outdir, exist_ok=True)
            k = [0, len(r["time"]) - 1] if len(r["time"]) > 1 else [0]
            print(spectrum_plot(r["spectrum"][k], os.path.join(a.outdir, f"{a.field}_spectrum.png"),
                                title=f"{a.field}: power per degree",
                                ylabel="E_l (m^2 / s^2)" if a.field == "ke" else "power per degree",
                                labels=[f"day {r['time'][j] / 86400.0:.2f}" for j in k]))
        if a.tracks:
            import numpy as np
            from .utils import zarr_lite
            from .utils.viz import tracks_plot
            ph = os.path.join(os.path.dirname(os.path.abspath(a.history)), "history_particles.zarr")
            nlat, nlon = a.latlon or (91, 180)
            r = regrid_history(a.history, a.field, nlat, nlon)
            os.makedirs(a.outdir, exist_ok=True)
            print(tracks_plot(r["field"][-1], r["lat"], r["lon"], zarr_lite.read_array(ph, "lat"),
                              zarr_lite.read_array(ph, "lon"), os.path.join(a.outdir, f"{a.field}_tracks.png"),
                              title=f"{a.field} and particle tracks, day {r['time'][-1] / 86400.0:.2f}"))
        return 0
    if a.cmd == "sample":
        import numpy as np
        pts = np.load(a.points)
        r = sample_history(a.history, a.field, pts["lat"], pts["lon"])
        np.savez(a.out, **r)
        print(json.dumps({"out": a.out, "field": a.field, "shape": list(r["field"].shape)}))
        return 0
    if a.cmd == "spectrum":
        import numpy as np
        r = spectrum_history(a.history, a.field, a.lmax)
        np.savez(a.out, **r)
        print(json.dumps({"out": a.out, "field": a.field, "shape": list(r["spectrum"].shape)}))
        return 0
    if a.cmd == "synth":
        import numpy as np
        r = synth_history(a.history, a.field, a.lmax, band=a.band)
        np.savez(a.out, **r)
        print(json.dumps({"out": a.out, "field": a.field, "shape": list(r["field"].shape)}))
        return 0
    if a.cmd == "regrid":
        import numpy as np
        r = regrid_history(a.history, a.field, a.nlat, a.nlon)
        np.savez(a.out, **r)
        print(json.dumps({"out": a.out, "field": a.field, "shape": list(r["field"].shape)}))
        return 0
    if a.cmd == "ensemble":
        print(json.dumps(run_ensemble(a.config, a.members, a.amplitude, a.days, a.nsteps, batched=a.batched),
                         default=float))
        return 0
    from .utils.config import load_config
    if a.cmd == "run" and load_config(a.config).physics.model == "planar_swe":
        from .models.planar import run_panel      # single flat panel, no halos
        print(json.dumps(run_panel(a.config), default=float))
        return 0
    from .driver import Solver
    s = Solver(a.config)
    if a.cmd == "info":
        s.setup_sharding()
        from .parallel.layout import TileLayout
        c = s.cfg
        L = TileLayout(c.grid.N, c.parallelization.tiles_per_edge, c.parallelization.num_devices,
                       ng=c.grid.halo, owner=s.sharding.owner)
        for rk in range(L.num_ranks):
            print(L.plan(rk).summary())
        return 0
    if a.cmd == "diag":
        if a.restore:
            s.cfg.io.restore = a.restore
        s.initialize()
        inv = s.invariants()                      # collective under SPMD
        s.close()
        if s.rank == 0:
            print(json.dumps(dict(step=s.step_count, time_s=s.time, **inv), default=float))
        return 0
    from .models.derived import FIELDS as derived_names
    s.initialize()
    pf = a.plot_field
    if pf is not None and pf not in list(s.fields) + list(derived_names):
        ap.error(f"--plot-field {pf}: choose from {list(s.fields) + list(derived_names)}")
    summary = s.run(nsteps=a.nsteps, days=a.days)
    g = s.gather_global() if a.plot else None     # collective under SPMD
    dfield = s.derived_field(pf) if a.plot and pf in derived_names else None   # collective under SPMD
    s.close()                                     # collective under SPMD (exchange rings)
    if s.rank == 0:
        print(json.dumps(summary, default=float))
        if a.plot and pf is not None:
            from .utils.viz import sphere_plot
            out = s.cfg.io.output_dir
            os.makedirs(out, exist_ok=True)
            arr = dfield if dfield is not None else g[s.fields.index(pf)]
            print(sphere_plot(arr, s.grid, os.path.join(out, f"{pf}_final.png")))
        elif a.plot:
            from .utils.viz import history_products, sphere_plot
            out = s.cfg.io.output_dir
            os.makedirs(out, exist_ok=True)
            hist = os.path.join(out, "history.zarr")
            log = s.physics.name == "diffusion"
            if os.path.exists(os.path.join(hist, ".zgroup")):
                for f in history_products(hist, s.fields[0], os.path.join(out, "plots"), grid=s.grid, log=log,
                                          products=("band", "six")):
                    print(f)
            print(sphere_plot(g[0], s.grid, os.path.join(out, f"{s.fields[0]}_final.png"), log=log))
    return 0


def sample_history(history: str, field: str, lat, lon) -> dict:
    """Every frame of a history field at the points lat / lon [K] (radians;
    ``u`` / ``v``: from the h, mx, my, mz of a shallow-water history), with the
    twin on the CPU (models/points.py): field [frames, K], lat, lon, time."""
    import numpy as np
    import torch
    from .models import points as mp
    from .utils import zarr_lite
    have = zarr_lite.list_arrays(history)
    wind = field in ("u", "v") and field not in have
    need = ["h", "mx", "my", "mz"] if wind else [field]
    missing = [f for f in need if f not in have]
    if missing:
        raise ValueError(f"{history}: no array {missing} (it holds {[f for f in have if f not in ('time', 'step')]})")
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    lon = np.asarray(lon, dtype=np.float64).reshape(-1)
    p = mp.lonlat_points(lat, lon)
    if len(p) < 1 or not np.isfinite(p).all():
        raise ValueError("sample: lat and lon must be finite and hold at least one point")
    src = np.stack([zarr_lite.read_array(history, f) for f in need], 1)       # [frames, C, 6, N, N]
    loc = mp.locate(src.shape[-1], p)
    if wind:
        d = (np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)]) if field == "u" else
             np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)]))
        d = torch.as_tensor(d)
    out = []
    for fr in torch.as_tensor(np.ascontiguousarray(src, dtype=np.float64)):
        if wind:
            v = mp.velocity(fr, loc)
            out.append((v[0] * d[0] + v[1] * d[1]) + v[2] * d[2])
        else:
            out.append(mp.sample(fr, loc)[0])
    return {"field": torch.stack(out).numpy(), "lat": lat, "lon": lon, "time": zarr_lite.read_array(history, "time")}


def regrid_history(history: str, field: str, nlat: int, nlon: int) -> dict:
    """Every frame of a history field on the cell-centred nlat x nlon grid
    (``u`` / ``v``: from the h, mx, my, mz of a shallow-water history), with the
    PyTorch twin on the CPU: field [frames, nlat, nlon], zonal_mean [frames,
    nlat], lat, lon (radians), time."""
    import numpy as np
    import torch
    from .models import latlon as ml
    from .utils import zarr_lite
    have = zarr_lite.list_arrays(history)
    wind = field in ("u", "v") and field not in have
    need = ["h", "mx", "my", "mz"] if wind else [field]
    missing = [f for f in need if f not in have]
    if missing:
        raise ValueError(f"{history}: no array {missing} (it holds {[f for f in have if f not in ('time', 'step')]})")
    src = np.stack([zarr_lite.read_array(history, f) for f in need], 1)       # [frames, C, 6, N, N]
    lat, lon = ml.default_grid(nlat, nlon)
    tb = ml.regrid_tables(ml.tables_for(src.shape[-1], lat, lon))
    out = []
    for fr in torch.as_tensor(np.ascontiguousarray(src, dtype=np.float64)):
        out.append(ml.winds(fr[0], fr[1:4], tb)[("u", "v").index(field)] if wind else ml.regrid(fr, tb)[0])
    out = torch.stack(out)
    return {"field": out.numpy(), "zonal_mean": ml.zonal_mean(out).numpy(), "lat": lat, "lon": lon,
            "time": zarr_lite.read_array(history, "time")}


def spectrum_history(history: str, field: str, lmax: int) -> dict:
    """Power per degree of every frame of a history field with the PyTorch
    twin on the CPU (models/spectra.py): spectrum [frames, L+1], degree, time.
    ``ke``: the kinetic-energy spectrum from the h, mx, my, mz of a
    shallow-water history (vorticity and divergence by the derived-field twin)."""
    import numpy as np
    import torch
    from .models import spectra as ms
    from .models.geometry import EARTH_RADIUS, CubedSphereGrid
    from .utils import zarr_lite
    have = zarr_lite.list_arrays(history)
    if field in ("u", "v") and field not in have:
        raise ValueError(f"{field!r} is a vector component, not a scalar on the sphere; use the field 'ke' for the "
                         f"kinetic-energy spectrum of the winds")
    ke = field == "ke" and field not in have
    need = ["h", "mx", "my", "mz"] if ke else [field]
    missing = [f for f in need if f not in have]
    if missing:
        raise ValueError(f"{history}: no array {missing} (it holds {[f for f in have if f not in ('time', 'step')]})")
    src = np.stack([zarr_lite.read_array(history, f) for f in need], 1)       # [frames, C, 6, N, N]
    N = src.shape[-1]
    cfg = (zarr_lite.read_attrs(history).get("config") or {})
    radius = (cfg.get("grid") or {}).get("radius") or EARTH_RADIUS
    grid = CubedSphereGrid(N, radius)
    out = []
    if ke:
        from .engine import Engine
        from .models.swe import ShallowWater
        from .parallel.layout import TileLayout
        e = Engine(ShallowWater((cfg.get("physics") or {}).get("case") or "tc5"), TileLayout(N, 1, 1, ng=2), grid=grid)
        sp = e.spectra(lmax)
        for fr in torch.as_tensor(np.ascontiguousarray(src, dtype=np.float64)):
            e.set_state(fr)
            c = sp.partial_tiles(e.derived()[0][:2])
            out.append(ms.ke_spectrum(c[0], c[1], radius))
    else:
        tb = ms.grid_tables(grid, lmax)
        for fr in torch.as_tensor(np.ascontiguousarray(src, dtype=np.float64)):
            out.append(ms.power(ms.analyse(fr.reshape(1, -1), tb))[0])
    return {"spectrum": torch.stack(out).numpy(), "degree": np.arange(lmax + 1),
            "time": zarr_lite.read_array(history, "time")}


def synth_history(history: str, field: str, lmax: int, band=None) -> dict:
    """Every frame of a history field analysed to degree ``lmax``, its degrees
    outside ``band`` = (lmin, lcut) dropped, and synthesised back on the cells
    with the PyTorch twin on the CPU (models/spectra.py): field [frames, 6, N, N],
    time.  ``streamfunction`` / ``velocity_potential``: psi / chi (m^2 / s) from
    the h, mx, my, mz of a shallow-water history (vorticity and divergence by
    the derived-field twin)."""
    import numpy as np
    import torch
    from .models import spectra as ms
    from .models.geometry import EARTH_RADIUS, CubedSphereGrid
    from .utils import zarr_lite
    have = zarr_lite.list_arrays(history)
    if field in ("u", "v") and field not in have:
        raise ValueError(f"{field!r} is a vector component, not a scalar on the sphere; use the fields "
                         f"'streamfunction' and 'velocity_potential' for the winds")
    hel = field in ("streamfunction", "velocity_potential") and field not in have
    need = ["h", "mx", "my", "mz"] if hel else [field]
    missing = [f for f in need if f not in have]
    if missing:
        raise ValueError(f"{history}: no array {missing} (it holds {[f for f in have if f not in ('time', 'step')]})")
    src = np.stack([zarr_lite.read_array(history, f) for f in need], 1)       # [frames, C, 6, N, N]
    N = src.shape[-1]
    cfg = (zarr_lite.read_attrs(history).get("config") or {})
    radius = (cfg.get("grid") or {}).get("radius") or EARTH_RADIUS
    grid = CubedSphereGrid(N, radius)
    lmax = ms.check_lmax(lmax, N)
    fac = ms.band_factors(lmax) if band is None else ms.band_factors(lmax, band[0], band[1])
    out = []
    if hel:
        from .engine import Engine
        from .models.swe import ShallowWater
        from .parallel.layout import TileLayout
        e = Engine(ShallowWater((cfg.get("physics") or {}).get("case") or "tc5"), TileLayout(N, 1, 1, ng=2), grid=grid)
        sp = e.spectra(lmax)
        which = 0 if field == "streamfunction" else 1
        for fr in torch.as_tensor(np.ascontiguousarray(src, dtype=np.float64)):
            e.set_state(fr)
            c = sp.partial_tiles(e.derived()[0][:2])
            co = ms.scale_degrees(ms.helmholtz(c[0], c[1], radius)[which], fac)
            out.append(sp.synthesise(co[None])[0])
    else:
        tb = ms.grid_tables(grid, lmax)
        for fr in torch.as_tensor(np.ascontiguousarray(src, dtype=np.float64)):
            co = ms.scale_degrees(ms.analyse(fr.reshape(1, -1), tb), fac)
            out.append(ms.synthesise(ms.clean_coeffs(co), tb)[0].reshape(6, N, N))
    return {"field": torch.stack(out).numpy(), "time": zarr_lite.read_array(history, "time")}


def run_ensemble(config, members: int, amplitude: float, days=None, nsteps=None, *, batched: bool = False) -> dict:
    """``members`` perturbed copies of a run configuration stepped together
    on one device (``stsphere.Ensemble``; ``batched``: its mode 'batched', one
    stage launch for all members); returns throughput and spread."""
    import math
    import time
    import torch
    from .ensemble import Ensemble
    from .models.geometry import DAY
    from .utils.config import load_config
    c = load_config(config)
    ens = Ensemble.from_config(c, members, amplitude=amplitude, mode="batched" if batched else "streams")
    if nsteps is None:
        d = days if days is not None else c.time.days
        nsteps = int(math.ceil(d * DAY / ens.dt - 1e-9)) if d is not None else (c.time.nsteps or 1)
    ens.prepare(nsteps)
    before = ens.spread()
    sync = torch.cuda.synchronize if ens.native else (lambda: None)
    sync()
    t0 = time.perf_counter()
    ens.run(nsteps)
    sync()
    wall = time.perf_counter() - t0
    after = ens.spread()
    ens.close()
    cells = 6 * c.grid.N ** 2
    return {"members": members, "mode": ens.mode, "steps": nsteps, "dt": ens.dt, "wall_s": wall,
            "aggregate_cell_updates_per_s": members * cells * nsteps / max(wall, 1e-12),
            "native": ens.native, "field0_mean": after["mean"], "field0_spread_rms_initial": before["spread_rms"],
            "field0_spread_rms_final": after["spread_rms"]}


if __name__ == "__main__":
    sys.exit(main())
