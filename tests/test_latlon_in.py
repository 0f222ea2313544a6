"""Lat-lon input, the twin (models/latlon_in.py) on the CPU: constants, order of
accuracy across the poles, pole rows, quadrature, refusals and the file paths."""
import math

import numpy as np
import pytest

from stsphere.driver import Solver
from stsphere.models import initial_conditions as ic
from stsphere.models import latlon_in as ml
from stsphere.models.geometry import CubedSphereGrid, lonlat_to_xyz, lonlat_vectors
from stsphere.models.latlon import default_grid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

EPS = np.finfo(np.float64).eps
SWE = ShallowWater("tc2")


def source(nlat, nlon, poles):
    lat = np.linspace(-0.5 * math.pi, 0.5 * math.pi, nlat) if poles else default_grid(nlat, nlon)[0]
    return lat, np.arange(nlon) * (2.0 * math.pi / nlon)


def tc2(lat, lon):
    """h, u, v of TC2 tilted by pi / 2 (the flow crosses both poles) on the grid."""
    p = lonlat_to_xyz(*np.meshgrid(lon, lat))
    h, wind, _ = ic.williamson_tc2(p, alpha=0.5 * math.pi)
    e, n = lonlat_vectors(p)
    return h, (wind * e).sum(-1), (wind * n).sum(-1)


def ingest_global(N, lat, lon, order=3, q=1, **arrays):
    g = ml.source_grid(lat, lon)
    plan = ml.channel_plan(SWE, list(arrays))
    return ml.ingest_tiles(g, plan, ml.prepare(g, plan, arrays), TileLayout(N, 1, 1), 0, order, q)


def tc2_error(N, nlat, nlon, order, **kw):
    """linf errors of (h, M) at C<N> against the analytic cell-centre values."""
    lat, lon = source(nlat, nlon, True)
    h, u, v = tc2(lat, lon)
    out = ingest_global(N, lat, lon, order, h=h, u=kw.get("u", u), v=kw.get("v", v))
    ht, wind, _ = ic.williamson_tc2(CubedSphereGrid(N).centers(), alpha=0.5 * math.pi)
    M = np.stack([out[1], out[2], out[3]], -1)
    return np.abs(out[0] - ht).max(), np.abs(M - ht[..., None] * wind).max(), out


@pytest.mark.parametrize("poles", [True, False])
@pytest.mark.parametrize("order", ml.ORDERS)
@pytest.mark.parametrize("q", ml.QUADRATURES)
def test_constant(poles, order, q):
    lat, lon = source(13 if poles else 12, 24, poles)
    one = np.ones((lat.size, lon.size))
    out = ingest_global(5, lat, lon, order, q, h=7.0 * one, u=0.0 * one, v=0.0 * one)
    assert np.abs(out[0] - 7.0).max() <= 4 * EPS * 7.0
    assert all(np.abs(out[k]).max() == 0.0 for k in (1, 2, 3))


@pytest.mark.parametrize("order,least", [(1, 3.0), (3, 8.0)])
def test_order_of_accuracy(order, least):
    eh1, em1, _ = tc2_error(16, 25, 48, order)
    eh2, em2, _ = tc2_error(16, 49, 96, order)
    print(f"order {order}: h linf {eh1:.3e} -> {eh2:.3e} (x{eh1 / eh2:.2f}), M {em1:.3e} -> {em2:.3e} (x{em1 / em2:.2f})")
    assert eh1 / eh2 >= least and em1 / em2 >= least


def test_pole_rows():
    lat, lon = source(13, 24, True)
    _, _, out = tc2_error(5, 13, 24, 3)
    em16 = tc2_error(16, 25, 48, 3)[1]
    ht, wind, _ = ic.williamson_tc2(CubedSphereGrid(5).centers(), alpha=0.5 * math.pi)
    M = np.stack([out[1], out[2], out[3]], -1)
    for f in (0, 5):                                 # the polar cells: the panel centres
        assert np.isfinite(M[f, 2, 2]).all()
        err = np.abs(M[f, 2, 2] - (ht[..., None] * wind)[f, 2, 2]).max()
        print(f"polar cell of panel {f}: |M - analytic| = {err:.3e} (C16 from 25 x 48: {em16:.3e})")
        assert err <= 32.0 * em16                    # fourth order: 16 for the doubled spacing, 2 as in test 2
    # pole rows that hold other raw, multi-valued (u, v): every longitude's vector moved by a
    # wavenumber-2 horizontal vector, which sums to zero around the circle
    h, u, v = tc2(lat, lon)
    u2, v2 = u.copy(), v.copy()
    e, n = lonlat_vectors(lonlat_to_xyz(*np.meshgrid(lon, lat)))
    d = 10.0 * np.stack([np.cos(2 * lon), np.sin(2 * lon), 0 * lon], -1)
    for j in (0, 12):
        V = u[j, :, None] * e[j] + v[j, :, None] * n[j] + d
        u2[j], v2[j] = (V * e[j]).sum(-1), (V * n[j]).sum(-1)
    assert np.abs(u2[12] - u[12]).max() > 1.0
    _, _, out2 = tc2_error(5, 13, 24, 3, u=u2, v=v2)
    scale = np.abs(M).max()
    assert max(np.abs(out2[k] - out[k]).max() for k in (1, 2, 3)) <= 64 * EPS * scale


def test_quadrature_of_a_wave():
    """cos(12 lon) at C4, where a cell spans 3 / 4 of a wavelength, from a source fine
    enough in longitude (cubic error 0.0234 (12 dlon)^4 = 1e-11) that the cell value
    is the Gauss rule on the analytic wave: to 1e-10 for q = 1 and q = 4."""
    lat, lon = source(5, 16384, True)
    wave = np.cos(12.0 * lon)[None, :] * np.ones((lat.size, 1))
    amp = {}
    for q in (1, 4):
        got = ingest_global(4, lat, lon, 3, q, h=wave)[0]
        f, J, I = np.meshgrid(np.arange(6), np.arange(4), np.arange(4), indexing="ij")
        p, w = ml.cell_points(4, f, I, J, q)
        rule = (w * np.cos(12.0 * np.arctan2(p[..., 1], p[..., 0]))).sum(-1) / w.sum(-1)
        assert np.abs(got - rule).max() <= 1e-10
        amp[q] = np.abs(got[4, 1:3]).max()              # the equatorial rows of panel +x
    print(f"amplitude q = 1: {amp[1]:.6f}, q = 4: {amp[4]:.6f}")
    assert amp[4] < 0.5 * amp[1]


def test_refusals():
    lat, lon = source(13, 24, True)
    a = np.ones((13, 24))
    for bad_lat, bad_lon, word in ((np.sin(lat), lon, "non-uniform"), (lat[2:-2], lon, "regional"),
                                   (lat, lon[:12], "regional"), (lat, np.arange(23) * 2 * math.pi / 23, "even"),
                                   (lat[:3], lon, "4 latitude")):
        with pytest.raises(ValueError, match=word):
            ml.source_grid(bad_lat, bad_lon)
    cfg = {"parallelization": {"num_devices": 1}, "grid": {"N": 5}, "physics": {"model": "swe", "case": "tc2"}}
    s = Solver(cfg, verbose=False)
    s.initialize()
    with pytest.raises(ValueError, match="together"):
        s.set_from_latlon(lat, lon, h=a, u=a)
    with pytest.raises(ValueError, match="not among"):
        s.set_from_latlon(lat, lon, q0=a)
    adv = Solver(dict(cfg, physics={"model": "advection"}), verbose=False)
    adv.initialize()
    with pytest.raises(ValueError, match="shallow-water"):
        adv.set_from_latlon(lat, lon, u=a, v=a)
    lay = Solver(dict(cfg, physics={"model": "swe", "case": "rest", "layers": {"depths": [1e3, 2e3]}}), verbose=False)
    lay.initialize()
    with pytest.raises(ValueError, match="layered"):
        lay.set_from_latlon(lat, lon, h=a)
    with pytest.raises(ValueError, match="one of the two"):
        Solver(dict(cfg, io={"initial_condition": "a.zarr", "initial_latlon": "b.npz"}), verbose=False).initialize()


@pytest.mark.parametrize("devices,tiles", [(1, 1), (6, 2)])
def test_config_key_and_cli(tmp_path, devices, tiles):
    """``io.initial_latlon`` through ``Solver.initialize`` (one rank, virtual ranks)
    equals the twin, and the ``ingest`` command's group is read back by
    ``io.initial_condition``."""
    from stsphere.__main__ import main
    lat, lon = source(25, 48, True)
    h, u, v = tc2(lat, lon)
    npz = str(tmp_path / "data.npz")
    np.savez(npz, lat=lat, lon=lon, h=h, u=u, v=v, order=1)
    cfg = {"parallelization": {"num_devices": devices, "tiles_per_edge": tiles}, "grid": {"N": 8},
           "physics": {"model": "swe", "case": "tc2"}}
    s = Solver(dict(cfg, io={"initial_latlon": npz}), verbose=False)
    s.initialize()
    ref = ingest_global(8, lat, lon, 1, h=h, u=u, v=v)
    got = s.gather_global()
    assert all(np.array_equal(got[f], ref[f]) for f in range(4))
    e = s.engines[0]
    assert np.array_equal(e.state[:, e.halo_dst].numpy(), e.state[:, e.halo_src].numpy())
    import yaml
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    out = str(tmp_path / "ic.zarr")
    assert main(["ingest", str(tmp_path / "cfg.yaml"), npz, out]) == 0
    s2 = Solver(dict(cfg, io={"initial_condition": out}), verbose=False)
    s2.initialize()
    assert np.array_equal(s2.gather_global(), got)
