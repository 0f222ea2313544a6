"""Lat-lon regridding (models/latlon.py, ops/latlon.py): the dual-mesh tables,
the PyTorch twin and the public interface, on the CPU."""
import functools
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import stsphere as S
from stsphere.__main__ import main as cli
from stsphere.engine import Engine, assemble_global
from stsphere.models import latlon as ml
from stsphere.models.geometry import CubedSphereGrid, xyz_to_lonlat
from stsphere.models.initial_conditions import williamson_tc2
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout
from stsphere.utils import zarr_lite

EPS = float(np.finfo(np.float64).eps)


def _pole_grid():
    """19 x 36 with the rows lat = -pi/2 and +pi/2 and the column lon = 0."""
    return np.linspace(-0.5 * math.pi, 0.5 * math.pi, 19), np.linspace(0.0, 2.0 * math.pi, 36, endpoint=False)


GRIDS = {"centred": lambda: ml.default_grid(45, 90), "poles": _pole_grid}


@functools.lru_cache(maxsize=None)
def _tables(N, grid):
    return ml.LatLonTables(N, *GRIDS[grid]())


def _signed_sides(tab):
    """[K, nelem] the smallest p . (v_i x v_i+1) over the sides of every element
    taken counter-clockwise (> 0: strictly inside, ~ 0: on a side), -inf for an
    element on the far side of the sphere.  Great-circle geometry only: no
    projection, no weights."""
    ctr = CubedSphereGrid(tab.N).centers().reshape(-1, 3)
    cells = tab.mesh.element_cells()
    tri = cells[:, 3] < 0
    ring = np.where(tri[:, None], cells[:, [0, 1, 2, 2]], cells[:, [0, 1, 3, 2]])      # around the element
    v = ctr[ring]                                                                       # [E, 4, 3]
    nrm = np.cross(v, np.roll(v, -1, axis=1))                                           # [E, 4, 3]
    orient = np.sign(np.einsum("ec,ec->e", nrm[:, 0], v[:, 2]))                         # side 0 against a third vertex
    out = []
    for p in np.array_split(tab.p, max(1, len(tab.p) // 256)):
        d = np.einsum("kc,esc->kes", p, nrm) * orient[None, :, None]
        d[:, tri, 2:] = np.inf                                                          # degenerate sides of a triangle
        d[:, tri, 2] = np.einsum("kc,ec->ke", p, nrm[tri, 3]) * orient[None, tri]       # v2 -> v0
        m = d.min(2)
        m[(np.einsum("kc,esc->kes", p, v) <= 0).any(2)] = -np.inf
        out.append(m)
    return np.concatenate(out)


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("N", [2, 3, 6, 12, 24])
def test_partition_of_the_sphere(N, grid):
    """Every target point lies in exactly one element: at most one element
    holds it strictly, the tables name that one, and a point on a shared side
    goes to the lowest id that holds it."""
    tab = _tables(N, grid)
    mesh = tab.mesh
    assert mesh.nelem == 6 * (N - 1) ** 2 + 12 * (N - 1) + 8
    m = _signed_sides(tab)
    tol = 1e-10
    strict = m > tol
    assert strict.sum(1).max() <= 1
    k = np.nonzero(strict.any(1))[0]
    assert np.array_equal(np.argmax(strict[k], 1), tab.elem[k])
    holds = m >= -tol
    assert holds.any(1).all()
    assert np.array_equal(np.argmax(holds, 1), tab.elem)          # the lowest id that holds the point
    # weights
    assert tab.w.min() >= -1e-12
    assert np.abs(tab.w.sum(1) - 1.0).max() <= 4 * EPS
    c = 3.7
    out = ml.regrid(torch.full((1, 6 * N * N), c, dtype=torch.float64), ml.regrid_tables(tab))
    assert float((out - c).abs().max()) <= 4 * EPS * c
    tri = tab.elem >= mesh.nelem - 8
    assert ((tab.w[tri] == 0).sum(1) == 1).all() and (tab.w[tri, 3] == 0).all()
    if N <= 6 and grid == "centred":
        assert tri.any()        # the check above is not vacuous
        assert ((tab.elem >= mesh.nint) & ~tri).any()
    # sources: real cells, the element's own
    assert tab.src.min() >= 0 and tab.src.max() < 6 * N * N
    cells = mesh.element_cells()[tab.elem]
    assert np.array_equal(np.where(cells >= 0, cells, cells[:, :1]), tab.src)


@pytest.mark.parametrize("N,t", [(6, 1), (12, 2), (12, 3)])
def test_rank_index_addresses_interior_cells(N, t):
    tab = _tables(N, "centred")
    L = TileLayout(N, t, 1, ng=2)
    pad, unp = tab.rank_index(L, 0)
    P, n = L.n + 4, L.n
    x, y = pad % P, (pad // P) % P
    assert pad.min() >= 0 and ((x >= 2) & (x < 2 + n) & (y >= 2) & (y < 2 + n)).all()
    e = Engine(ShallowWater("tc5"), L, grid=CubedSphereGrid(N))
    gid = torch.as_tensor(np.stack([e.geo.gather_global(np.arange(6 * N * N).reshape(6, N, N))]), dtype=torch.float64)
    e.interior(e.pool[1][:1]).copy_(gid)
    assert np.array_equal(e.pool[1][0].numpy()[pad], tab.src) and np.array_equal(gid.reshape(-1).numpy()[unp], tab.src)
    # two ranks: each source is owned by exactly one
    L2 = TileLayout(N, t, 2, ng=2)
    own = [tab.rank_index(L2, r)[0] >= 0 for r in range(2)]
    assert (own[0] ^ own[1]).all()


@pytest.mark.parametrize("N", [3, 6, 12])
def test_nodal_exactness(N):
    """A target at a cell centre returns that cell's value: interior, border
    and corner cells of every panel.  An interior centre is snapped onto its dual
    grid line (weights exactly 0 / 1); at a border or corner cell Newton and the
    barycentric formula leave weights within a few eps of 0 / 1, so the bound is
    16 eps max|field| (four slots, each within 4 eps of its nodal weight)."""
    grid = CubedSphereGrid(N)
    lon, lat = xyz_to_lonlat(grid.centers())
    rng = np.random.default_rng(5)
    field = rng.uniform(-1.0, 1.0, (6, N, N))
    x = torch.as_tensor(field.reshape(1, -1))
    picks = [(0, 0), (N - 1, 0), (0, N - 1), (N - 1, N - 1), (N // 2, 0), (N - 1, N // 2), (0, N // 2), (N // 2, N - 1),
             (N // 2, N // 2), (1, 1)]
    for f in range(6):
        for (i, j) in picks:
            tab = ml.LatLonTables(N, np.array([lat[f, j, i]]), np.array([lon[f, j, i]]))
            got = float(ml.regrid(x, ml.regrid_tables(tab))[0, 0, 0])
            assert abs(got - field[f, j, i]) <= 16 * EPS, (f, i, j, got - field[f, j, i])


# ---- second order -------------------------------------------------------------------
_AX = np.array([math.sin(0.6) * math.cos(0.4), math.sin(0.6) * math.sin(0.4), math.cos(0.6)])
_BX = np.array([0.48, -0.6, 0.64])


def _scalar(p):
    return 1.0 + 0.5 * (p @ _AX) ** 2 + 0.3 * (p @ _BX)


def _rotation(p):
    """Solid-body rotation about the tilted axis _AX, 38 m/s at its equator."""
    return np.cross(np.broadcast_to(38.0 * _AX, p.shape), p)


@functools.lru_cache(maxsize=None)
def _errors(N):
    """Relative (l2, linf) of the scalar, u and v on the 45 x 90 grid."""
    tab = _tables(N, "centred")
    tb = ml.regrid_tables(tab)
    c = CubedSphereGrid(N).centers().reshape(-1, 3)
    h = 1000.0 * _scalar(c)
    M = np.ascontiguousarray((h[:, None] * _rotation(c)).T)
    s = ml.regrid(torch.as_tensor(_scalar(c)[None]), tb).numpy().reshape(-1)
    uv = ml.winds(torch.as_tensor(h), torch.as_tensor(M), tb).numpy().reshape(2, -1)
    ve = _rotation(tab.p)
    exact = (_scalar(tab.p), (ve * tab.east).sum(1), (ve * tab.north).sum(1))
    out = []
    for a, b in zip((s, uv[0], uv[1]), exact):
        out += [math.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()), np.abs(a - b).max() / np.abs(b).max()]
    return out


def test_second_order():
    """Errors fall by at least 3.4 per doubling of N (asymptote 4).  Measured
    (scalar l2, linf; u l2, linf; v l2, linf), the table of docs/ARCHITECTURE.md:
      C12  1.134e-03 2.558e-03  2.645e-03 3.625e-03  2.714e-03 4.045e-03
      C24  2.706e-04 6.393e-04  6.530e-04 8.953e-04  6.536e-04 1.000e-03
      C48  7.055e-05 1.542e-04  1.656e-04 2.290e-04  1.708e-04 2.612e-04
      C96  1.793e-05 4.123e-05  4.196e-05 5.835e-05  4.328e-05 6.487e-05"""
    Ns = (12, 24, 48, 96)
    for a, b in zip(Ns[:-1], Ns[1:]):
        ratios = [x / y for x, y in zip(_errors(a), _errors(b))]
        print(f"C{a} -> C{b}:", " ".join(f"{r:.2f}" for r in ratios), " errors", " ".join(f"{v:.3e}" for v in _errors(b)))
        assert min(ratios) >= 3.4, (a, b, ratios)


# ---- decomposition and ghosts ------------------------------------------------------------
NAMES = ("h", "mx", "my", "mz", "vorticity", "divergence", "pv", "u", "v")


@functools.lru_cache(maxsize=None)
def _global_state(N=12, case="tc5"):
    e = Engine(ShallowWater(case), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N))
    e.step(2)
    return np.stack([assemble_global(e.layout, {0: v}) for v in e.tiles_view().numpy()]), e.dt


def _solver(tmp, N=12, nd=1, t=1, case="tc5", model="swe", **io):
    s = S.Solver({"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
                  "grid": {"N": N}, "physics": {"model": model, "case": case}, "time": {"nsteps": 10, "cfl": 0.9},
                  "io": dict({"output_dir": str(tmp)}, **io)}, verbose=False)
    s.initialize()
    return s


def _with_state(s, state):
    for e in s.engines:
        e.set_state(torch.as_tensor(np.stack([e.geo.gather_global(v) for v in state])))
    return s


def _all(s, nlat=19, nlon=36):
    return {n: (s.latlon_field(n, nlat, nlon), s.zonal_mean(n, nlat, nlon)) for n in NAMES}


def test_decomposition_independence(tmp_path):
    """One rank with 1, 2 and 3 tiles per edge: bitwise equal.  Six one-panel
    virtual ranks: within 8 eps max|field| of one rank, the bound of a four-term
    sum split over at most three ranks.  The ranks exchange the terms and not
    their partial sums (a partial sum of the Cartesian velocity rounds at the
    scale of the whole wind, which missed that bound for the small meridional
    component), so the channels that read the state alone are bitwise equal."""
    state, _ = _global_state()
    ref = _all(_with_state(_solver(tmp_path), state))
    for n in NAMES:
        assert np.isfinite(ref[n][0]).all() and ref[n][0].shape == (19, 36) and ref[n][1].shape == (19,)
    for t in (2, 3):
        got = _all(_with_state(_solver(tmp_path, t=t), state))
        for n in NAMES:
            assert np.array_equal(got[n][0], ref[n][0]) and np.array_equal(got[n][1], ref[n][1]), (t, n)
    got = _all(_with_state(_solver(tmp_path, nd=6), state))
    for n in NAMES:
        scale = np.abs(ref[n][0]).max()
        assert np.abs(got[n][0] - ref[n][0]).max() <= 8 * EPS * scale, n
        assert np.abs(got[n][1] - ref[n][1]).max() <= 8 * EPS * scale, n
        if n not in ("vorticity", "divergence", "pv"):
            assert np.array_equal(got[n][0], ref[n][0]) and np.array_equal(got[n][1], ref[n][1]), n


def _spmd_worker(rank, world, port, cfg, steps, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    s = S.Solver(cfg, verbose=False)
    try:
        s.initialize()
        s.step(steps)
        got = {n: (s.latlon_field(n, 19, 36), s.zonal_mean(n, 19, 36)) for n in NAMES}
        if rank == 0:
            np.savez(os.path.join(outdir, "r0.npz"), **{n: got[n][0] for n in NAMES},
                     **{"zm_" + n: got[n][1] for n in NAMES})
        else:
            assert all(a is None and z is None for a, z in got.values())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_gloo_two_ranks_equal_one_rank(tmp_path):
    """SPMD ranks: the term arrays are added on rank 0; other ranks get None."""
    out = str(tmp_path)
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    one = _solver(tmp_path)
    cfg = dict(one.config, parallelization=dict(one.config["parallelization"], num_devices=2))
    mp.spawn(_spmd_worker, args=(2, port, cfg, 3, out), nprocs=2, join=True)
    one.step(3)
    got = np.load(os.path.join(out, "r0.npz"))
    for n in NAMES:
        assert np.array_equal(got[n], one.latlon_field(n, 19, 36)), n
        assert np.array_equal(got["zm_" + n], one.zonal_mean(n, 19, 36)), n


def test_ghost_independence():
    """NaN in every ghost slot of the padded state: finite, bitwise unchanged."""
    state, dt = _global_state()
    e = Engine(ShallowWater("tc5"), TileLayout(12, 2, 1, ng=2), grid=CubedSphereGrid(12), dt=dt)
    e.set_state(torch.as_tensor(np.stack([e.geo.gather_global(v) for v in state])))
    ll = e.latlon(nlat=19, nlon=36)
    before = [ll.fields()[0].clone(), ll.winds()[0].clone()]
    keep = e.tiles_view().clone()
    e.state.fill_(float("nan"))
    e.tiles_view().copy_(keep)
    assert int(torch.isnan(e.state).sum()) == 4 * (e.plan.S - e.plan.T * e.plan.n ** 2)
    after = [ll.fields()[0], ll.winds()[0]]
    for a, b in zip(before, after):
        assert torch.isfinite(b).all() and torch.equal(a, b)


def test_zonal_mean():
    """TC2 (alpha = 0) is zonally symmetric: a regridded row of h varies by no
    more than the regridding error (measured against the closed form at the
    target points; C24: error 3.704 m, largest row spread 3.501 m).  ``zonal_mean`` is the row mean within 1e-13 max|field|."""
    N = 24
    e = Engine(ShallowWater("tc2"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N))
    ll = e.latlon(nlat=45, nlon=90)
    arr, zm = ll.fields()
    h = arr[0].numpy()
    exact = williamson_tc2(ll.tab.p)[0].reshape(45, 90)
    err = np.abs(h - exact).max()
    spread = (h.max(1) - h.min(1)).max()
    print(f"TC2 C{N}: regridding error {err:.3e} m, largest row spread {spread:.3e} m")
    assert err > 0 and spread <= err
    assert np.abs(zm[0].numpy() - h.mean(1)).max() <= 1e-13 * np.abs(h).max()
    assert np.abs(ml.zonal_mean(arr).numpy() - arr.numpy().mean(-1)).max() <= 1e-13 * np.abs(arr.numpy()).max()
    uv, zuv = ll.winds()
    assert np.abs(zuv.numpy() - uv.numpy().mean(-1)).max() <= 1e-13 * np.abs(uv.numpy()).max()
    assert np.abs(uv[1].numpy()).max() <= 1e-3 * np.abs(uv[0].numpy()).max()      # no meridional wind


# ---- public interface ------------------------------------------------------------------------
def test_engine_caches_and_arbitrary_grids():
    e = Engine(ShallowWater("tc5"), TileLayout(6, 1, 1, ng=2), grid=CubedSphereGrid(6))
    assert e.latlon(nlat=7, nlon=10) is e.latlon(nlat=7, nlon=10)
    lat, lon = ml.default_grid(7, 10)
    assert e.latlon(lat, lon) is e.latlon(nlat=7, nlon=10)
    band = e.latlon(np.radians([-30.0, 0.0, 12.5]), np.radians([10.0, 200.0]))
    assert band.fields()[0].shape == (4, 3, 2)
    with pytest.raises(ValueError):
        e.latlon()
    with pytest.raises(ValueError):
        e.latlon(np.array([0.3, 0.1]), lon)


def test_solver_history_and_cli(tmp_path):
    s = _solver(tmp_path / "run", history_interval=5, latlon=[19, 36])
    s.run()
    hl = str(tmp_path / "run" / "history_latlon.zarr")
    assert sorted(zarr_lite.list_arrays(hl)) == sorted(["h", "mx", "my", "mz", "u", "v", "lat", "lon", "time", "step"])
    lat, lon = ml.default_grid(19, 36)
    assert np.array_equal(zarr_lite.read_array(hl, "lat"), lat) and np.array_equal(zarr_lite.read_array(hl, "lon"), lon)
    assert list(zarr_lite.read_array(hl, "step")) == [0, 5, 10]
    for n in ("h", "mx", "u", "v"):
        a = zarr_lite.read_array(hl, n)
        assert a.shape == (3, 19, 36) and np.array_equal(a[-1], s.latlon_field(n, 19, 36)), n
        assert not np.array_equal(a[0], a[-1])
    # the middle frame: the state five steps in
    mid = _solver(tmp_path / "mid")
    mid.step(5)
    for n in ("h", "u"):
        assert np.array_equal(zarr_lite.read_array(hl, n)[1], mid.latlon_field(n, 19, 36)), n
    # the cube history is what it was
    assert zarr_lite.read_array(str(tmp_path / "run" / "history.zarr"), "h").shape == (3, 6, 12, 12)
    # offline regrid of the cube history: the same numbers (first and last frame:
    # a CPU run writes the cube history's middle frames from a view of the state
    # after the next chunk has stepped, so they are not the state of their step)
    for n in ("h", "u", "v"):
        out = str(tmp_path / f"{n}.npz")
        assert cli(["regrid", str(tmp_path / "run" / "history.zarr"), n, "19", "36", out]) == 0
        z = np.load(out)
        assert z["field"].shape == (3, 19, 36) and z["zonal_mean"].shape == (3, 19)
        assert np.array_equal(z["field"][[0, -1]], zarr_lite.read_array(hl, n)[[0, -1]]) and np.array_equal(z["lat"], lat)
        assert np.array_equal(z["zonal_mean"][-1], s.zonal_mean(n, 19, 36))
    with pytest.raises(ValueError):
        cli(["regrid", str(tmp_path / "run" / "history.zarr"), "pv", "19", "36", str(tmp_path / "x.npz")])


def test_history_fields_select_the_latlon_arrays(tmp_path):
    s = _solver(tmp_path, history_interval=10, history_fields=["h", "pv"], latlon=[7, 12])
    s.run()
    hl = str(tmp_path / "history_latlon.zarr")
    assert sorted(zarr_lite.list_arrays(hl)) == ["h", "lat", "lon", "pv", "step", "time"]
    assert np.array_equal(zarr_lite.read_array(hl, "pv")[-1], s.latlon_field("pv", 7, 12))


def test_unset_latlon_writes_nothing(tmp_path):
    s = _solver(tmp_path, history_interval=5)
    s.run()
    assert not os.path.exists(tmp_path / "history_latlon.zarr")
    with pytest.raises(ValueError):
        _solver(tmp_path, history_interval=5, latlon=[19])
    with pytest.raises(ValueError):
        _solver(tmp_path, history_interval=5, latlon=[19, 0])


@pytest.mark.parametrize("model,case", [("advection", "cosine_bell"), ("diffusion", "lima_flag")])
def test_other_models_regrid_their_scalar(tmp_path, model, case):
    s = _solver(tmp_path, model=model, case=case, history_interval=5, latlon=[9, 18])
    s.run()
    name = s.fields[0]
    a = s.latlon_field(name, 9, 18)
    g = s.global_field(name)
    assert a.shape == (9, 18) and g.min() - 1e-9 <= a.min() and a.max() <= g.max() + 1e-9 and a.max() > a.min()
    assert np.array_equal(zarr_lite.read_array(str(tmp_path / "history_latlon.zarr"), name)[-1], a)
    for bad in ("u", "v", "vorticity", "divergence", "pv"):
        with pytest.raises(ValueError, match="shallow-water model"):
            s.latlon_field(bad, 9, 18)
        with pytest.raises(ValueError, match="shallow-water model"):
            s.zonal_mean(bad, 9, 18)
    with pytest.raises(ValueError, match="unknown"):
        s.latlon_field("enstrophy", 9, 18)


def test_latlon_image_and_plot(tmp_path):
    from stsphere.utils.viz import latlon_image
    s = _solver(tmp_path / "run", history_interval=10)
    s.run()
    lat, lon = ml.default_grid(19, 36)
    p = latlon_image(s.latlon_field("h", 19, 36), lat, lon, str(tmp_path / "h.png"), zonal=s.zonal_mean("h", 19, 36))
    assert os.path.getsize(p) > 1000
    out = tmp_path / "plots"
    assert cli(["plot", str(tmp_path / "run" / "history.zarr"), "h", str(out), "--products", "six", "--latlon", "19", "36"]) == 0
    assert os.path.getsize(out / "h_latlon.png") > 1000
