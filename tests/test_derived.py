"""Derived shallow-water fields (vorticity, divergence, potential vorticity) and
invariants: the PyTorch twin (models/derived.py) and its plumbing, on the CPU."""
import functools
import math
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import stsphere as S
from stsphere.engine import Engine, VirtualCluster, assemble_global
from stsphere.models import derived as md
from stsphere.models.base import extend
from stsphere.models.geometry import DAY, GRAVITY, CubedSphereGrid, xyz_to_lonlat
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout
from stsphere.utils import zarr_lite
from stsphere.utils.history import read_history

SUMS = md.INVARIANTS[:5]


def _exact_vorticity(case, grid):
    lon, lat = xyz_to_lonlat(grid.centers())
    if case == "tc2":
        u0 = 2.0 * math.pi * grid.radius / (12.0 * DAY)
        return 2.0 * u0 / grid.radius * np.sin(lat)
    w = K = 7.848e-6
    return 2.0 * w * np.sin(lat) - K * np.sin(lat) * np.cos(lat) ** 4 * 30.0 * np.cos(4.0 * lon)


def _raw_fields(e):
    """The raw-ghost variant: index-space ghosts, no panel-edge interpolation."""
    d = e.derived_fields
    w = extend(e.state, None, e.gmap, d.T, d.n, 1, ng=d.ng, cmap=e.cmap)
    w = torch.stack([w[0], w[1] / w[0], w[2] / w[0], w[3] / w[0]])
    return md.fields_from_window(w, e.tens, d.tabs, d.n, d.omega2)


@functools.lru_cache(maxsize=None)
def _errors(case, N):
    """{variant: (zeta l2, zeta linf, delta l2, delta linf)} at t = 0, relative
    to the exact vorticity (delta is exactly 0 for both cases)."""
    grid = CubedSphereGrid(N)
    L = TileLayout(N, 1, 1, ng=2)
    e = Engine(ShallowWater(case), L, grid=grid)
    A, ze = grid.areas(), _exact_vorticity(case, grid)
    nz = math.sqrt((ze * ze * A).sum())
    out = {}
    for name, f in (("interp", e.derived(exchange=False)[0]), ("raw", _raw_fields(e))):
        z = assemble_global(L, {0: f[0].numpy()})
        dv = assemble_global(L, {0: f[1].numpy()})
        out[name] = (math.sqrt(((z - ze) ** 2 * A).sum()) / nz, np.abs(z - ze).max() / np.abs(ze).max(),
                     math.sqrt((dv * dv * A).sum()) / nz, np.abs(dv).max() / np.abs(ze).max())
    return out


@pytest.mark.parametrize("case", ["tc2", "tc6"])
def test_convergence_against_analytic_fields(case):
    """Area-weighted l2 of zeta and of delta (over ||zeta_exact||) falls by at
    least 3x per doubling of N from 12 to 48; Linf falls from 24 to 48.  The
    raw-ghost variant does not meet the 3x ratio on delta: the panel-edge
    interpolation is what makes the errors converge."""
    e12, e24, e48 = (_errors(case, N) for N in (12, 24, 48))
    for a, b in ((e12, e24), (e24, e48)):
        zr, dr = a["interp"][0] / b["interp"][0], a["interp"][2] / b["interp"][2]
        print(f"{case}: zeta l2 ratio {zr:.2f}, delta l2 ratio {dr:.2f}, raw delta ratio "
              f"{a['raw'][2] / b['raw'][2]:.2f}")
        assert zr >= 3.0
        assert dr >= 3.0
        assert a["raw"][2] / b["raw"][2] < 3.0
    assert e48["interp"][1] < e24["interp"][1]
    assert e48["interp"][3] < e24["interp"][3]


def _global(layout, engines_fields):
    return np.stack([assemble_global(layout, {r: f[k].numpy() for r, f in engines_fields.items()})
                     for k in range(3)])


@pytest.mark.parametrize("case", ["tc5", "tc6"])
def test_decomposition_independence(case):
    N = 24
    grid = CubedSphereGrid(N)
    ref = None
    for t in (1, 2, 3):
        L = TileLayout(N, t, 1, ng=2)
        e = Engine(ShallowWater(case), L, grid=grid, dt=100.0)
        f, inv = e.derived()
        got = (_global(L, {0: f}), inv.numpy())
        if ref is None:
            ref = got
            assert np.isfinite(got[0]).all() and np.abs(got[0][0]).max() > 0
        else:
            assert np.array_equal(got[0], ref[0]), f"fields differ at t = {t}"
            assert np.array_equal(got[1], ref[1]), f"invariants differ at t = {t}: {got[1]} vs {ref[1]}"


def test_virtual_cluster_equals_one_rank():
    N = 12
    grid = CubedSphereGrid(N)
    single = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=grid)
    L = TileLayout(N, 1, 6, ng=2)
    vc = VirtualCluster(lambda: ShallowWater("tc5"), L, grid=grid, dt=single.dt)
    single.step(2)
    vc.step(2)
    f1, inv1 = single.derived()
    ds = [e.derived_fields for e in vc.engines]
    for d in ds:
        d.start()
    for d in ds:
        d.finish()
    res = [d.compute() for d in ds]
    got = _global(L, {e.rank: r[0] for e, r in zip(vc.engines, res)})
    assert np.array_equal(got, _global(single.layout, {0: f1}))
    tot = res[0][1].clone()
    for _, inv in res[1:]:
        tot[:5] = tot[:5] + inv[:5]
        tot[5] = torch.maximum(tot[5], inv[5])
    assert torch.equal(tot, inv1), (tot, inv1)


def test_stale_ghost_slots_are_never_read():
    """The window is pulled through the ghost map: NaN in every ghost slot of
    the padded state that is not a carried corner changes nothing."""
    N, t = 24, 2
    e = Engine(ShallowWater("tc5"), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N))
    f0, inv0 = e.derived()
    e.poison_corners()
    n, g, T, P = e.plan.n, e.plan.ng, e.plan.T, e.plan.P
    c = torch.arange(P)
    out = (c < g) | (c >= n + g)
    edge = out[:, None] ^ out[None, :]                      # exactly one coordinate outside: edge ghost strips
    idx = torch.nonzero(edge.reshape(-1)).reshape(-1)
    slots = (torch.arange(T)[:, None] * P * P + idx[None, :]).reshape(-1)
    for b in e.pool:
        b[:, slots] = float("nan")
    assert torch.isnan(e.state).any() and torch.isfinite(e.tiles_view()).all()
    f1, inv1 = e.derived()
    assert torch.equal(f0, f1) and torch.equal(inv0, inv1)


def _idxy(grid):
    LX, LY = grid.x_edge_lengths(), grid.y_edge_lengths()
    return 1.0 / (0.5 * (LY[:, :-1, :] + LY[:, 1:, :])) + 1.0 / (0.5 * (LX[:, :, :-1] + LX[:, :, 1:]))


def test_lake_at_rest():
    N = 12
    grid = CubedSphereGrid(N)
    e = Engine(ShallowWater("rest"), TileLayout(N, 2, 1, ng=2), grid=grid)
    f, inv = e.derived()
    inv = dict(zip(md.INVARIANTS, inv.tolist()))
    assert float(f[0].abs().max()) == 0.0 and float(f[1].abs().max()) == 0.0
    assert inv["circulation"] == 0.0 and inv["abs_circulation"] == 0.0
    assert inv["max_courant"] == e.dt * (math.sqrt(GRAVITY * 1000.0) * _idxy(grid).max())
    assert abs(inv["mass"] - 1000.0 * grid.total_area()) <= 1e-13 * inv["mass"]


def _cfg(out, N=12, nd=1, t=1, case="tc5", model="swe", **io):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
            "grid": {"N": N}, "physics": {"model": model, "case": case}, "time": {"nsteps": 10, "cfl": 0.9},
            "io": dict({"output_dir": str(out)}, **io)}


def test_max_courant_at_t0_against_cfl(tmp_path):
    """TC5 at the config's own cfl = 0.9.  The time step comes from
    ``min_spacing()`` (the shortest edge of the grid) and twice the largest
    speed; the running Courant number uses each cell's own spacings, so it is
    below cfl by the slack of that bound.  Measured with the twin: C24 0.7547,
    C48 0.7611 (0.84 cfl)."""
    s = S.Solver(_cfg(tmp_path, N=24), verbose=False)
    s.initialize()
    mc = s.invariants()["max_courant"]
    print("max_courant", mc)
    assert 0.5 * 0.9 <= mc <= 0.9


def test_history_fields_select_prognostic_and_derived(tmp_path):
    s = S.Solver(_cfg(tmp_path, history_interval=5, history_fields=["h", "vorticity"]), verbose=False)
    s.run()
    hist = str(tmp_path / "history.zarr")
    assert sorted(zarr_lite.list_arrays(hist)) == ["h", "step", "time", "vorticity"]
    z = read_history(hist, "vorticity")
    assert z.shape == (3, 6, 12, 12)
    assert np.array_equal(z[-1], s.derived_field("vorticity"))
    assert np.array_equal(read_history(hist, "h")[-1], s.global_field("h"))
    assert np.abs(z[0]).max() > 0 and not np.array_equal(z[0], z[-1])


def _tree_bytes(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root)] = fh.read()
    return out


def test_history_fields_null_keeps_the_history(tmp_path, monkeypatch):
    """``history_fields: null`` and a config without the key write the same
    bytes: the four prognostic fields through the unchanged path."""
    trees = []
    for k, extra in enumerate(({"history_fields": None}, {})):
        d = tmp_path / f"run{k}"
        d.mkdir()
        monkeypatch.chdir(d)
        S.Solver(_cfg("out", history_interval=5, **extra), verbose=False).run()
        trees.append(_tree_bytes(str(d / "out" / "history.zarr")))
    assert {os.path.dirname(k) for k in trees[0] if os.path.dirname(k)} == {"h", "mx", "my", "mz", "time", "step"}
    assert trees[0] == trees[1]


def test_history_fields_errors(tmp_path):
    s = S.Solver(_cfg(tmp_path, history_interval=5, history_fields=["h", "enstrophy"]), verbose=False)
    with pytest.raises(ValueError):
        s.initialize()
    c = _cfg(tmp_path, model="advection", case="cosine_bell", history_interval=5, history_fields=["vorticity"])
    with pytest.raises(ValueError):
        S.Solver(c, verbose=False).initialize()


def test_metrics_gain_the_invariants(tmp_path):
    from stsphere.utils.history import read_metrics
    s = S.Solver(_cfg(tmp_path, nd=2, metrics_interval=5), verbose=False)
    s.run()
    m = read_metrics(str(tmp_path / "metrics.jsonl"))
    inv, diag = s.invariants(), s.diagnostics()
    assert len(m) == 2 and m[-1]["step"] == 10
    for k in ("potential_enstrophy", "circulation", "max_courant"):
        assert m[-1][k] == inv[k]
    assert m[-1]["mass"] == diag["mass"] and m[-1]["energy"] == diag["energy"]
    assert set(diag) == {"mass", "energy"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, cfg, steps, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    s = S.Solver(cfg, verbose=False)
    try:
        s.initialize()
        s.step(steps)
        inv = s.invariants()
        fields = [s.derived_field(k) for k in md.FIELDS]
        if rank == 0:
            np.savez(os.path.join(outdir, "r0.npz"), fields=np.stack(fields),
                     inv=np.array([inv[k] for k in md.INVARIANTS]))
        else:
            assert all(f is None for f in fields)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def _native_buffers_worker(rank, world, port, N, outdir):
    """An engine whose halo traffic the native runtime owns (NativeBuffers):
    the derived fields exchange through a TorchDistTransport of their own."""
    import torch.distributed as dist
    from stsphere.parallel.comm import NativeBuffers
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        L = TileLayout(N, 1, world, ng=2)
        tr = NativeBuffers(L.plan(rank), 4, torch.float64, torch.device("cpu"))
        e = Engine(ShallowWater("tc5"), L, rank, transport=tr, dt=300.0)
        f, inv = e.derived()
        np.savez(os.path.join(outdir, f"r{rank}.npz"), fields=f.numpy(), inv=inv.numpy())
    finally:
        dist.destroy_process_group()


def test_gloo_native_buffers_exchange_on_their_own():
    N, world = 12, 2
    out = tempfile.mkdtemp()
    mp.spawn(_native_buffers_worker, args=(world, _free_port(), N, out), nprocs=world, join=True)
    L = TileLayout(N, 1, world, ng=2)
    single = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), dt=300.0)
    got = [np.load(os.path.join(out, f"r{r}.npz")) for r in range(world)]
    f1, inv1 = single.derived()
    glob = np.stack([assemble_global(L, {r: got[r]["fields"][k] for r in range(world)}) for k in range(3)])
    assert np.array_equal(glob, _global(single.layout, {0: f1}))
    assert max(g["inv"][5] for g in got) == float(inv1[5])
    assert abs(sum(g["inv"][0] for g in got) - float(inv1[0])) <= 1e-13 * float(inv1[0])


def test_gloo_two_ranks_equal_one_rank(tmp_path):
    out = tempfile.mkdtemp()
    cfg = _cfg(tmp_path, nd=2)
    mp.spawn(_worker, args=(2, _free_port(), cfg, 3, out), nprocs=2, join=True)
    s = S.Solver(_cfg(tmp_path, nd=1), verbose=False)
    s.initialize()
    s.step(3)
    got = np.load(os.path.join(out, "r0.npz"))
    for k, name in enumerate(md.FIELDS):
        assert np.array_equal(got["fields"][k], s.derived_field(name)), name
    inv = s.invariants()
    g = dict(zip(md.INVARIANTS, got["inv"].tolist()))
    for k in ("mass", "energy", "potential_enstrophy", "abs_circulation"):
        assert abs(g[k] - inv[k]) <= 1e-13 * abs(inv[k]), k
    assert abs(g["circulation"] - inv["circulation"]) <= 1e-13 * inv["abs_circulation"]
    assert g["max_courant"] == inv["max_courant"]
