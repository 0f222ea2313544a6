"""Multi-rank paths without a cluster: in-process virtual ranks and
multi-process gloo (modes (a) and (b))."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from stsphere.engine import Engine, VirtualCluster
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater, ShallowWaterTracers
from stsphere.models.advection import Advection
from stsphere.parallel.layout import TileLayout

from layer_states import layer_physics


# physics axis: the MC-limited default (two ghost layers) and PPM (limiter 4), the
# only scheme with three: two interpolated panel-edge layers, 3 x 3 carried corners
PHYSICS = {"swe_mc": lambda: ShallowWater("tc5"),
           "swe_ppm": lambda: ShallowWater("tc5", limiter=4),
           "adv_ppm": lambda: Advection(limiter=4)}
HALO = {"swe_mc": 2, "swe_ppm": 3, "adv_ppm": 3}


def _with_physics(cases, names):
    """Every case for every physics; the MC cases keep their bare ids."""
    return [pytest.param(*c, ph, id="-".join(map(str, c)) + ("" if ph == "swe_mc" else "-" + ph))
            for ph in names for c in cases]


@pytest.mark.parametrize("t,R,phys", _with_physics([(1, 2), (1, 3), (1, 6), (2, 4), (2, 8), (2, 12)], list(PHYSICS)))
def test_virtual_ranks_bitwise_equal_single(t, R, phys):
    N = 12
    g = CubedSphereGrid(N)
    make = PHYSICS[phys]
    ng = make().halo
    assert ng == HALO[phys]
    single = Engine(make(), TileLayout(N, t, 1, ng=ng), grid=g)
    vc = VirtualCluster(make, TileLayout(N, t, R, ng=ng), grid=g, dt=single.dt)
    if phys == "adv_ppm":     # the cosine bell is zero on most of the sphere: a state with signal at every rank boundary
        from rough_states import install, make_state
        G = make_state(single, "scalar")
        for e in [single] + vc.engines:
            install(e, G)
    single.step(3)
    vc.step(3)
    for f in range(make().F):
        assert np.array_equal(single.global_field(f), vc.global_field(f))


# the physics with wider receive rows: tracers ride behind (h, M) (F = 4 + NQ; with
# PPM mixing ratios three ghost layers), two layers are two shallow-water blocks (F = 8)
WIDE = {"trc_mc": lambda: ShallowWaterTracers("tc5", tracers=["cap", "cosine_bell"], limiter=2),
        "trc_ppm": lambda: ShallowWaterTracers("tc5", tracers=["cap"], limiter=2, tracer_limiter="ppm"),
        "layers": lambda: layer_physics()}
WIDE_F = {"trc_mc": (6, 2), "trc_ppm": (5, 3), "layers": (8, 2)}        # (F, ghost layers)


def _wide_start(phys, N):
    """The rough start state [F, 6, N, N] of a WIDE physics (tracer_states.py,
    layer_states.py): the cap and the cosine bell are zero on most of the
    sphere, the rough states have signal in every column at every rank boundary."""
    if phys == "layers":
        from layer_states import global_state
        return global_state(N, "rough")
    from tracer_states import global_state
    return global_state(WIDE_F[phys][0] - 4, N, "rough")


def _wide_single(phys, N, t, steps=3):
    from rough_states import install
    make = WIDE[phys]
    F, ng = WIDE_F[phys]
    assert (make().F, make().halo) == (F, ng)
    single = Engine(make(), TileLayout(N, t, 1, ng=ng), grid=CubedSphereGrid(N), dt=300.0)
    install(single, _wide_start(phys, N))
    single.step(steps)
    return single


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, N, t, staged, outdir, limiter=None):
    import torch.distributed as dist
    from stsphere.parallel.comm import TorchDistTransport
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        phys = ShallowWater("tc5") if limiter is None else ShallowWater("tc5", limiter=limiter)
        L = TileLayout(N, t, world, ng=phys.halo)
        tr = TorchDistTransport(L.plan(rank), 4, torch.float64, torch.device("cpu"), staged=staged)
        e = Engine(phys, L, rank, transport=tr, dt=300.0)
        e.step(3)
        np.save(os.path.join(outdir, f"r{rank}.npy"), e.tiles_view().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,t,staged", [(2, 1, False), (3, 1, True), (4, 2, False), (6, 1, False), (6, 1, True),
                                            (8, 2, False), (8, 2, True)])
def test_gloo_multiprocess_equals_single(world, t, staged):
    _gloo_equals_single(8, world, t, staged, None)


@pytest.mark.parametrize("world,t,staged", [(2, 1, False), (4, 2, True), (8, 2, False)])
def test_gloo_multiprocess_equals_single_ppm(world, t, staged):
    """Three ghost layers through real messages.  N = 12: carried corners need
    n >= 2 ng, so t = 2 needs n = 6."""
    _gloo_equals_single(12, world, t, staged, 4)


def _gloo_equals_single(N, world, t, staged, limiter):
    out = tempfile.mkdtemp()
    mp.spawn(_worker, args=(world, _free_port(), N, t, staged, out, limiter), nprocs=world, join=True)
    phys = ShallowWater("tc5") if limiter is None else ShallowWater("tc5", limiter=limiter)
    ng = phys.halo
    L = TileLayout(N, t, world, ng=ng)
    g = CubedSphereGrid(N)
    single = Engine(phys, TileLayout(N, t, 1, ng=ng), grid=g, dt=300.0)
    single.step(3)
    from stsphere.engine import assemble_global
    for f in range(4):
        glob = assemble_global(L, {r: np.load(os.path.join(out, f"r{r}.npy"))[f] for r in range(world)})
        assert np.array_equal(glob, single.global_field(f))


def _worker_wide(rank, world, port, N, t, staged, outdir, phys):
    import torch.distributed as dist
    from rough_states import install
    from stsphere.parallel.comm import TorchDistTransport
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ph = WIDE[phys]()
        L = TileLayout(N, t, world, ng=ph.halo)
        tr = TorchDistTransport(L.plan(rank), ph.F, torch.float64, torch.device("cpu"), staged=staged)
        e = Engine(ph, L, rank, transport=tr, dt=300.0)
        install(e, _wide_start(phys, N))
        e.step(3)
        np.save(os.path.join(outdir, f"r{rank}.npy"), e.tiles_view().numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("phys,world,t,staged", [("trc_mc", 2, 1, False), ("trc_mc", 3, 1, True), ("trc_mc", 4, 2, False),
                                                 ("trc_ppm", 2, 2, False), ("trc_ppm", 3, 1, False), ("trc_ppm", 4, 2, True),
                                                 ("layers", 2, 1, True), ("layers", 3, 1, False), ("layers", 4, 2, False)])
def test_gloo_multiprocess_equals_single_wide_rows(phys, world, t, staged, tmp_path):
    """Receive rows of 5, 6 and 8 values through real messages, from the rough
    states: every field of every rank count bitwise equal to one rank.  N = 12:
    the PPM tracers' carried corners need n >= 2 ng at t = 2."""
    from stsphere.engine import assemble_global
    N = 12
    out = str(tmp_path)
    mp.spawn(_worker_wide, args=(world, _free_port(), N, t, staged, out, phys), nprocs=world, join=True)
    single = _wide_single(phys, N, t)
    F, ng = WIDE_F[phys]
    L = TileLayout(N, t, world, ng=ng)
    for f in range(F):
        glob = assemble_global(L, {r: np.load(os.path.join(out, f"r{r}.npy"))[f] for r in range(world)})
        assert np.isfinite(glob).all() and np.array_equal(glob, single.global_field(f)), (phys, f)


def _wide_loopback(phys, t, N=12, steps=3):
    """The loopback engine of a WIDE physics after ``steps`` steps from the rough state."""
    from rough_states import install
    from stsphere.parallel.comm import LoopbackTransport
    F, ng = WIDE_F[phys]
    L = TileLayout(N, t, 1, ng=ng, loopback=True)
    p = L.plan(0)
    assert p.recv_peers == [0] and (p.ghost_map < 0).all() and p.ghost_map.shape[2] == ng
    lb = Engine(WIDE[phys](), L, grid=CubedSphereGrid(N), dt=300.0,
                transport=LoopbackTransport(p, F, torch.float64, torch.device("cpu")))
    assert lb.transport.recv.shape == (p.num_recv, F)
    install(lb, _wide_start(phys, N))
    lb.step(steps)
    return lb


@pytest.mark.parametrize("phys,t", [("trc_mc", 2), ("trc_mc", 1), ("trc_ppm", 2), ("trc_ppm", 1), ("layers", 2), ("layers", 1)])
def test_loopback_layout_equals_single_wide_rows(phys, t):
    """Every ghost of every column comes out of a receive buffer with rows of F = 5, 6 or 8 values."""
    single, lb = _wide_single(phys, 12, t), _wide_loopback(phys, t)
    for f in range(WIDE_F[phys][0]):
        assert torch.equal(single.tiles_view()[f], lb.tiles_view()[f]), (phys, single.physics.fields[f])


@pytest.mark.parametrize("phys,cols", [("trc_mc", (4, 5)), ("layers", (0, 4))])
def test_loopback_comparison_notices_a_misplaced_column(phys, cols, monkeypatch):
    """The comparison above is sensitive to what it is there for: with two
    columns of the receive buffer swapped on delivery (hq_0 and hq_1; h_0 and
    h_1) both fields differ from one rank, after one step already."""
    from stsphere.parallel.comm import LoopbackTransport
    finish = LoopbackTransport.finish

    def swapped(self):
        recv = finish(self)
        recv[:, list(cols)] = recv[:, list(cols[::-1])]
        return recv

    single = _wide_single(phys, 12, 2, steps=1)
    monkeypatch.setattr(LoopbackTransport, "finish", swapped)
    lb = _wide_loopback(phys, 2, steps=1)
    for f in cols:
        assert torch.isfinite(lb.tiles_view()[f]).all()
        assert not torch.equal(single.tiles_view()[f], lb.tiles_view()[f]), (phys, single.physics.fields[f])


def test_loopback_layout_equals_single():
    _loopback_equals_single("swe_mc", 2)


@pytest.mark.parametrize("phys,t", [("swe_ppm", 2), ("swe_ppm", 1), ("adv_ppm", 2)])
def test_loopback_layout_equals_single_ppm(phys, t):
    """ng = 3: all three strip layers and the 3 x 3 carried corners come out of the receive buffer."""
    _loopback_equals_single(phys, t)


def _loopback_equals_single(phys, t):
    from stsphere.parallel.comm import LoopbackTransport
    N = 12
    g = CubedSphereGrid(N)
    make = PHYSICS[phys]
    ng = make().halo
    L = TileLayout(N, t, 1, ng=ng, loopback=True)
    p = L.plan(0)
    assert p.recv_peers == [0] and p.send_peers == [0] and (p.ghost_map < 0).all() and (p.push_map < 0).all()
    assert p.ghost_map.shape[2] == ng and (t == 1 or p.remote_corners().sum() > 0) and (p.corner_push < 0).all()
    single = Engine(make(), TileLayout(N, t, 1, ng=ng), grid=g)
    lb = Engine(make(), L, grid=g, dt=single.dt,
                transport=LoopbackTransport(p, make().F, torch.float64, torch.device("cpu")))
    single.step(3)
    lb.step(3)
    assert torch.equal(single.tiles_view(), lb.tiles_view())
