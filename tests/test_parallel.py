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
from stsphere.models.swe import ShallowWater
from stsphere.models.advection import Advection
from stsphere.parallel.layout import TileLayout


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
