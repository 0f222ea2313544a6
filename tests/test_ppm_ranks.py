"""Three-layer halos across ranks (GPU): PPM (limiter 4) is the only scheme
with ``ng = 3`` (two interpolated panel-edge layers, 3 x 3 carried tile-corner
ghosts), and a rank of a multi-GPU PPM run is the block stage kernel plus one
of the transports (the fused step and the streaming stage refuse PPM).  Here
every such path runs on one GPU:

* virtual ranks: the receive-buffer gather on the boundary block list beside
  the interior block list (``stage_kernel<.., 4, true, true, false>`` and
  ``<.., 4, false, true, false>``),
* the direct xGMI exchange (``<.., 4, false, false, true>``) on the loopback
  layout and across processes,

for shallow water (F = 4) and tracer advection (F = 1), on the tile sizes where
the 3-wide window ring decides something:

    C24 t=2 (n 12)  partial 16x16 block, every block a boundary block, 3 x 3
                    carried corners at tile corners inside panels
    C32 t=2 (n 16)  exactly one full block per tile: PPM still takes the
                    block-wide panel-edge fix-up
    C34 t=1 (n 34)  the block at x0 = 16 reaches the ghost strip only with
                    window layer 3; the last block is 2 cells wide
    C36 t=2 (n 18)  block 0 reaches the far ghost strip only with layer 3
    C48 t=1 (n 48)  3 x 3 blocks: one interior block per tile, so the interior
                    list launch runs beside the boundary list

Every case prints what it measured; profiles/ppm_ranks/README.md records it."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from rough_states import global_of, grid_of, increment_error, install, local_of
from test_hip_kernels import PHYS, _relerr
from test_rough_kernels import BOUND, _engine as _rough_engine, _global as _rough_global, _reference as _rough_reference
from test_xgmi import _free_port, _worker
from stsphere.engine import Engine, VirtualCluster, assemble_global
from stsphere.models.swe import ShallowWater
from stsphere.ops.hip_compute import block_supports
from stsphere.parallel.comm import NativeBuffers
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

STEPS = 4


@functools.lru_cache(maxsize=None)
def _oracle(name, N, t):
    """The fp64 PyTorch engine (one rank) after STEPS steps: computed once per
    case, shared by every block shape and rank count, never stepped again."""
    ref = Engine(PHYS[name](), TileLayout(N, t, 1, ng=PHYS[name]().halo), grid=grid_of(N), device="cuda",
                 backend="torch")
    _start(name, N, [ref])
    ref.step(STEPS)
    torch.cuda.synchronize()
    return ref


def _start(name, N, engines):
    """The start state of the virtual-rank cases.  Shallow water: TC5 as set
    up (flow everywhere).  Advection: the ``scalar`` class of rough_states.py,
    because the cosine bell is zero on most of the sphere and a two-rank
    boundary never sees it (a kernel that dropped ghost layer 3 passed)."""
    if name == "adv_ppm":
        for e in engines:
            install(e, _rough_global("adv", N, "scalar"))


def _single(name, N, t, block, dt, **kw):
    return Engine(PHYS[name](), TileLayout(N, t, 1, ng=PHYS[name]().halo), grid=grid_of(N), device="cuda",
                  backend="hip", block=block, dt=dt, **kw)


def _cluster(name, N, t, R, block, dt):
    ng = PHYS[name]().halo
    assert ng == 3
    return VirtualCluster(PHYS[name], TileLayout(N, t, R, ng=ng), grid=grid_of(N), device="cuda", backend="hip",
                          block=block, dt=dt)


def _close_to_single(a, b, what):
    """The bound of test_remote_ghost_path_virtual_ranks, per field, on the
    global fields [F, 6, N, N]; prints the largest difference and whether the
    two states are bitwise equal."""
    assert torch.isfinite(a).all() and torch.isfinite(b).all(), what
    worst = 0.0
    for f in range(a.shape[0]):
        d, m = float((a[f] - b[f]).abs().max()), float(a[f].abs().max())
        worst = max(worst, d / max(m, 1e-300))
        assert d <= 1e-12 * max(1.0, m), (what, f, d, m)
    print(f"PPMRANKS {what}: ranks vs one rank {worst:.2e} of the field maximum, bitwise {bool(torch.equal(a, b))}")


def _global_relerr(ref, G):
    """``_relerr`` of a global field [F, 6, N, N] against the one-rank oracle."""
    a = global_of(ref).reshape(G.shape[0], -1)
    return float(((a - G.reshape(G.shape[0], -1)).abs().amax(1) / a.abs().amax(1).clamp_min(1e-30)).max())


# ---- a. virtual ranks: the receive-buffer gather and the two block lists ---------------------
VIRTUAL = [(24, 2, 2, (16, 16)), (24, 2, 8, (16, 16)), (34, 1, 2, (16, 16)), (48, 1, 6, (16, 16)),
           (36, 2, 8, (16, 16)), (24, 2, 8, (16, 8)), (24, 2, 8, (8, 16)), (24, 2, 8, (32, 8))]


@pytest.mark.parametrize("name", ["swe_ppm", "adv_ppm"])
@pytest.mark.parametrize("N,t,R,block", VIRTUAL, ids=[f"C{N}-t{t}-R{R}-{b[0]}x{b[1]}" for N, t, R, b in VIRTUAL])
def test_virtual_ranks_ppm(N, t, R, block, name):
    ref = _oracle(name, N, t)
    single = _single(name, N, t, block, ref.dt)
    vc = _cluster(name, N, t, R, block, ref.dt)
    for e in vc.engines:
        assert e.compute.remote and (e.compute.bx, e.compute.by) == block
        if (N, t) == (48, 1):       # both launches of a stage run
            assert e.compute.blk_interior.numel() > 0 and e.compute.blk_boundary.numel() > 0
    _start(name, N, [single] + vc.engines)
    single.step(STEPS)
    vc.step(STEPS)
    torch.cuda.synchronize()
    what = f"virtual {name} C{N} t={t} R={R} block {block[0]}x{block[1]}"
    a, b = global_of(single), global_of(vc.engines)
    _close_to_single(a, b, what)
    e1, eR = _relerr(ref, single), _global_relerr(ref, b)
    print(f"PPMRANKS {what}: against the oracle one rank {e1:.2e}, {R} ranks {eR:.2e}")
    assert e1 < 1e-11 and eR < 1e-11


@pytest.mark.parametrize("name", ["swe_ppm", "adv_ppm"])
def test_virtual_ranks_ppm_chosen_block(name):
    """``block=None``: what choose_block gives a rank of an 8-rank C24 run (3
    tiles of 12 x 12) must be a block shape PPM can run, not the streaming stage."""
    N, t, R = 24, 2, 8
    ref = _oracle(name, N, t)
    vc = _cluster(name, N, t, R, None, ref.dt)
    shapes = {(e.compute.bx, e.compute.by) for e in vc.engines}
    assert len(shapes) == 1
    bx, by = shapes.pop()
    print(f"PPMRANKS chosen block {name} C{N} t={t} R={R}: {bx}x{by}")
    assert block_supports(bx, by, 4) and not any(e.compute.march for e in vc.engines)
    single = _single(name, N, t, (bx, by), ref.dt)
    _start(name, N, [single] + vc.engines)
    single.step(STEPS)
    vc.step(STEPS)
    torch.cuda.synchronize()
    b = global_of(vc.engines)
    _close_to_single(global_of(single), b, f"virtual {name} C{N} t={t} R={R} chosen block {bx}x{by}")
    assert _global_relerr(ref, b) < 1e-11


# ---- b. rough states across ranks --------------------------------------------------------------
class _RankOf:
    """The one-rank oracle's state (or start state) cut to one rank's tiles, in
    the shape ``increment_error`` reads an engine."""

    def __init__(self, engine, G):
        self.plan, self.geo, self.physics = engine.plan, engine.geo, engine.physics
        self._q = local_of(engine, G)

    def tiles_view(self):
        return self._q


@pytest.mark.parametrize("N,t,R", [(24, 2, 2), (24, 2, 8), (34, 1, 2)])
def test_remote_ghost_path_on_rough_ppm(N, t, R):
    """The PPM twin of test_remote_ghost_path_on_rough: every arm of the PPM
    limiter on both sides of every rank boundary, two steps."""
    steps, block = 2, (16, 16)
    ref, _ = _rough_reference("tc5", N, t, 4, "rough", "ssprk3", steps)
    single, _ = _rough_engine("tc5", N, t, 4, "rough", backend="hip", block=block, dt=ref.dt)
    vc = VirtualCluster(lambda: ShallowWater("tc5", limiter=4), TileLayout(N, t, R, ng=3), grid=grid_of(N),
                        device="cuda", backend="hip", block=block, dt=ref.dt)
    G0 = _rough_global("tc5", N, "rough")
    q0 = [install(e, G0) for e in vc.engines]
    single.step(steps)
    vc.step(steps)
    torch.cuda.synchronize()
    what = f"rough swe_ppm C{N} t={t} R={R}"
    _close_to_single(global_of(single), global_of(vc.engines), what)
    Gref = global_of(ref)
    errs = [increment_error(_RankOf(e, Gref), e, q, block=block, what=f"{what} rank {e.rank}")
            for e, q in zip(vc.engines, q0)]
    print(f"PPMRANKS {what}: increment error against the oracle, worst rank per field: "
          + " ".join(f"{max(x[f] for x in errs):.2e}" for f in range(4)))
    for e, q in zip(vc.engines, q0):
        increment_error(_RankOf(e, Gref), e, q, bound=BOUND, block=block, what=f"{what} rank {e.rank}")


# ---- c. the direct xGMI exchange on the loopback layout -----------------------------------------
def _xg_pair(name, N, t, integ, dtype, block):
    a = _single(name, N, t, block, None, integrator=integ, dtype=dtype)
    L = TileLayout(N, t, 1, ng=3, loopback=True)
    b = Engine(PHYS[name](), L, grid=grid_of(N), device="cuda", backend="hip", integrator=integ, dt=a.dt, dtype=dtype,
               block=block, transport=NativeBuffers(L.plan(0), a.physics.F, dtype, torch.device("cuda")))
    assert (a.compute.bx, a.compute.by) == (b.compute.bx, b.compute.by) and not b.compute.march
    return a, b


@pytest.mark.parametrize("N,t,integ,use_graph,dtype,block", [
    pytest.param(24, 2, "ssprk3", True, torch.float64, (16, 16), id="24-2-ssprk3-graph"),
    pytest.param(24, 2, "ssprk3", False, torch.float64, (16, 16), id="24-2-ssprk3-eager"),
    pytest.param(34, 1, "ssprk3", True, torch.float64, (16, 16), id="34-1-ssprk3-graph"),
    pytest.param(32, 2, "rk4", True, torch.float64, (16, 16), id="32-2-rk4-graph"),
    pytest.param(24, 2, "ssprk3", True, torch.float32, (16, 16), id="24-2-ssprk3-graph-fp32"),
    pytest.param(24, 2, "ssprk3", True, torch.float64, None, id="24-2-ssprk3-graph-chosen-block")])
def test_xgmi_loopback_ppm_matches_single(N, t, integ, use_graph, dtype, block):
    """Every ghost of all three layers, and every carried corner, goes through
    the ring: bitwise equal to the one-rank engine of the same dtype."""
    from stsphere.ops.native_runtime import NativeStepper
    from stsphere.ops.xgmi import XgmiHalo
    a, b = _xg_pair("swe_ppm", N, t, integ, dtype, block)
    xg = XgmiHalo(b, timeout_s=1.0)
    assert xg.xp.halo == 3 and xg.xp.push.shape[2] == 3
    ns = NativeStepper(b, use_graph=use_graph, steps_per_graph=4, xgmi=xg)
    a.step(12)
    ns.run(12)
    torch.cuda.synchronize()
    ns.check()
    print(f"PPMRANKS xgmi loopback swe_ppm C{N} t={t} {integ} block {b.compute.bx}x{b.compute.by}: "
          f"max |difference| {float((a.tiles_view() - b.tiles_view()).abs().max()):.2e}")
    assert torch.equal(a.tiles_view(), b.tiles_view())
    assert int(xg.epoch.min()) == int(xg.epoch.max()) >= 12 * len(b.integ.stages)
    ns.close()
    xg.close()


def test_xgmi_loopback_ppm_advection_and_reprime():
    """F = 1 (the one-value ring record) with three layers, plus a state reset
    mid-run (re-delivery of all three layers and the corners)."""
    from stsphere.ops.native_runtime import NativeStepper
    from stsphere.ops.xgmi import XgmiHalo
    a, b = _xg_pair("adv_ppm", 32, 2, "ssprk3", torch.float64, (16, 16))
    xg = XgmiHalo(b, timeout_s=1.0)
    ns = NativeStepper(b, use_graph=True, steps_per_graph=5, xgmi=xg)
    a.step(5)
    ns.run(5)
    torch.cuda.synchronize()
    assert torch.equal(a.tiles_view(), b.tiles_view())
    q0 = torch.as_tensor(a.physics.initial_state(a.geo), dtype=torch.float64)
    a.set_state(q0)
    b.set_state(q0)
    xg.prime()
    a.step(5)
    ns.run(5)
    torch.cuda.synchronize()
    ns.check()
    assert torch.equal(a.tiles_view(), b.tiles_view())
    ns.close()
    xg.close()


# ---- d. the direct xGMI exchange across processes sharing the GPU --------------------------------
@pytest.mark.parametrize("N,world,t", [(24, 2, 2), (24, 4, 2), (24, 3, 1), (34, 2, 1)])
def test_xgmi_multiprocess_one_gpu_ppm(N, world, t):
    """Real IPC rings between processes.  C34: blocks that reach another
    process's cells only with window layer 3 wait on that peer's granules."""
    steps = 10
    out = tempfile.mkdtemp()
    mp.spawn(_worker, args=(world, _free_port(), N, t, steps, out, None, 1, 4), nprocs=world, join=True)
    single = Engine(ShallowWater("tc5", limiter=4), TileLayout(N, t, 1, ng=3), grid=grid_of(N), device="cuda",
                    backend="hip", dt=200.0)
    single.step(steps)
    L = TileLayout(N, t, world, ng=3)
    for f in range(4):
        glob = assemble_global(L, {r: np.load(os.path.join(out, f"r{r}.npy"))[f] for r in range(world)})
        assert np.isfinite(glob).all() and np.array_equal(glob, single.global_field(f)), f
