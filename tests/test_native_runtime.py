"""Native C++ step runtime (hipGraph + RCCL) on one GPU.

The loopback layout routes every ghost through pack -> RCCL grouped
send/recv (to self) -> receive-buffer gather, i.e. the complete multi-GPU
path, on a single MI355X."""
import functools
import os
import socket

import pytest
import torch

from stsphere.engine import Engine
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater, ShallowWaterTracers
from stsphere.models.advection import Advection
from stsphere.parallel.comm import LoopbackTransport, NativeBuffers
from stsphere.parallel.layout import TileLayout

import layer_states
import tracer_states
from rough_states import grid_of, install

pytestmark = pytest.mark.gpu


def _single(N=24, t=2, phys=lambda: ShallowWater("tc5"), integ="ssprk3"):
    g = CubedSphereGrid(N)
    return g, Engine(phys(), TileLayout(N, t, 1, ng=phys().halo), grid=g, device="cuda", backend="hip", integrator=integ)


# the physics of the loopback transports: MC-limited (two ghost layers), and PPM
# (limiter 4) with three layers and 3 x 3 carried corners in every message
MK = {"swe": lambda: ShallowWater("tc5"), "adv": lambda: Advection(),
      "swe_ppm": lambda: ShallowWater("tc5", limiter=4), "adv_ppm": lambda: Advection(limiter=4),
      # receive rows wider than 4 values: tracers behind (h, M) (F = 4 + NQ; PPM mixing
      # ratios read three ghost layers), two layers (F = 8)
      "trc1": lambda: _tracers(1), "trc3": lambda: _tracers(3), "trc4": lambda: _tracers(4),
      "trc2_ppm": lambda: _tracers(2, tracer_limiter="ppm"), "layers": lambda: layer_states.layer_physics()}
WIDE_F = {"trc1": 5, "trc3": 7, "trc4": 8, "trc2_ppm": 6, "layers": 8}


def _tracers(nq, **kw):
    return ShallowWaterTracers("tc5", tracers=tracer_states.TRACER_SETS[nq], limiter=2, **kw)


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("integ", ["ssprk3", "rk4", "euler"])
def test_native_stepper_matches_engine(use_graph, integ):
    from stsphere.ops.native_runtime import NativeStepper
    g, a = _single(integ=integ)
    _, b = _single(integ=integ)
    ns = NativeStepper(b, use_graph=use_graph, steps_per_graph=4)
    a.step(10)
    ns.run(10)
    torch.cuda.synchronize()
    assert torch.equal(a.tiles_view(), b.tiles_view())
    assert b.step_count == 10
    ns.close()


@pytest.mark.parametrize("integ", ["euler", "ssprk3"])
def test_odd_chunks_keep_runner_and_pool_in_sync(integ):
    """run(3); run(3) == Engine.step(6) even when a chunk is not a multiple of
    the integrator period (euler ping-pongs its buffers: ADVICE r1)."""
    from stsphere.engine import GraphStepper
    from stsphere.ops.native_runtime import NativeStepper
    _, a = _single(integ=integ)
    _, b = _single(integ=integ)
    _, c = _single(integ=integ)
    ns = NativeStepper(b, use_graph=True, steps_per_graph=4)
    gs = GraphStepper(c, steps_per_graph=2)
    a.step(6)
    for _ in range(2):
        ns.run(3)
        gs.run(3)
    torch.cuda.synchronize()
    assert torch.equal(a.tiles_view(), b.tiles_view())
    assert torch.equal(a.tiles_view(), c.tiles_view())
    assert b.step_count == 6 and c.step_count == 6
    ns.close()


def test_short_run_replays_a_graph():
    """run(20) with the default 30-step graph length replays recorded graphs
    only (r1: 20 // 30 = 0 graphs, so every step ran eagerly)."""
    from stsphere.ops.native_runtime import NativeStepper
    _, a = _single()
    _, b = _single()
    ns = NativeStepper(b, use_graph=True, steps_per_graph=30)
    ns.prepare(20)
    assert b.step_count == 0 and torch.equal(a.tiles_view(), b.tiles_view())   # prepare leaves the state alone
    s0 = dict(ns.stats)
    ns.run(20)
    a.step(20)
    torch.cuda.synchronize()
    assert ns.stats["eager_steps"] == s0["eager_steps"]
    assert ns.stats["graph_steps"] - s0["graph_steps"] == 20 and ns.stats["replays"] - s0["replays"] == 1
    assert torch.equal(a.tiles_view(), b.tiles_view())
    ns.run(35)      # one 30-step graph + a 5-step graph
    a.step(35)
    torch.cuda.synchronize()
    assert ns.stats["eager_steps"] == s0["eager_steps"]
    assert torch.equal(a.tiles_view(), b.tiles_view())
    ns.close()


@pytest.fixture(scope="module")
def nccl_comm():
    import torch.distributed as dist
    from stsphere.ops import native_runtime as nr
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    comm = nr.create_nccl_comm(0, 1, 0)
    yield comm
    nr.lib().stsp_nccl_comm_destroy(comm)
    dist.destroy_process_group()


def test_rccl_selftest(nccl_comm):
    from stsphere.ops.native_runtime import nccl_selftest
    nccl_selftest(nccl_comm)


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("phys", ["swe", "adv"])
def test_rccl_loopback_full_multigpu_path(nccl_comm, use_graph, phys):
    _rccl_loopback(nccl_comm, use_graph, phys)


@pytest.mark.parametrize("phys", ["swe_ppm", "adv_ppm"])
def test_rccl_loopback_full_multigpu_path_ppm(nccl_comm, phys):
    """Three ghost layers through pack -> RCCL -> the receive-buffer gather of the PPM stage kernel."""
    _rccl_loopback(nccl_comm, False, phys)


def _rccl_loopback(nccl_comm, use_graph, phys):
    from stsphere.ops.native_runtime import NativeStepper
    mk = MK[phys]
    g, ref = _single(phys=mk)
    L = TileLayout(24, 2, 1, ng=mk().halo, loopback=True)
    p = L.plan(0)
    F = ref.physics.F
    e = Engine(mk(), L, grid=g, device="cuda", backend="hip", dt=ref.dt,
               transport=NativeBuffers(p, F, torch.float64, torch.device("cuda")))
    assert e.compute.remote and e.compute.blk_boundary.numel() > 0
    ns = NativeStepper(e, nccl_comm=nccl_comm, use_graph=use_graph, steps_per_graph=3)
    assert not ns.use_graph      # comm op lists run eagerly (RCCL capture crash, see native_runtime.py)
    ref.step(6)
    ns.run(6)
    torch.cuda.synchronize()
    assert torch.equal(ref.tiles_view(), e.tiles_view())
    ns.close()



@pytest.mark.parametrize("use_graph", [True, False])
def test_ipc_copy_loopback_full_multigpu_path_ppm(use_graph):
    """PPM: three layers and the carried corners in one copy per stage."""
    _ipc_loopback(use_graph, "ssprk3", "swe_ppm")


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("integ", ["ssprk3", "rk4"])
def test_ipc_copy_loopback_full_multigpu_path(use_graph, integ):
    """The IPC copy transport (pack -> one copy kernel into the peer's receive
    slot, which also stores the peer's flag -> interior blocks -> spin-wait
    kernel -> boundary blocks) on the loopback layout, where every ghost
    crosses it: bitwise equal to the single-rank engine, and, unlike the RCCL
    op list, recorded into a graph and replayed."""
    _ipc_loopback(use_graph, integ, "swe")


def _ipc_loopback(use_graph, integ, phys):
    from stsphere.ops.native_runtime import IpcExchange, NativeStepper
    mk = MK[phys]
    g, ref = _single(integ=integ, phys=mk)
    L = TileLayout(24, 2, 1, ng=mk().halo, loopback=True)
    p = L.plan(0)
    e = Engine(mk(), L, grid=g, device="cuda", backend="hip", dt=ref.dt, integrator=integ,
               transport=NativeBuffers(p, ref.physics.F, torch.float64, torch.device("cuda")))
    assert e.compute.remote and e.compute.blk_boundary.numel() > 0
    ipc = IpcExchange(e, IpcExchange.slots_for(e))
    ns = NativeStepper(e, use_graph=use_graph, steps_per_graph=3, ipc=ipc)
    assert ns.use_graph == use_graph
    ref.step(9)
    ns.run(9)
    torch.cuda.synchronize()
    ns.check()
    assert torch.equal(ref.tiles_view(), e.tiles_view())
    if use_graph:
        assert ns.stats["graph_steps"] >= 6 and ns.stats["eager_steps"] <= 3
    ns.close()
    ipc.close()


@pytest.mark.parametrize("phys,dtype", [("adv", torch.float32), ("adv", torch.float64), ("swe", torch.float32),
                                        ("adv_ppm", torch.float32), ("swe_ppm", torch.float32)])
def test_ipc_copy_kernel_word_sizes(phys, dtype):
    """The IPC copy kernel (runtime.cpp::ipc_copy_signal_kernel) copies
    16-byte words when every payload allows, else 4-byte words: one field in
    fp32 (tracer advection) gives payloads that are not 16-byte multiples.
    Each case is bitwise equal to the single-rank engine of the same dtype,
    graph-replayed.  The PPM cases carry three layers per strip."""
    from stsphere.ops.native_runtime import IpcExchange, NativeStepper
    mk = MK[phys]
    ng = mk().halo
    g = CubedSphereGrid(24)
    ref = Engine(mk(), TileLayout(24, 2, 1, ng=ng), grid=g, dtype=dtype, device="cuda", backend="hip")
    L = TileLayout(24, 2, 1, ng=ng, loopback=True)
    F = ref.physics.F
    e = Engine(mk(), L, grid=g, dtype=dtype, device="cuda", backend="hip", dt=ref.dt,
               transport=NativeBuffers(L.plan(0), F, dtype, torch.device("cuda")))
    ipc = IpcExchange(e, IpcExchange.slots_for(e))
    ns = NativeStepper(e, use_graph=True, steps_per_graph=3, ipc=ipc)
    ref.step(6)
    ns.run(6)
    torch.cuda.synchronize()
    ns.check()
    assert torch.equal(ref.tiles_view(), e.tiles_view())
    ns.close()
    ipc.close()


# ---- receive rows of 5 to 8 values: tracers and layers through the loopback transports ----------
WIDE_N, WIDE_T, WIDE_STEPS = 24, 2, 6       # n = 12: partial blocks, tile sides on and inside panel edges, carried corners


def _wide_engine(phys, dtype, block, dt=None, transport=None):
    """An engine of MK[phys] on C24 t = 2 from the rough state of tracer_states.py
    / layer_states.py (the cap and the bell are zero on most of the sphere; the
    rough states put signal into every column of every receive row).
    ``transport``: a transport class for the loopback layout, None for the plain
    one-rank layout."""
    ph = MK[phys]()
    F = WIDE_F[phys]
    assert ph.F == F
    L = TileLayout(WIDE_N, WIDE_T, 1, ng=ph.halo, loopback=transport is not None)
    tr = None if transport is None else transport(L.plan(0), F, dtype, torch.device("cuda"))
    e = Engine(ph, L, grid=grid_of(WIDE_N), dtype=dtype, device="cuda", backend="hip", block=block, dt=dt, transport=tr)
    assert (e.compute.bx, e.compute.by) == block and not e.compute.march
    if transport is not None:
        assert e.compute.remote and e.compute.blk_boundary.numel() > 0 and tuple(tr.recv.shape) == (L.plan(0).num_recv, F)
    G = layer_states.global_state(WIDE_N, "rough") if phys == "layers" else tracer_states.global_state(F - 4, WIDE_N, "rough")
    install(e, G)
    return e


@functools.lru_cache(maxsize=None)
def _wide_reference(phys, dtype, block):
    """(dt, state of the loopback layout stepped from Python, state of the one-rank
    engine) after WIDE_STEPS steps: computed once per case, shared by the IPC
    (graph, eager) and RCCL tests.  The first is the transports' contract: same
    kernels, same instantiation, same block lists, the receive buffer filled by
    ``LoopbackTransport`` (a torch copy of the packed rows).  The second has no
    receive buffer at all (the plain instantiation of the stage kernel)."""
    one = _wide_engine(phys, dtype, block)
    lb = _wide_engine(phys, dtype, block, dt=one.dt, transport=LoopbackTransport)
    q0 = one.tiles_view().clone()
    one.step(WIDE_STEPS)
    lb.step(WIDE_STEPS)
    torch.cuda.synchronize()
    assert torch.isfinite(one.tiles_view()).all()
    assert all(not torch.equal(q0[f], one.tiles_view()[f]) for f in range(q0.shape[0]))      # every column moved
    return one.dt, lb.tiles_view().clone(), one.tiles_view().clone()


def _wide_assert(phys, dtype, block, how, e):
    """Assertion 1 (the transport's contract), then assertion 2 (the one-rank engine)."""
    _, lb, one = _wide_reference(phys, dtype, block)
    got = e.tiles_view()
    what = f"{how} {phys} {str(dtype).split('.')[-1]} block {block[0]}x{block[1]}"
    d1 = max(float((got[f] - lb[f]).abs().max() / lb[f].abs().max()) for f in range(got.shape[0]))
    d2 = max(float((got[f] - one[f]).abs().max() / one[f].abs().max()) for f in range(got.shape[0]))
    print(f"WIDEROWS {what}: against the loopback layout stepped from Python {d1:.2e}, "
          f"against one rank {d2:.2e} of the field maximum")
    for f, name in enumerate(e.physics.fields):
        assert torch.equal(got[f], lb[f]), f"{what}: field {name} differs from the same layout stepped from Python"
    for f, name in enumerate(e.physics.fields):
        assert torch.equal(got[f], one[f]), f"{what}: field {name} differs from the one-rank engine"


WIDE_CASES = [pytest.param("trc1", torch.float64, (16, 8), id="trc1-fp64-16x8"),
              pytest.param("trc3", torch.float64, (16, 8), id="trc3-fp64-16x8"),
              pytest.param("trc3", torch.float64, (16, 16), id="trc3-fp64-16x16"),
              pytest.param("trc4", torch.float64, (16, 8), id="trc4-fp64-16x8"),
              pytest.param("trc1", torch.float32, (16, 8), id="trc1-fp32-16x8"),
              pytest.param("trc2_ppm", torch.float64, (16, 8), id="trc2_ppm-fp64-16x8"),
              pytest.param("layers", torch.float64, (16, 8), id="layers-fp64-16x8"),
              pytest.param("layers", torch.float64, (16, 16), id="layers-fp64-16x16"),
              pytest.param("layers", torch.float32, (16, 8), id="layers-fp32-16x8")]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("phys,dtype,block", WIDE_CASES)
def test_ipc_copy_loopback_wide_rows(phys, dtype, block, use_graph):
    """Tracers and layers through pack (F = 5 .. 8) -> the IPC copy kernel with
    payloads of ``cnt * F * esize`` bytes and slots sized by F -> the REMOTE
    instantiation of their stage kernels reading the receive slot: bitwise
    equal to the same layout stepped from Python, and to the one-rank engine.
    The loopback plan has one peer at offset 0 and 1920 or 2592 rows, so every
    payload here is a multiple of 16 bytes (the copy kernel's 16-byte words)."""
    from stsphere.ops.native_runtime import IpcExchange, NativeStepper
    dt = _wide_reference(phys, dtype, block)[0]
    e = _wide_engine(phys, dtype, block, dt=dt, transport=NativeBuffers)
    ipc = IpcExchange(e, IpcExchange.slots_for(e))
    try:
        assert ipc.F == WIDE_F[phys] and ipc.slot_bytes >= e.plan.num_recv * ipc.F * ipc.esize
        assert list(e.plan.send_offsets) == [0] and e.plan.send_counts[0] * ipc.F * ipc.esize % 16 == 0
        ns = NativeStepper(e, use_graph=use_graph, steps_per_graph=3, ipc=ipc)
        try:
            assert ns.use_graph == use_graph
            ns.run(WIDE_STEPS)
            torch.cuda.synchronize()
            ns.check()
            if use_graph:
                assert ns.stats["graph_steps"] >= WIDE_STEPS and ns.stats["eager_steps"] <= 3, ns.stats
            _wide_assert(phys, dtype, block, "ipc graph" if use_graph else "ipc eager", e)
        finally:
            ns.close()
    finally:
        ipc.close()


@pytest.mark.parametrize("phys,dtype,block", WIDE_CASES)
def test_rccl_loopback_wide_rows(nccl_comm, phys, dtype, block):
    """The same cases through the grouped RCCL send / receive with ``slot_elems = F``."""
    from stsphere.ops.native_runtime import NativeStepper
    dt = _wide_reference(phys, dtype, block)[0]
    e = _wide_engine(phys, dtype, block, dt=dt, transport=NativeBuffers)
    ns = NativeStepper(e, nccl_comm=nccl_comm, use_graph=False, steps_per_graph=3)
    try:
        assert not ns.use_graph
        ns.run(WIDE_STEPS)
        torch.cuda.synchronize()
        _wide_assert(phys, dtype, block, "rccl", e)
    finally:
        ns.close()
