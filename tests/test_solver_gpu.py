"""Solver on the GPU: the native runtime path (graph replay), the SPMD path
with the direct xGMI exchange (ranks sharing one GPU, STSP_SHARE_GPU=1), and
checkpoint/restore with re-delivery of the remote ghosts."""
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from stsphere.driver import Solver

pytestmark = pytest.mark.gpu


def _cfg(nd, t, N=24, out="run", limiter="mc", comm="auto", device="gpu", dt=150.0):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": device},
            "grid": {"N": N, "halo": 2, "dtype": "float64"},
            "physics": {"model": "swe", "case": "tc5", "limiter": limiter},
            "time": {"integrator": "ssprk3", "dt": dt},
            "io": {"output_dir": out},
            "runtime": {"comm": comm, "steps_per_graph": 4}}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("limiter", ["mc", "ppm"])
def test_single_gpu_solver_matches_cpu(limiter, tmp_path):
    g = Solver(_cfg(1, 2, out=str(tmp_path / "g"), limiter=limiter), verbose=False)
    g.initialize()
    c = Solver(_cfg(1, 2, out=str(tmp_path / "c"), limiter=limiter, device="cpu"), verbose=False)
    c.initialize()
    g.run(nsteps=9)
    c.run(nsteps=9)
    a, b = g.gather_global(), c.gather_global()
    err = max(np.abs(a[f] - b[f]).max() / np.abs(b[f]).max() for f in range(4))
    assert err < 1e-11
    assert type(g.runner).__name__ == "NativeStepper"


def _spmd_worker(rank, world, port, t, outdir, comm, fused="auto", fail_xgmi=False, limiter="mc"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), STSP_SHARE_GPU="1")
    if fail_xgmi:
        os.environ["STSP_FAIL_XGMI"] = "1"     # every ring setup raises: the chain lands on ipc
    import torch.distributed as dist
    try:
        c = _cfg(world, t, out=os.path.join(outdir, "run"), comm="xgmi" if fail_xgmi else comm, limiter=limiter)
        c["runtime"]["fused"] = fused
        s = Solver(c, verbose=False)
        s.initialize()
        s.run(nsteps=6)
        assert s.comm == comm, s.comm
        # the default SPMD runtime is the fused step with the xGMI ring inside
        # it (every block of the rank's share resident); "off", or another
        # exchange: stage kernels (ipc: graph-replayed IPC copies)
        # (the fused step refuses PPM: "auto" falls back to the stage kernels)
        assert (s.fused is not None) == (fused != "off" and comm == "xgmi" and not fail_xgmi
                                         and limiter != "ppm"), s.fused
        if comm == "ipc":
            assert s.runner.use_graph and s.runner.stats["graph_steps"] > 0, s.runner.stats
        s.save_checkpoint()
        s.run(nsteps=4)
        a = s.gather_global()
        s.restore_checkpoint(os.path.join(outdir, "run", "checkpoints", "00000006"))
        s.run(nsteps=4)
        b = s.gather_global()
        if rank == 0:
            np.save(os.path.join(outdir, "a.npy"), a)
            np.save(os.path.join(outdir, "b.npy"), b)
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.parametrize("world,t,fused,comm", [(2, 1, "auto", "xgmi"), (4, 2, "auto", "xgmi"), (2, 1, "off", "xgmi"),
                                               (2, 2, "off", "ipc")])
def test_spmd_xgmi_solver_matches_single_and_restarts(world, t, fused, comm, tmp_path):
    """SPMD ranks sharing one GPU with the default configuration take the
    fused step (xGMI ring inside the kernel); the one-GPU reference runs the
    same kernels (the fused step with the ranks' block size, or the stage
    kernels with fused = off), so the states agree bitwise, restart included."""
    out = str(tmp_path)
    mp.spawn(_spmd_worker, args=(world, _free_port(), t, out, comm, fused), nprocs=world, join=True)
    c = _cfg(1, t, out=str(tmp_path / "ref"))
    c["runtime"]["fused"] = fused
    ref = Solver(c, verbose=False)
    ref.initialize()
    ref.run(nsteps=10)
    if fused != "off":
        from stsphere.ops.fused import fused_block
        n = ref.layout.n
        B_rank = fused_block(n, 6 * t * t // world, torch.cuda.get_device_properties(0).multi_processor_count // world)
        assert ref.fused is not None and ref.fused.plan.B == B_rank, (ref.fused, B_rank)
    r = ref.gather_global()
    a = np.load(os.path.join(out, "a.npy"))
    b = np.load(os.path.join(out, "b.npy"))
    assert np.array_equal(a, r)      # same kernels, same order: bitwise
    assert np.array_equal(b, r)      # restart from step 6 re-delivers the remote ghosts


@pytest.mark.parametrize("world,t", [(2, 1), (4, 2)])
def test_spmd_xgmi_solver_ppm_takes_the_stage_kernels(world, t, tmp_path):
    """PPM (three ghost layers) through the Solver with the default runtime:
    the fused step refuses PPM, so ``fused: auto`` must fall back to the stage
    kernels with the direct xGMI exchange (the worker asserts ``s.fused is None``
    and ``s.comm == "xgmi"``), bitwise equal to one GPU with ``fused: off``,
    restart from the step-6 checkpoint included."""
    out = str(tmp_path)
    mp.spawn(_spmd_worker, args=(world, _free_port(), t, out, "xgmi", "auto", False, "ppm"), nprocs=world, join=True)
    c = _cfg(1, t, out=str(tmp_path / "ref"), limiter="ppm")
    c["runtime"]["fused"] = "off"
    ref = Solver(c, verbose=False)
    ref.initialize()
    ref.run(nsteps=10)
    assert ref.fused is None
    r = ref.gather_global()
    assert np.isfinite(r).all()
    assert np.array_equal(np.load(os.path.join(out, "a.npy")), r)
    assert np.array_equal(np.load(os.path.join(out, "b.npy")), r)


@pytest.mark.parametrize("fused", ["auto", "off"])
def test_spmd_solver_falls_back_to_ipc_when_the_rings_fail(fused, tmp_path):
    """Transport chain xgmi -> ipc -> rccl: with every direct-ring setup
    refused (STSP_FAIL_XGMI=1, as on a node without peer IPC) the Solver lands
    on the graph-captured IPC copy transport on every rank, bitwise equal to
    one GPU running the stage kernels."""
    out = str(tmp_path)
    mp.spawn(_spmd_worker, args=(2, _free_port(), 1, out, "ipc", fused, True), nprocs=2, join=True)
    c = _cfg(1, 1, out=str(tmp_path / "ref"))
    c["runtime"]["fused"] = "off"
    ref = Solver(c, verbose=False)
    ref.initialize()
    ref.run(nsteps=10)
    r = ref.gather_global()
    assert np.array_equal(np.load(os.path.join(out, "a.npy")), r)
    assert np.array_equal(np.load(os.path.join(out, "b.npy")), r)


def test_tc1_norms_on_the_hip_path_match_reference_and_converge():
    """Williamson TC1 (alpha = pi/4), one revolution on the fused gfx950 stage
    kernel at C48 and C96: the error norms equal the PyTorch reference run's
    and the l2 error converges (CPU reference: 0.175 -> 0.060, order 1.54)."""
    import math
    from stsphere.engine import Engine
    from stsphere.models.advection import Advection
    from stsphere.models.errors import convergence_order, williamson_norms
    from stsphere.models.geometry import DAY, CubedSphereGrid
    from stsphere.parallel.layout import TileLayout
    errs = []
    for N in (48, 96):
        g = CubedSphereGrid(N)
        ph = Advection(alpha=math.pi / 4)
        L = TileLayout(N, 2, 1, ng=2)
        hip = Engine(ph, L, grid=g, device="cuda", backend="hip")
        n = int(math.ceil(12 * DAY / hip.dt))
        hip.dt = 12 * DAY / n
        hip.step(n)
        nr = williamson_norms(hip.global_field(0), ph.exact(g, hip.time), g.areas())
        if N == 48:
            ref = Engine(ph, L, grid=g, device="cuda", backend="torch", dt=hip.dt)
            ref.step(n)
            nref = williamson_norms(ref.global_field(0), ph.exact(g, ref.time), g.areas())
            assert all(abs(nr[k] - nref[k]) < 1e-9 for k in nr), (nr, nref)
        errs.append(nr["l2"])
    assert errs[1] < 0.07 and convergence_order(errs, (48, 96)) > 1.4, errs


def test_solver_run_replays_graphs_for_io_intervals(tmp_path):
    """Solver.run with history / metrics / watchdog intervals: every step is a
    graph replay (chunks follow the intervals, graphs are recorded before the
    clock starts), history frames are written asynchronously, and the state
    equals an engine stepped the same number of steps."""
    from stsphere.utils.history import read_history, read_metrics
    c = _cfg(1, 2, N=48, out=str(tmp_path))
    c["io"].update(history_interval=12, metrics_interval=6)
    c["runtime"].update(watchdog_interval=6, steps_per_graph=30, fused="off")   # the stage path's graphs
    s = Solver(c, verbose=False)
    s.initialize()
    out = s.run(nsteps=40)
    st = s.runner.stats
    assert st["eager_steps"] == 0 and st["graph_steps"] == 40, st
    assert out["setup_s"] > 0 and out["steps_run"] == 40
    ref = Solver(dict(c, runtime={"graph": False}, io={"output_dir": str(tmp_path / "ref")}), verbose=False)
    ref.initialize()
    ref.step(40)
    assert np.array_equal(s.gather_global(), ref.gather_global())
    from stsphere.utils import zarr_lite
    h = read_history(str(tmp_path / "history.zarr"), "h")
    t = zarr_lite.read_array(str(tmp_path / "history.zarr"), "time")
    assert h.shape[0] == 4 and np.isfinite(h).all() and np.allclose(t, np.arange(4) * 12 * s.dt)
    assert [r["step"] for r in read_metrics(str(tmp_path / "metrics.jsonl"))][-1] == 40


def test_solver_run_uses_fused_multi_step_launches(tmp_path):
    """Solver.run at C96 TC5 (tiles of 48, B = 16) steps with the fused
    SSP-RK3 kernel: chunks between history / checkpoint / metrics / watchdog
    intervals are whole multi-step launches (direct, no graph), the history and
    checkpoints are written, and the state equals the launch-per-stage path
    (runtime.fused = off) to 1e-11."""
    from stsphere.utils import checkpoint as ckpt
    from stsphere.utils.history import read_history
    c = _cfg(1, 2, N=96, out=str(tmp_path / "f"), dt=None)
    c["time"].pop("dt")
    c["io"].update(history_interval=20, metrics_interval=10, checkpoint_interval=40)
    c["runtime"].update(watchdog_interval=10)
    s = Solver(c, verbose=False)
    s.initialize()
    out = s.run(nsteps=80)
    assert out["runtime"] == "fused", out
    st = s.runner.stats
    assert st["direct_steps"] == 80 and st["graph_steps"] == 0 and st["eager_steps"] == 0, st
    assert st["launches"] == 8, st             # chunks of 10 steps: one 10-step launch each
    s.runner.check()
    c2 = _cfg(1, 2, N=96, out=str(tmp_path / "s"), dt=s.dt)
    c2["runtime"].update(fused="off")
    r = Solver(c2, verbose=False)
    r.initialize()
    o2 = r.run(nsteps=80)
    assert o2["runtime"] == "native"
    a, b = s.gather_global(), r.gather_global()
    err = max(np.abs(a[f] - b[f]).max() / np.abs(b[f]).max() for f in range(4))
    assert err < 1e-11, err
    h = read_history(str(tmp_path / "f" / "history.zarr"), "h")
    assert h.shape[0] == 5 and np.isfinite(h).all()
    assert ckpt.list_checkpoints(s.checkpoint_root())[-1] == 80


def test_solver_run_raises_when_a_fused_wait_times_out(tmp_path, monkeypatch):
    """a timed-out in-launch producer wait sets the kernel's error
    word and the state can no longer be trusted; Solver.run must raise (after
    its pending host work) instead of returning as if the run succeeded.  A
    zero wait bound makes the first wait that polls at all time out."""
    import stsphere.ops.fused as F
    orig = F.FusedKernel.__init__

    def init_zero_timeout(self, engine, B=None, timeout_s=2.0, group=None):
        orig(self, engine, B=B, timeout_s=0.0, group=group)

    monkeypatch.setattr(F.FusedKernel, "__init__", init_zero_timeout)
    s = Solver(_cfg(1, 2, out=str(tmp_path / "run")), verbose=False)
    s.initialize()
    with pytest.raises(RuntimeError, match="did not finish its step in time"):
        s.run(nsteps=40)
    assert s.fused is not None and s.fused.timeout_ticks == 0


def test_frame_outputs_together_equal_each_alone(tmp_path):
    """Lat-lon, spectra and particle frames written beside the history frames
    of one run (one shared set of derived fields per frame, one staging path,
    the deferred pinned copies of the single-GPU mode) equal, array for array
    and bit for bit, the frames of a run with only that product on; the last
    lat-lon frame is ``latlon_field`` at the final state."""
    from stsphere.utils import zarr_lite
    products = {"latlon": [8, 16], "spectra": 4, "particles": {"count": 5, "fields": ["h", "u"]}}
    groups = {"latlon": "history_latlon.zarr", "spectra": "history_spectra.zarr",
              "particles": "history_particles.zarr"}

    def run(name, **io):
        c = _cfg(1, 2, N=12, out=str(tmp_path / name))
        c["io"].update(history_interval=4, history_fields=["h", "vorticity"], **io)
        s = Solver(c, verbose=False)
        s.run(nsteps=8)
        assert s.mode == "single" and s.runner is not None
        return s

    def arrays(name, group):
        g = str(tmp_path / name / group)
        return {a: zarr_lite.read_array(g, a) for a in zarr_lite.list_arrays(g)}

    both = run("all", **products)
    last = {f: both.latlon_field(f, 8, 16) for f in ("h", "vorticity")}
    both.close()
    for p, group in groups.items():
        run(p, **{p: products[p]}).close()
        for g in (group, "history.zarr"):
            one, ref = arrays(p, g), arrays("all", g)
            assert sorted(one) == sorted(ref) and len(one) > 2, (p, g)
            for a in one:
                assert one[a].shape[0] == 3 or a in ("lat", "lon", "degree"), (p, g, a)
                assert np.array_equal(one[a], ref[a], equal_nan=True), (p, g, a)
    ll = arrays("all", groups["latlon"])
    assert list(ll["step"]) == [0, 4, 8]
    for f, v in last.items():
        assert np.array_equal(ll[f][-1], v), f
