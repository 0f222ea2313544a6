"""Ensemble members: M independent runs of one configuration on one GPU.

SURVEY.md 2.4 lists ensembles (data parallelism over replicas) as the
optional second axis of the reference's decomposition; the reference itself
has one member (PY:19-85 builds a single 'tiles' mesh).  On MI355X a C96
stage is latency-bound: 216 blocks of one 10-wave workgroup each on 256 CUs,
plus a 1.5 us dependent-launch floor per stage (docs/ARCHITECTURE.md).
Members have no data dependence on each other, so each gets its own engine,
native runner (one hipGraph per chunk length) and HIP stream, and the
members' graphs run concurrently: one member's launch gaps and drain phases
are filled by another's blocks.  Measured at C96 fp64 (tools/ensemble_probe.py,
profiles/r2_ensemble), every member bitwise equal to the same member run alone:
one member 16.3 us/step (3.39e9 cell-updates/s); two members 22.5-23.9 us per
member step, 4.63-4.91e9 aggregate (1.38-1.45x; `python -m stsphere ensemble
configs/reference_6dev.yaml --members 2`: 4.81-4.83e9 against 3.27e9, 1.48x).  Three or more members share the
process's 4 hardware queues (GPU_MAX_HW_QUEUES) with the runners' own streams
and lose (3.2-4.1e9 for three, 2.7e9 for four), so two members per process is
the useful setting at C96 in this mode (``mode="streams"``, the default).

``mode="batched"`` puts the members into the grid of one launch instead: every
buffer is one [M, F, S] tensor, a stage of all members is one launch of
``stage_batch_kernel`` (the plain stage body with a base offset per member; the
same logical block of every member runs on one XCD, so the members share its
geometry lines), and ``steps_per_graph`` steps are one linear graph on one
stream.  Every member is bitwise equal to ``Engine(backend='hip', block=<the
same shape>)`` run alone.  Measured with tools/ensemble_batch_probe.py
(profiles/ensemble_batched, SWE TC5 MC, event-timed, interleaved in one process
with streams mode at 2 members), aggregate cell-updates/s:
C48 fp64  streams-2 1.58e9; batched M = 8 3.04e9 (1.92x), M = 32 5.76e9;
C96 fp64  streams-2 2.86e9; batched M = 8 6.14e9 (2.15x), M = 32 7.60e9;
C96 fp32  streams-2 3.14e9; batched M = 8 8.29e9, M = 32 1.05e10.
Against M sequential runs of the fused step (one run: C96 5.51e9, C48 1.81e9)
batched M = 8 is 1.11x at C96 and 1.68x at C48, M = 32 1.38x and 3.2x.  Below
four members the fused step run M times is faster (C96 M = 4: 4.79e9).
``stats()`` gives the per-cell ensemble mean and variance (a kernel on the
batched state, ops/csrc/ensemble_kernel.hip; the twin elsewhere).

Members differ by a relative perturbation of the initial height (field 0):
member m starts from ``q0 * (1 + amplitude * r_m)`` with ``r_m`` a fixed-seed
standard-normal field (member 0 unperturbed).
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch

from .engine import Engine
from .models.base import Physics
from .models.geometry import CubedSphereGrid
from .parallel.layout import TileLayout


MODES = ("streams", "batched")


class _BatchedCore:
    """What ``GraphStepper`` needs of an engine, for the batched ensemble: the
    pool is the list of [M, F, S] buffers, a step is one batched launch per
    stage, and time / step count are those of every member."""

    def __init__(self, ens: "Ensemble"):
        self.ens = ens
        e0 = ens.engines[0]
        self.integ, self.device, self.dt = e0.integ, e0.device, ens.dt

    @property
    def pool(self):
        return self.ens.batch

    @pool.setter
    def pool(self, bufs):
        self.ens._set_batch(list(bufs))

    @property
    def time(self):
        return self.ens.engines[0].time

    @time.setter
    def time(self, t):
        for e in self.ens.engines:
            e.time = t

    @property
    def step_count(self):
        return self.ens.engines[0].step_count

    @step_count.setter
    def step_count(self, c):
        for e in self.ens.engines:
            e.step_count = c

    def step(self, nsteps: int = 1) -> None:
        self.ens._step_batched(nsteps)


class Ensemble:
    """``members`` engines of one physics / grid / layout on one device.

    mode='streams' (default), backend='hip' on a GPU: each member steps through
    its own NativeStepper (graph replay) on its own stream; otherwise members
    step one after the other through ``Engine.step`` (CPU reference path).

    mode='batched': every buffer of the integrator is allocated once as
    [M, F, S] (``batch``) and member m's ``pool`` entries are its [F, S] slices,
    rotated in lockstep.  backend='hip' on a GPU: one launch per stage runs that
    stage of all members (``stsp_stage_batch_launch``), ``steps_per_graph`` steps
    (rounded up to the integrator's period) are captured into one graph on one
    stream, and a remainder is stepped eagerly.  ``block``: the stage block shape
    (default ``choose_block`` for the tiles of all members).  Otherwise the
    members step one after the other on the batched storage."""

    def __init__(self, physics_factory: Callable[[], Physics], layout: TileLayout, members: int,
                 amplitude: float = 1e-4, seed: int = 0, grid: Optional[CubedSphereGrid] = None,
                 dtype=torch.float64, device="cpu", backend: str = "torch", integrator: str = "ssprk3",
                 dt: Optional[float] = None, steps_per_graph: int = 100, *, mode: str = "streams", block=None):
        if members < 1:
            raise ValueError(f"an ensemble needs at least one member, got {members}")
        if layout.num_ranks != 1:
            raise ValueError("ensemble members run whole grids on one device (layout with one rank)")
        if mode not in MODES:
            raise ValueError(f"unknown ensemble mode {mode!r}; choose from {MODES}")
        self.mode = mode
        self.grid = grid or CubedSphereGrid(layout.N)
        self.engines: List[Engine] = []
        self.batch: List[torch.Tensor] = []
        self.steps_per_graph = steps_per_graph
        self._graph = None
        self._stats = None
        phys0 = physics_factory()
        if getattr(phys0, "time_dependent", False):
            raise ValueError(f"an ensemble of a time-dependent physics ({phys0.name}, flow "
                             f"{getattr(phys0, 'flow', None)!r}) is not supported in mode {mode!r}: the members' "
                             f"graphs and the batched stage hold one set of tables and no step clock; step the "
                             f"members as separate engines")
        engine_kw = {}
        if block is not None:
            engine_kw["block"] = tuple(block)
        if mode == "batched":
            block = self._batched_block(phys0, layout, members, dtype, torch.device(device), backend, block)
            if block is not None:
                engine_kw["block"] = block
        for m in range(members):
            e = Engine(phys0 if (m == 0 and phys0 is not None) else physics_factory(), layout, 0, grid=self.grid,
                       dtype=dtype, device=device, backend=backend, integrator=integrator, dt=dt, **engine_kw)
            if dt is None:
                dt = e.dt                       # every member steps with member 0's dt
            if m > 0 and amplitude != 0.0:
                q = e.tiles_view().clone()
                g = torch.Generator().manual_seed(seed * 100003 + m)
                r = torch.randn(q[0].shape, generator=g, dtype=torch.float64).to(q.device, q.dtype)
                q[0].mul_(1.0 + amplitude * r)
                e.set_state(q)
            self.engines.append(e)
        self.dt = dt
        self.native = backend == "hip" and self.engines[0].device.type == "cuda"
        self.runners = []
        self.streams = []
        if mode == "batched":
            self._make_batch()
            if self.native:
                from .ops import native
                self._lib = native.require_native()
                self._core = _BatchedCore(self)
        elif self.native:
            from .ops.native_runtime import NativeStepper
            for e in self.engines:
                self.runners.append(NativeStepper(e, use_graph=True, steps_per_graph=steps_per_graph))
                self.streams.append(torch.cuda.Stream(e.device))

    # ---- batched mode -------------------------------------------------------
    @staticmethod
    def _batched_block(phys, layout, members, dtype, device, backend, block):
        """Refuse what the batched stage does not run; the block shape of the
        batched launch (None where no stage kernel runs)."""
        if getattr(phys, "two_pass", False):
            raise ValueError("mode='batched': a two_pass physics (the consistent diffusion) runs two launches and "
                             "an exchange per stage, which the batched stage does not have; use mode='streams'")
        if not (backend == "hip" and device.type == "cuda"):
            return tuple(block) if block is not None else None
        from .ops.hip_compute import BLOCK_SHAPES, MARCH_SHAPES, choose_block
        if phys.kernel_id in (3, 4):
            raise ValueError(f"mode='batched': kernel physics {phys.kernel_id} (shallow water with tracers / layers) "
                             f"has no batched stage kernel; use mode='streams'")
        if block is not None:
            block = tuple(block)
            if block in MARCH_SHAPES:
                raise ValueError(f"mode='batched': the streaming stage (march block {block}) has no batched form; "
                                 f"choose from {BLOCK_SHAPES}")
            return block
        plan = layout.plan(0)
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        esize = torch.tensor([], dtype=dtype).element_size()
        return choose_block(plan.n, plan.T * members, cus, int(getattr(phys, "limiter", 0)), esize)

    def _make_batch(self) -> None:
        """Move every member's buffers into the [M, F, S] batch buffers; the
        members' pools become slices of them.  Members 1.. share member 0's
        tables (same physics, grid and layout)."""
        e0 = self.engines[0]
        F, S = e0.pool[0].shape
        self.batch = [torch.zeros((self.members, F, S), dtype=e0.dtype, device=e0.device) for _ in e0.pool]
        for m, e in enumerate(self.engines):
            for k, b in enumerate(self.batch):
                b[m].copy_(e.pool[k])
            if m > 0:
                e.tens = e0.tens
        self._set_batch(self.batch)

    def _set_batch(self, bufs: List[torch.Tensor]) -> None:
        self.batch = bufs
        for m, e in enumerate(self.engines):
            e.pool = [b[m] for b in bufs]

    def _rotate(self) -> None:
        """The batch list in the order of the members' (rotated) pools."""
        p0 = self.engines[0].pool
        by_ptr = {b.data_ptr(): b for b in self.batch}
        self.batch = [by_ptr[p.data_ptr()] for p in p0]

    def _step_batched(self, nsteps: int) -> None:
        """``nsteps`` steps of all members: one batched launch per stage on the
        current stream (descriptor of member 0, whose pool entries are the
        bases of the batch buffers)."""
        from .ops import native
        e0 = self.engines[0]
        hc = e0.compute
        F, S = e0.pool[0].shape
        M = self.members
        for _ in range(nsteps):
            stream = native.current_stream_handle(e0.device)
            for st in e0.integ.stages:
                d = hc.desc(st, self.dt, None, hc.nblocks)
                rc = self._lib.stsp_stage_batch_launch(hc.phys_id, hc.dcode, hc.bx, hc.by, d, M, F * S, stream)
                native.check(rc, "batched stage kernel")
            for e in self.engines:
                e.end_step()
            self._rotate()

    @property
    def block(self):
        """Block shape of the batched stage launches (None: no stage kernel)."""
        c = self.engines[0].compute
        return (c.bx, c.by) if hasattr(c, "bx") else None

    def _graph_for(self, nsteps: int):
        """The captured chunk of ``steps_per_graph`` steps, built when a run is
        long enough to replay it at least once."""
        from .engine import GraphStepper
        per = self.engines[0].integ.period
        k = max(per, -(-self.steps_per_graph // per) * per)
        if self._graph is None and nsteps >= k:
            self._graph = GraphStepper(self._core, steps_per_graph=k)
        return self._graph

    @classmethod
    def from_config(cls, config, members: int, amplitude: float = 1e-4, seed: int = 0,
                    steps_per_graph: int = 100, *, mode: str = "streams") -> "Ensemble":
        """Members of a run configuration (YAML path, dict or Config): the
        grid, physics, dtype, integrator and dt of ``Solver``; each member is
        a whole grid on one device (cuda:0 for ``device_type: gpu``)."""
        from .driver import make_physics
        from .models.geometry import EARTH_RADIUS
        from .utils.config import load_config
        c = load_config(config)
        gpu = c.parallelization.device_type == "gpu"
        if gpu and not torch.cuda.is_available():
            raise RuntimeError("device_type 'gpu' requested but no GPU is visible (use device_type: cpu)")
        device = torch.device("cuda:0") if gpu else torch.device("cpu")
        backend = c.runtime.backend
        if backend == "auto":
            backend = "hip" if gpu else "torch"
        dtype = {"float64": torch.float64, "fp64": torch.float64, "float32": torch.float32,
                 "fp32": torch.float32}[c.grid.dtype]
        phys0 = make_physics(c.physics)
        grid = CubedSphereGrid(c.grid.N, c.grid.radius or EARTH_RADIUS)
        layout = TileLayout(c.grid.N, c.parallelization.tiles_per_edge, 1, ng=max(c.grid.halo, phys0.halo))
        dt = c.time.dt or (phys0.max_dt(grid, c.time.cfl) if c.time.cfl else phys0.max_dt(grid))
        return cls(lambda: make_physics(c.physics), layout, members, amplitude=amplitude, seed=seed, grid=grid,
                   dtype=dtype, device=device, backend=backend, integrator=c.time.integrator, dt=dt,
                   steps_per_graph=steps_per_graph, mode=mode)

    @property
    def members(self) -> int:
        return len(self.engines)

    def prepare(self, nsteps: int) -> None:
        """Record (and upload) every member's graphs for ``run(nsteps)``,
        each primed on the stream it will replay on (the first replay of a
        graph on another stream pays a one-time cost again).  Batched: capture
        the one graph of ``steps_per_graph`` steps."""
        if self.mode == "batched":
            if self.native:
                self._graph_for(nsteps)
                torch.cuda.synchronize(self.engines[0].device)
            return
        for m, r in enumerate(self.runners):
            if m == 0:
                r.prepare(nsteps)
            else:
                with torch.cuda.stream(self.streams[m]):
                    r.prepare(nsteps)
        if self.runners:
            torch.cuda.synchronize(self.engines[0].device)

    def run(self, nsteps: int) -> None:
        """Advance every member ``nsteps`` steps.  Native: the members' graph
        replays are issued on their streams back to back and run concurrently;
        the caller's stream waits for all of them.  Batched, native: full
        chunks of the captured graph are replayed on the caller's stream and
        the remainder is stepped eagerly (the pools then go back to
        construction order, which the graph holds)."""
        if not self.native:
            for e in self.engines:
                e.step(nsteps)
            if self.mode == "batched":
                self._rotate()
            return
        if self.mode == "batched":
            g = self._graph_for(nsteps)
            if g is not None:
                g.run(nsteps)
            else:
                self._step_batched(nsteps)
            return
        # member 0 replays on the caller's stream (a graph replayed on a side
        # stream costs ~3 us/step more at C96, docs/ARCHITECTURE.md "Graph
        # replay"), the others on their own streams, ordered after the
        # caller's earlier work
        # Launches are interleaved chunk by chunk across the members: a graph
        # exec launched again while its previous launch is still running
        # holds the host until that one is done, so issuing all of member 0's
        # chunks first would keep member 1 from starting until member 0 is
        # nearly finished (measured: no overlap at C96 with 6 chunks each).
        cur = torch.cuda.current_stream(self.engines[0].device)
        for s in self.streams[1:]:
            s.wait_stream(cur)
        per = self.runners[0].period
        chunks = [c * per for c in self.runners[0].plan(nsteps)]
        if nsteps > sum(chunks):
            chunks.append(nsteps - sum(chunks))          # partial period: eager
        for k in chunks:
            self.runners[0].run(k)
            for r, s in zip(self.runners[1:], self.streams[1:]):
                with torch.cuda.stream(s):
                    r.run(k)
        for s in self.streams[1:]:
            cur.wait_stream(s)

    def states(self) -> torch.Tensor:
        """[M, F, T, n, n] interior states of all members."""
        return torch.stack([e.tiles_view() for e in self.engines])

    def spread(self, field: int = 0) -> dict:
        """Area-weighted ensemble mean and spread (standard deviation over
        members, then RMS over the sphere) of one field."""
        x = self.states()[:, field]                              # [M, T, n, n]
        area = self.engines[0].tens["area"].reshape(x.shape[1:]).to(x.dtype)
        w = area / area.sum()
        mean = x.mean(0)
        sd = x.std(0, unbiased=False) if self.members > 1 else torch.zeros_like(mean)
        return {"mean": float((w * mean).sum()), "spread_rms": float(torch.sqrt((w * sd * sd).sum()))}

    def stats(self, field: int = 0) -> dict:
        """Per-cell ensemble mean and population variance of one field
        (``mean_field``, ``var_field``: [T, n, n] float64 device tensors) and
        their area-weighted summaries (floats): ``mean``, ``spread_rms`` =
        sqrt(sum A var / sum A), ``max_var`` (models/ensemble_stats.py).
        Batched mode on the HIP backend runs ops/csrc/ensemble_kernel.hip on the
        batched state (the fields are its buffers, overwritten by the next
        call); every other setting stacks the members and runs the twin."""
        e0 = self.engines[0]
        if not 0 <= int(field) < e0.physics.F:
            raise ValueError(f"field {field} of a state with {e0.physics.F} fields")
        if self.mode == "batched" and self.native:
            if self._stats is None:
                from .ops.ensemble_stats import EnsembleStats
                self._stats = EnsembleStats(e0, self.members)
            return self._stats.compute(self.batch[0], field)
        from .models.ensemble_stats import ensemble_stats
        x = torch.stack([e.tiles_view()[field] for e in self.engines])      # [M, T, n, n]
        return ensemble_stats(x, e0.tens["area"].reshape(x.shape[1:]))

    def global_fields(self, field: int = 0) -> np.ndarray:
        """[M, 6, N, N] global field of every member (host)."""
        return np.stack([e.global_field(field) for e in self.engines])

    def close(self) -> None:
        for r in self.runners:
            r.close()
        self.runners = []
        self._graph = None
