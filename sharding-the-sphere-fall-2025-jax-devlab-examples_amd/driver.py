"""Solver driver: the "JAXStream" pipeline of PDF s.6 (Geometry -> Initial
Conditions -> Solver -> {History, Restarts, Analysis}) on MI355X.

The reference shows only a method ``setup_sharding(self)`` of an unnamed class
holding ``self.config``, ``self.mesh`` and ``self.sharding`` (PY:19-85).
``Solver`` is that class:

    solver = Solver("config.yaml")      # or a dict / Config
    solver.setup_sharding()             # validation + banner, sets .mesh/.sharding
    solver.initialize()                 # grid, physics, per-rank engines, restore
    summary = solver.run(days=5)        # time loop, history, checkpoints, metrics

Execution modes (chosen from the config and the launch environment):

* ``single``  one device (GPU: fused HIP stage kernels + HIP-graph replay;
              CPU: PyTorch reference);
* ``virtual`` several ranks in one process, stepped in lockstep (the analogue
              of the reference's CPU virtual devices, PY:64-68; also works on
              one GPU);
* ``spmd``    one process per device under ``torchrun`` (WORLD_SIZE > 1):
              RCCL (backend "nccl") on GPUs, gloo on CPUs, bundled P2P halos.
"""
from __future__ import annotations

import math
import os
import time
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .diagnostics import LATLON_WINDS, SolverDiagnostics
from .engine import Engine, VirtualCluster
from .models.advection import Advection
from .models.base import limiter_code
from .models.derived import FIELDS as DERIVED_FIELDS, INVARIANTS
from .models.diffusion import OPERATORS, ConsistentDiffusion, Diffusion
from .models.geometry import DAY, EARTH_RADIUS, CubedSphereGrid
from .models.spectra import check_lmax
from .models.swe import MAX_TRACERS, LayeredShallowWater, ShallowWater, ShallowWaterTracers
from .parallel.comm import NativeBuffers, TorchDistTransport
from .parallel.layout import TileLayout
from .parallel.mesh import setup_sharding
from .utils import checkpoint as ckpt
from .utils.config import Config, default_case, load_config
from .utils.history import (HistoryWriter, LatLonHistoryWriter, MetricsLogger, ParticleHistoryWriter,
                            SpectraHistoryWriter)


# invariants the metrics records gain with the shallow-water model
METRIC_INVARIANTS = ("potential_enstrophy", "circulation", "max_courant")


def _fold_tracers(rec: Dict[str, float], nq: int) -> Dict[str, Any]:
    """The per-tracer scalars ``tracer_mass_k`` (and ``tracer_min_k`` /
    ``tracer_max_k``) of a metrics record as lists ``tracer_mass`` (..) [NQ]."""
    if not nq:
        return rec
    out = {k: v for k, v in rec.items() if not k.startswith("tracer_")}
    for name in ("tracer_mass", "tracer_min", "tracer_max"):
        if f"{name}_0" in rec:
            out[name] = [rec[f"{name}_{k}"] for k in range(nq)]
    return out


def make_physics(pc) -> Any:
    model = pc.model.lower()
    case = pc.case or default_case(model)
    lim = limiter_code(pc.limiter)
    tracers = pc.tracers
    if tracers is not None and (not isinstance(tracers, (list, tuple)) or len(tracers) > MAX_TRACERS
                                or not all(isinstance(t, str) for t in tracers)):
        raise ValueError(f"physics.tracers: a list of at most {MAX_TRACERS} initial-condition names expected, "
                         f"not {tracers!r}")
    if tracers and model != "swe":
        raise ValueError(f"physics.tracers: tracers are carried by the shallow-water model, not {model!r}")
    tlim = getattr(pc, "tracer_limiter", None)
    if tlim is not None:
        if not (isinstance(tlim, str) and tlim.lower() == "ppm"):
            raise ValueError(f"physics.tracer_limiter: null or ppm expected, not {tlim!r}")
        if not tracers:
            raise ValueError("physics.tracer_limiter: set together with physics.tracers (it reconstructs the "
                             "mixing ratios)")
        tlim = "ppm"
    op = pc.operator
    if op not in OPERATORS:
        raise ValueError(f"physics.operator: one of {list(OPERATORS)} expected, not {op!r}")
    if op == "consistent" and model != "diffusion":
        raise ValueError(f"physics.operator: consistent is defined for the diffusion model, not {model!r}")
    flow, period_days = getattr(pc, "flow", None), getattr(pc, "period_days", None)
    if (flow is not None or period_days is not None) and model != "advection":
        raise ValueError(f"physics.flow / physics.period_days: the prescribed wind of the advection model, "
                         f"not of {model!r}")
    layers = layers_spec(pc)
    if layers is not None:
        if tracers:
            raise ValueError("physics.layers with physics.tracers: tracers ride one shallow-water layer; a "
                             "layered run carries none")
        return LayeredShallowWater(case, limiter=lim, alpha=pc.alpha, **layers)
    if model == "swe":
        if tracers:
            return ShallowWaterTracers(case, tracers=list(tracers), limiter=lim, alpha=pc.alpha, tracer_limiter=tlim)
        return ShallowWater(case, limiter=lim, alpha=pc.alpha)
    if model == "advection":
        kw = {}
        if flow is not None:
            kw["flow"] = flow
        if period_days is not None:
            try:                                 # YAML 1.1 reads 1.2e1 (no sign in the exponent) as a string
                kw["period"] = float(period_days) * DAY
            except (TypeError, ValueError):
                raise ValueError(f"physics.period_days: a number expected, not {period_days!r}") from None
        return Advection(case, alpha=pc.alpha, limiter=lim, **kw)
    if model == "diffusion":
        try:                                     # YAML 1.1 reads 2.0e6 (no sign in the exponent) as a string
            kappa = float(pc.kappa)
        except (TypeError, ValueError):
            raise ValueError(f"physics.kappa: a number expected, not {pc.kappa!r}") from None
        return (ConsistentDiffusion if op == "consistent" else Diffusion)(kappa=kappa, case=case)
    raise ValueError(f"unknown physics model {pc.model!r}")


def layers_spec(pc) -> Optional[Dict[str, Any]]:
    """``physics.layers`` checked: the keyword arguments {depths, density_ratio,
    winds, jet_scale} of ``LayeredShallowWater``, or None when it is off."""
    d = getattr(pc, "layers", None)
    if d is None:
        return None
    if not isinstance(d, dict) or "depths" not in d:
        raise ValueError(f"physics.layers: {{depths, density_ratio, winds, jet_scale}} expected, not {d!r}")
    unknown = set(d) - {"depths", "density_ratio", "winds", "jet_scale"}
    if unknown:
        raise ValueError(f"physics.layers: unknown key(s) {sorted(unknown)}")
    if pc.model.lower() != "swe":
        raise ValueError(f"physics.layers: defined for the shallow-water model, not {pc.model!r}")
    def numbers(key, v):
        try:                                     # YAML 1.1 reads 4.0e3 (no sign in the exponent) as a string
            return [float(x) for x in v]
        except (TypeError, ValueError):
            raise ValueError(f"physics.layers.{key}: a list of numbers expected, not {v!r}") from None
    out: Dict[str, Any] = {"depths": numbers("depths", d["depths"])}
    if len(out["depths"]) != 2:
        raise ValueError(f"physics.layers.depths: two layers [H_0, H_1] expected, not {d['depths']!r}")
    if d.get("winds") is not None:
        out["winds"] = numbers("winds", d["winds"])
    for key in ("density_ratio", "jet_scale"):
        if d.get(key) is not None:
            out[key] = numbers(key, [d[key]])[0]
    return out


def dissipation_spec(pc) -> Optional[Dict[str, Any]]:
    """``physics.dissipation`` checked and completed: {order, nu, interval,
    depth}, or None when it is off."""
    d = pc.dissipation
    if d is None:
        return None
    if not isinstance(d, dict):
        raise ValueError(f"physics.dissipation: {{order, nu, interval, depth}} expected, not {d!r}")
    unknown = set(d) - {"order", "nu", "interval", "depth"}
    if unknown:
        raise ValueError(f"physics.dissipation: unknown key(s) {sorted(unknown)}")
    order, nu, interval, depth = d.get("order"), d.get("nu"), d.get("interval", 1), d.get("depth", True)
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"physics.dissipation: order must be 1 or 2, not {order!r}")
    if isinstance(nu, str):                  # YAML 1.1 reads 1.0e5 (no sign in the exponent) as a string
        try:
            nu = float(nu)
        except ValueError:
            pass
    if isinstance(nu, bool) or not isinstance(nu, (int, float)) or not nu > 0:
        raise ValueError(f"physics.dissipation: nu must be a positive number, not {nu!r}")
    if isinstance(interval, bool) or not isinstance(interval, int) or interval < 1:
        raise ValueError(f"physics.dissipation: interval must be a positive integer, not {interval!r}")
    if not isinstance(depth, bool):
        raise ValueError(f"physics.dissipation: depth must be true or false, not {depth!r}")
    if pc.model.lower() != "swe":
        raise ValueError(f"physics.dissipation: defined for the shallow-water model, not {pc.model!r}")
    if getattr(pc, "layers", None) is not None:
        raise ValueError("physics.dissipation with physics.layers: the dissipation operator acts on one "
                         "shallow-water layer (h, M); a layered run takes none")
    if pc.tracers and depth:
        raise ValueError("physics.dissipation with physics.tracers: only depth: false is accepted (diffusing h "
                         "would change the mixing ratios hq / h)")
    return {"order": int(order), "nu": float(nu), "interval": int(interval), "depth": depth}


class _HostQueue:
    """Host work of the run loop, in submission order: ``append((event,
    work))`` runs ``work()`` once ``event`` (a CUDA event, or None) has
    completed; threaded, on one background thread, else inline at ``drain``."""

    def __init__(self, threaded: bool):
        self._items: List[Any] = []
        self._ex = None
        if threaded:
            from concurrent.futures import ThreadPoolExecutor
            self._ex = ThreadPoolExecutor(max_workers=1, thread_name_prefix="stsp-io")

    def append(self, item) -> None:
        ev, work = item
        if self._ex is None:
            self._items.append(item)
            return

        def job():
            if ev is not None:
                ev.synchronize()
            work()
        self._items.append(self._ex.submit(job))

    def __len__(self) -> int:
        return len(self._items)

    def drain(self, block: bool = False) -> None:
        """Finish the completed items (all of them when ``block``); a failed
        background item raises here."""
        while self._items:
            it = self._items[0]
            if self._ex is not None:
                if not block and not it.done():
                    return
                self._items.pop(0).result()
                continue
            ev, work = it
            if not block and ev is not None and not ev.query():
                return
            self._items.pop(0)
            if ev is not None:
                ev.synchronize()
            work()

    def close(self) -> None:
        self.drain(block=True)
        if self._ex is not None:
            self._ex.shutdown(wait=True)
            self._ex = None

    def clear(self) -> None:
        """Drop what has not run yet (recovery); a running item completes."""
        for it in self._items:
            if self._ex is not None:
                it.cancel()
        if self._ex is not None:
            for it in self._items:
                if not it.cancelled():
                    it.exception()
        self._items = []


def stage(v, async_copy: bool):
    """(event or None, host copy) of the tensor ``v``, or of a list of tensors
    (one event, a list of copies).  ``async_copy`` and device tensors: the copy
    goes to pinned host memory on the current stream without blocking and the
    event, recorded after it, says when the host may read it.  Otherwise a
    plain blocking copy (a CPU tensor is cloned) and no event."""
    vs = list(v) if isinstance(v, (list, tuple)) else [v]
    ev = None
    if async_copy and all(x.is_cuda for x in vs):
        hs = []
        for x in vs:
            hs.append(torch.empty(x.shape, dtype=x.dtype, pin_memory=True))
            hs[-1].copy_(x, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
    else:
        hs = [x.cpu() if x.is_cuda else x.clone() for x in vs]
    return ev, (hs if isinstance(v, (list, tuple)) else hs[0])


class Solver(SolverDiagnostics):
    def __init__(self, config=None, verbose: bool = True):
        super().__init__()
        self._wd_pending = None       # (event, pinned flags) of the deferred watchdog check in flight
        self.cfg: Config = load_config(config)
        self.config: Dict[str, Any] = self.cfg.to_dict()
        self.verbose = verbose
        self.mesh = None
        self.sharding = None
        self.engines: List[Engine] = []
        self.cluster: Optional[VirtualCluster] = None
        self.runner = None            # NativeStepper (GPU) once stepping starts
        self.fused = None             # ops/fused.py::FusedKernel when the runner steps with it
        self.xgmi = None
        self._ipc = None
        self._nccl = None
        self.comm = "local"
        self.mode = None
        self.world, self.rank = 1, 0
        self._dspec = None            # physics.dissipation, checked (initialize)
        self._dinterval = 0           # model steps between its applications (doubles when dt is halved)
        self._gstepper = None         # engine.GraphStepper of a time-dependent physics (one GPU, runtime.graph)

    # ---- setup ------------------------------------------------------------
    def setup_sharding(self) -> None:
        self.mesh, self.sharding = setup_sharding(self.config, verbose=self.verbose and self._is_root())

    def _is_root(self) -> bool:
        return int(os.environ.get("RANK", "0")) == 0

    def _log(self, *a) -> None:
        if self.verbose and self.rank == 0:
            print(*a, flush=True)

    def initialize(self) -> None:
        if self.sharding is None:
            self.setup_sharding()
        c = self.cfg
        nd = c.parallelization.num_devices
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        self._dspec = dissipation_spec(c.physics)
        if self._dspec is not None and self.world > 1:
            raise ValueError("physics.dissipation: one process per rank (spmd) is not supported; run one "
                             "rank or virtual ranks in one process")
        if (c.physics.flow or "solid_body") != "solid_body" and self.world > 1:
            raise ValueError("physics.flow: a time-dependent wind with one process per rank (spmd) is not "
                             "supported (the native runtime's graphs hold one set of transport tables and no step "
                             "clock); run one rank or virtual ranks in one process")
        if c.physics.operator == "consistent" and self.world > 1:
            raise ValueError("physics.operator: consistent: one process per rank (spmd) is not supported; run one "
                             "rank or virtual ranks in one process")
        gpu = c.parallelization.device_type == "gpu"
        if gpu and not torch.cuda.is_available():
            raise RuntimeError("device_type 'gpu' requested but no GPU is visible (use device_type: cpu)")
        if self.world > 1:
            if self.world != nd:
                raise ValueError(f"launched with {self.world} processes but num_devices = {nd}")
            self.mode = "spmd"
            import torch.distributed as dist
            # STSP_SHARE_GPU=1: every rank on cuda:0 with a gloo group (functional
            # rehearsal of the multi-GPU paths on a one-GPU machine)
            share = os.environ.get("STSP_SHARE_GPU") == "1"
            device = torch.device(f"cuda:{0 if share else local}") if gpu else torch.device("cpu")
            if gpu:
                torch.cuda.set_device(device)
            if not dist.is_initialized():
                if gpu and not share:
                    dist.init_process_group("nccl", device_id=device)
                else:
                    dist.init_process_group("gloo")
        else:
            self.mode = "single" if nd == 1 else "virtual"
            device = torch.device("cuda:0") if gpu else torch.device("cpu")
        self.device = device
        if self._dspec is not None:
            self._dinterval = self._dspec["interval"]
            if c.io.checkpoint_interval > 0 and c.io.checkpoint_interval % self._dinterval:
                raise ValueError(f"io.checkpoint_interval = {c.io.checkpoint_interval} is not a multiple of "
                                 f"physics.dissipation.interval = {self._dinterval}")
        backend = c.runtime.backend
        if backend == "auto":
            backend = "hip" if device.type == "cuda" else "torch"
        self.backend = backend
        dtype = {"float64": torch.float64, "fp64": torch.float64, "float32": torch.float32,
                 "fp32": torch.float32}[c.grid.dtype]
        self.dtype = dtype
        N, t = c.grid.N, c.parallelization.tiles_per_edge
        phys0 = make_physics(c.physics)
        if c.runtime.comm == "xgmi" and phys0.F not in (1, 4):
            raise ValueError(f"runtime.comm = xgmi with physics.{'layers' if phys0.kernel_id == 4 else 'tracers'}: "
                             f"the direct xGMI exchange packs 1 or 4 fields; use comm: auto, ipc or rccl")
        # PPM reads three ghost layers: widen the halo if the config asks for fewer
        self.layout = TileLayout(N, t, nd, ng=max(c.grid.halo, phys0.halo), owner=self.sharding.owner)
        self.grid = self._geometry_stage(N, c.grid.radius or EARTH_RADIUS)
        dt = c.time.dt or (phys0.max_dt(self.grid, c.time.cfl) if c.time.cfl else phys0.max_dt(self.grid))
        if phys0.time_dependent:
            from .ops.hip_compute import MARCH_SHAPES
            if c.runtime.block and tuple(c.runtime.block) in MARCH_SHAPES:
                raise ValueError(f"physics.flow: runtime.block = {list(c.runtime.block)} is a march block of the "
                                 f"streaming stage, which runs shallow water and reads no transport tables; a "
                                 f"time-dependent wind steps through the block stage kernel")
            if not c.time.dt:
                # a whole number of steps per period: the run ends on t = m T, where the
                # initial condition is the exact solution
                dt = phys0.period / math.ceil(phys0.period / dt - 1e-9)
        kw = dict(grid=self.grid, dtype=dtype, device=device, backend=backend, integrator=c.time.integrator, dt=dt)
        if c.runtime.block:
            kw["block"] = tuple(c.runtime.block)
        if self.mode == "virtual":
            self.cluster = VirtualCluster(lambda: make_physics(c.physics), self.layout, **kw)
            self.engines = list(self.cluster.engines)
        elif self.mode == "spmd":
            comm = c.runtime.comm
            if comm == "auto":
                # GPUs: the native runtime with the direct xGMI exchange
                comm = "xgmi" if (backend == "hip" and c.runtime.graph and not c.runtime.canary) else "torch"
            if comm in ("xgmi", "rccl", "ipc") and backend != "hip":
                raise ValueError(f"runtime.comm = {comm} needs the HIP backend")
            self.comm = comm
            if comm in ("xgmi", "rccl", "ipc"):
                tr = NativeBuffers(self.layout.plan(self.rank), phys0.F, dtype, device)
            else:
                tr = TorchDistTransport(self.layout.plan(self.rank), phys0.F, dtype, device,
                                        staged=(comm == "staged"))
            self.engines = [Engine(phys0, self.layout, self.rank, transport=tr, **kw)]
        else:
            self.engines = [Engine(phys0, self.layout, 0, **kw)]
        for e in self.engines:
            e.canary = c.runtime.canary
        self.dt = dt
        self.physics = phys0
        self.fields = list(phys0.fields)
        hf = c.io.history_fields
        if hf is not None:
            unknown = [f for f in hf if f not in self.fields and f not in DERIVED_FIELDS
                       and f not in self.mix_names()]
            if not hf:
                raise ValueError("io.history_fields: an empty list (use null for the prognostic fields)")
            if unknown:
                raise ValueError(f"io.history_fields: unknown field(s) {unknown}; choose from "
                                 f"{self.fields + self.mix_names() + list(DERIVED_FIELDS)}")
            if self.layers() and any(f in DERIVED_FIELDS for f in hf):
                raise ValueError(f"io.history_fields: derived fields of a layered run are per layer; choose from "
                                 f"{self.fields + self.mix_names()}")
            if phys0.name != "swe" and any(f in DERIVED_FIELDS for f in hf):
                raise ValueError(f"io.history_fields: derived fields {list(DERIVED_FIELDS)} need the "
                                 f"shallow-water model, not {phys0.name!r}")
        ll = c.io.latlon
        if ll is not None and not (isinstance(ll, (list, tuple)) and len(ll) == 2
                                   and all(isinstance(v, int) and v > 0 for v in ll)):
            raise ValueError(f"io.latlon: [nlat, nlon] of two positive integers expected, not {ll!r}")
        if c.io.spectra is not None:
            try:
                check_lmax(c.io.spectra, N)
            except ValueError as err:
                raise ValueError(f"io.spectra: {err}") from None
        self._log(f"Initialized {phys0.name} ({getattr(phys0, 'case', '')}) C{N}, {self.mode} mode, "
                  f"backend={backend}, dtype={c.grid.dtype}, dt={dt:.3f} s, integrator={c.time.integrator}")
        if c.io.initial_condition and not c.io.restore:
            self._initial_condition_stage(c.io.initial_condition)
        if c.io.restore:
            path = c.io.restore
            if path == "latest":
                path = ckpt.latest_checkpoint(self.checkpoint_root())
            if path:
                self.restore_checkpoint(path)
        if c.io.particles is not None:
            self._init_particles(c.io.particles)

    # ---- pipeline stages: Geometry and Initial Conditions through zarr (PDF s.6) ----
    def _geometry_stage(self, N: int, radius: float) -> CubedSphereGrid:
        """Read the grid from ``io.geometry`` when that zarr group exists, else
        compute it and (rank 0) write it there."""
        path = self.cfg.io.geometry
        if path and os.path.exists(os.path.join(path, ".zgroup")):
            g = CubedSphereGrid.load_zarr(path, N=N, radius=radius)
            self._log(f"Geometry: read C{N} grid from {path}")
            return g
        g = CubedSphereGrid(N, radius)
        if path:
            if self.rank == 0:
                g.save_zarr(path)
                self._log(f"Geometry: wrote C{N} grid to {path}")
            self._barrier()
        return g

    def _initial_condition_stage(self, path: str) -> None:
        """Read the initial state [F, 6, N, N] from ``io.initial_condition``
        when that zarr group exists, else (rank 0) write the analytic initial
        condition the engines were built with.  Partition-independent, like
        checkpoints."""
        from .utils import zarr_lite
        if os.path.exists(os.path.join(path, ".zgroup")):
            attrs = zarr_lite.read_attrs(path)
            if int(attrs["N"]) != self.layout.N or list(attrs["fields"]) != list(self.fields):
                raise ValueError(f"{path}: initial condition is C{attrs['N']} {attrs['fields']}, "
                                 f"run is C{self.layout.N} {self.fields}")
            # the state must belong to this physics and case: TC2 and TC5 share the
            # SWE fields but not the topography the engines were built with
            want = {"physics": self.physics.name, "case": getattr(self.physics, "case", None)}
            for k, v in want.items():
                if k in attrs and attrs[k] != v:
                    raise ValueError(f"{path}: initial condition was written for {k} {attrs[k]!r}, "
                                     f"the run is {k} {v!r} (remove the file or fix io.initial_condition)")
            glob = np.stack([zarr_lite.read_array(path, f) for f in self.fields])
            for e in self.engines:
                loc = np.stack([e.geo.gather_global(glob[k]) for k in range(len(self.fields))])
                e.set_state(torch.as_tensor(loc, dtype=self.dtype))
            self._log(f"Initial conditions: read {path}")
            return
        g = self.gather_global()
        if self.rank == 0:
            zarr_lite.create_group(path, attrs={"N": self.layout.N, "fields": self.fields,
                                                "physics": self.physics.name,
                                                "case": getattr(self.physics, "case", None), "time": self.time})
            for k, f in enumerate(self.fields):
                zarr_lite.write_array(path, f, g[k], chunks=(1, self.layout.N, self.layout.N))
            self._log(f"Initial conditions: wrote {path}")
        self._barrier()

    # ---- state access ---------------------------------------------------------
    @property
    def time(self) -> float:
        return self.engines[0].time

    @property
    def step_count(self) -> int:
        return self.engines[0].step_count

    def local_values(self) -> Dict[int, np.ndarray]:
        """{rank: [F, T_local, n, n]} for the engines of this process."""
        return {e.rank: e.tiles_view().detach().cpu().double().numpy() for e in self.engines}

    def gather_global(self) -> Optional[np.ndarray]:
        """[F, 6, N, N] on rank 0 (None elsewhere)."""
        return self._gather_tiles(self.local_values())

    def global_field(self, name_or_index=0) -> Optional[np.ndarray]:
        f = self.fields.index(name_or_index) if isinstance(name_or_index, str) else name_or_index
        g = self.gather_global()
        return None if g is None else g[f]

    def _allreduce(self, vals: Dict[str, float], op: str = "sum") -> Dict[str, float]:
        if self.mode != "spmd":
            return vals
        import torch.distributed as dist
        keys = sorted(vals)
        t = torch.tensor([vals[k] for k in keys], dtype=torch.float64,
                         device=self.device if self.device.type == "cuda" else "cpu")
        dist.all_reduce(t, op={"sum": dist.ReduceOp.SUM, "min": dist.ReduceOp.MIN, "max": dist.ReduceOp.MAX}[op])
        return dict(zip(keys, t.tolist()))

    def diagnostics(self) -> Dict[str, float]:
        tot: Dict[str, float] = {}
        for e in self.engines:
            for k, v in e.diagnostics().items():
                tot[k] = tot.get(k, 0.0) + v
        return self._allreduce(tot)

    def error_norms(self) -> Optional[Dict[str, float]]:
        """Williamson l1 / l2 / linf of field 0 against the case's true
        solution at the current time (TC1, TC2, lake at rest), on rank 0;
        None where the case has no closed form (and on other ranks)."""
        from .models.errors import williamson_norms
        exact = getattr(self.physics, "exact", None)
        if self.layers() > 1:      # per layer: h0_l1, h0_l2, h0_linf, h1_l1, ..
            g = self.gather_global()
            ht = exact(self.grid, self.time)
            if g is None or ht is None:
                return None
            out = {}
            for k in range(self.layers()):
                out.update({f"h{k}_{n}": v for n, v in williamson_norms(g[4 * k], ht[k], self.grid.areas()).items()})
            return out
        h = self.global_field(0)
        if exact is None or h is None:
            return None
        # a time-dependent wind returns the field at t = m T: the step decides what "at" means
        ht = exact(self.grid, self.time, self.dt) if self.physics.time_dependent else exact(self.grid, self.time)
        if ht is None:
            return None
        return williamson_norms(h, ht, self.grid.areas())

    def tracer_error_norms(self, k: int = 0) -> Optional[Dict[str, float]]:
        """Williamson l1 / l2 / linf of the mixing ratio q_k against its true
        solution at the current time (a ``cosine_bell`` tracer on TC2), on
        rank 0; None where there is no closed form (and on other ranks)."""
        from .models.errors import williamson_norms
        exact = getattr(self.physics, "tracer_exact", None)
        if exact is None:
            return None
        qt = exact(self.grid, self.time, int(k))     # the same answer on every rank: the gather below is collective
        if qt is None:
            return None
        q = self.tracer(k)
        if q is None:
            return None
        return williamson_norms(q, qt, self.grid.areas())

    def all_finite(self) -> bool:
        if self.runner is not None:
            self.runner.check()      # direct xGMI exchange: raises on a halo poll timeout
        ok = float(all(bool(torch.isfinite(e.tiles_view()).all()) for e in self.engines))
        return self._allreduce({"ok": ok}, op="min")["ok"] > 0.5

    # ---- stepping ---------------------------------------------------------------
    def _use_native(self) -> bool:
        """Step through the C++ runtime (ops/native_runtime.py): one GPU with
        graph replay, or SPMD GPUs with the direct xGMI / RCCL exchange."""
        c = self.cfg.runtime
        if self.backend != "hip" or c.canary:
            return False
        if getattr(self.physics, "two_pass", False):
            return False                 # two launches and an exchange per stage: eager, through Engine.step
        if self.physics.time_dependent:
            return False                 # a table launch per stage and a device clock: Engine.step / GraphStepper
        if self.mode == "single":
            return c.graph
        return self.mode == "spmd" and self.comm in ("xgmi", "rccl", "ipc")

    def _fused_plan(self, chunks):
        """(use the fused step, steps per launch) for this run.  The fused
        SSP-RK3 step (ops/fused.py) is the flagship path: one launch advances
        a rank by several steps (every block resident, in-launch hand-offs), the
        reference's "one compiled program" (PY:238-246; PDF s.10) driven from the
        solver (PDF s.6 pipeline).  auto: shallow water + SSP-RK3 + PLR, one GPU
        or SPMD ranks with the direct xGMI exchange, and at most two passes of
        blocks over the CUs (one step per launch beyond one pass)."""
        from .ops.fused import fused_block, fused_supported, rank_cus
        c = self.cfg.runtime
        e = self.engines[0]
        if c.fused == "off" or e.device.type != "cuda":
            return False, 1
        # one GPU, or SPMD ranks with the direct xGMI exchange (the ring inside
        # the fused kernel); auto takes the multi-rank fused step when every
        # block of the rank's share is resident (checked below)
        if not (self.mode == "single" or (self.mode == "spmd" and self.comm == "xgmi")):
            if c.fused == "on":
                raise ValueError(f"runtime.fused = on needs one GPU or the xgmi exchange (mode {self.mode}, "
                                 f"comm {self.comm})")
            return False, 1
        why = fused_supported(e)
        if why:
            if c.fused == "on":
                raise ValueError(why)
            return False, 1
        cus = rank_cus(e.device)
        B = fused_block(e.plan.n, len(e.plan.tiles), cus)
        nb = len(e.plan.tiles) * (e.plan.n // B) ** 2
        if c.fused == "auto" and nb > (2 * cus if self.mode == "single" else cus):
            return False, 1
        if nb > cus:
            return True, 1                     # one step per launch (blocks not all resident)
        spl = c.steps_per_launch
        if spl <= 0:
            # the longest even launch dividing EVERY chunk length of the run
            # (each launch boundary costs ~18 us of ramp, profiles/r4_spl/); a
            # run whose chunks share no even divisor launches its longest even
            # part per chunk, the rest through the remainder path (its
            # descriptors are built and primed by prepare())
            lens = [max(1, int(k)) for k in (chunks if isinstance(chunks, (list, tuple)) else [chunks])]
            g = 0
            for k in lens:
                g = math.gcd(g, k)
            divs = [s for s in range(2, 513, 2) if g % s == 0]
            k0 = min(lens)
            spl = max(divs) if divs else (min(512, k0 - k0 % 2) if k0 >= 2 else 1)
        if spl > 1 and spl % 2:
            raise ValueError("runtime.steps_per_launch must be even")
        return True, spl

    def _make_runner(self, chunks=(20,)):
        from .ops.native_runtime import NativeStepper, create_nccl_comm
        e = self.engines[0]
        c = self.cfg.runtime
        use_fused, spl = self._fused_plan(list(chunks))
        self.fused = None
        if use_fused:
            from .ops.fused import FusedKernel, fused_block, rank_cus
            cus = rank_cus(e.device)
            try:
                fk = FusedKernel(e, B=fused_block(e.plan.n, len(e.plan.tiles), cus))   # collective with several ranks
            except RuntimeError as exc:
                if self.mode != "spmd":
                    raise
                # the ring setup raised on every rank alike: the stage-kernel op
                # list with the next transport of the chain
                self._log(f"Runtime: fused xGMI step unavailable ({exc}); falling back")
                self.comm = "ipc"
                fk = None
            if fk is not None:
                self.fused = fk
                self.xgmi = fk if self.mode == "spmd" else None
                self._log(f"Runtime: fused SSP-RK3 step, {fk.plan.nb} blocks of {fk.plan.B}x{fk.plan.B}, "
                          f"{spl} step(s) per launch, " + ("direct launches" if self.mode == "single" else "graph replay"))
                return NativeStepper(e, use_graph=True, steps_per_graph=c.steps_per_graph, fused=fk,
                                     steps_per_launch=spl, direct=self.mode == "single")
        if self.mode == "single" and c.march3 != "off":
            from .ops.march3 import March3Step, march3_unsupported, march3_wanted
            why = march3_unsupported(e)
            if c.march3 == "on" and why:
                raise ValueError(f"runtime.march3 = on: {why}")
            if c.march3 == "on" or march3_wanted(e):
                m3 = March3Step(e, rows=c.march3_rows)
                self._log(f"Runtime: pipelined SSP-RK3 march ({m3.ncs} strips x {m3.nrs} segments per tile, "
                          f"{m3.band.numel()} band blocks), graph replay")
                self.xgmi = self._ipc = None
                return NativeStepper(e, use_graph=c.graph, steps_per_graph=c.steps_per_graph, march3=m3)
        xg = nc = ipc = None
        if self.mode == "spmd":
            # transport chain between GPUs: direct xGMI rings -> IPC copy kernel
            # (graph-captured) -> RCCL (eager).  A setup that fails raises on
            # every rank alike (IpcRing agrees on every step), so all ranks
            # move down the chain together.
            order = ["xgmi", "ipc", "rccl"]
            chain = order[order.index(self.comm):] if self.comm in order else [self.comm]
            for k, cm in enumerate(chain):
                try:
                    if cm == "xgmi":
                        from .ops.xgmi import XgmiHalo
                        xg = XgmiHalo(e)
                    elif cm == "ipc":
                        from .ops.native_runtime import IpcExchange
                        ipc = IpcExchange(e, IpcExchange.slots_for(e))        # collective (IPC handles)
                    elif cm == "rccl":
                        if self._nccl is None:
                            self._nccl = create_nccl_comm(self.rank, self.world, self.device.index or 0)
                        nc = self._nccl
                    self.comm = cm
                    break
                except RuntimeError as exc:
                    if k == len(chain) - 1:
                        raise
                    self._log(f"Runtime: {cm} exchange unavailable ({exc}); falling back to {chain[k + 1]}")
        self.xgmi = xg
        self._ipc = ipc
        return NativeStepper(e, nccl_comm=nc, use_graph=c.graph, steps_per_graph=c.steps_per_graph, xgmi=xg,
                             ipc=ipc)

    def close(self) -> None:
        """Release the step runner and the exchange rings explicitly.  With
        several ranks this is collective (every rank calls it, as the run
        script does at the end): the rings' close joins a group barrier, which
        a garbage-collection finalizer must not do."""
        if self.runner is not None:
            self.runner.close()
            self.runner = None
        seen = set()
        for obj in (self.xgmi, self.fused, getattr(self, "_ipc", None)):
            if obj is not None and id(obj) not in seen and hasattr(obj, "close"):
                seen.add(id(obj))
                obj.close()
        self.xgmi = self.fused = self._ipc = None

    def step(self, nsteps: int = 1) -> None:
        """Advance the model ``nsteps`` steps; with particles attached, in
        pieces of their interval with a particle advance after each."""
        if nsteps <= 0:
            return
        div = self._dinterval if self._dspec is not None else 0
        piv = self._pinterval if self._particles else 0
        if not div and not piv:
            return self._step_model(nsteps)
        if piv and nsteps % piv:
            raise ValueError(f"step({nsteps}): with particles attached the step count must be a multiple of "
                             f"their interval {piv}")
        if div and nsteps % div:
            raise ValueError(f"step({nsteps}): with physics.dissipation the step count must be a multiple of "
                             f"its interval {div}")
        pos = 0
        while pos < nsteps:      # pieces that end at the next dissipation or particle time
            nxt = min((pos // v + 1) * v for v in (div, piv) if v)
            self._step_model(nxt - pos)
            pos = nxt
            if div and pos % div == 0:
                self.dissipate()
            if piv and pos % piv == 0:
                self._particles_advance()

    def _dissipations(self):
        """The dissipation operator of every engine of this process, as configured."""
        if self._dspec is None:
            raise ValueError("no dissipation configured (physics.dissipation)")
        s = self._dspec
        return [e.dissipation(s["order"], s["nu"], s["depth"]) for e in self.engines]

    def dissipate(self, tau: Optional[float] = None) -> int:
        """Apply the configured dissipation once over ``tau`` seconds (default:
        its interval times dt), split into equal Euler sub-steps where the
        explicit bound asks for it; returns their number."""
        from .ops.dissipation import apply_all
        ds = self._dissipations()
        return apply_all(ds, self._dinterval * self.dt if tau is None else float(tau))

    def _step_model(self, nsteps: int) -> None:
        if self.mode == "virtual":
            self.cluster.step(nsteps)
        elif self._use_native():
            if self.runner is None:
                self.runner = self._make_runner()
            self.runner.run(nsteps)
        elif self._graph_stepper() is not None:
            self._graph_stepper().run(nsteps)
        else:
            self.engines[0].step(nsteps)

    def _graph_stepper(self):
        """``engine.GraphStepper`` of a time-dependent physics on one GPU with
        ``runtime.graph`` (built on first use), else None: eager steps."""
        c = self.cfg.runtime
        if not (self.physics.time_dependent and self.mode == "single" and self.backend == "hip" and c.graph
                and not c.canary and self.device.type == "cuda"):
            return None
        if self._gstepper is None:
            from .engine import GraphStepper
            self._gstepper = GraphStepper(self.engines[0], steps_per_graph=c.steps_per_graph)
        return self._gstepper

    def _sync(self) -> None:
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # ticks per step at the run's initial dt: the watchdog halves dt at most
    # three times, so every interval stays a whole number of steps
    _SUB = 8

    def run(self, nsteps: Optional[int] = None, days: Optional[float] = None) -> Dict[str, Any]:
        """Advance ``nsteps`` steps (or ``days``) of the run's initial dt.

        The loop is graph-aware: history / checkpoint / metrics / watchdog
        intervals cut the run into equal chunks, the native runner records one
        graph of that chunk length (plus the final remainder) before the clock
        starts, and every chunk is one graph replay.  History snapshots and
        metrics are copied device -> pinned host memory on the stepping stream
        and written out while the next chunk runs; the watchdog's finite-check
        is read one chunk late (single-process modes).  The summary reports
        the stepping throughput without setup (``setup_s``: graph capture and
        first replay), plus the host time of each phase (``phase_s``; each phase
        is also a roctx range).

        Watchdog recovery restores a checkpoint, halves the *current* dt and
        continues to the same simulated end time; history frames are indexed by
        simulated time, so replayed intervals overwrite their frames.
        """
        from .utils.tracing import PhaseTimes
        if not self.engines:
            self.initialize()
        c = self.cfg
        if nsteps is None:
            days = days if days is not None else c.time.days
            if days is not None:
                nsteps = int(math.ceil(days * DAY / self.dt - 1e-9))
            else:
                nsteps = c.time.nsteps or 1
        io = c.io
        out = io.output_dir
        ph = PhaseTimes()
        SUB = self._SUB
        dt0, t0 = self.dt, self.time
        end = nsteps * SUB
        level = 0                               # dt = dt0 / 2**level

        def pos() -> int:
            return int(round((self.time - t0) / dt0 * SUB))

        iv = {"history": io.history_interval, "checkpoint": io.checkpoint_interval,
              "metrics": io.metrics_interval, "watchdog": c.runtime.watchdog_interval}
        particles = self._particles
        if particles:                            # chunks end at particle times
            iv["particles"] = self._pinterval
        dissipation = self._dspec is not None
        if dissipation:                          # ... and at dissipation times
            iv["dissipation"] = self._dspec["interval"]
            self._dinterval = self._dspec["interval"]
        iv = {k: v * SUB for k, v in iv.items() if v > 0}
        hist = None
        if "history" in iv:
            n_out = nsteps // io.history_interval + 1
            hpath = os.path.join(out, "history.zarr")
            # io.history_fields: a selection among the prognostic and the derived fields
            hfields = self.fields if io.history_fields is None else list(io.history_fields)
            if self.rank == 0:
                os.makedirs(out, exist_ok=True)
                HistoryWriter(hpath, hfields, self.layout.N, self.layout.n, n_out,
                              attrs={"config": self.config}, frame_chunks=self.mode != "spmd")
            self._barrier()
            hist = HistoryWriter(hpath, hfields, self.layout.N, self.layout.n, n_out, create=False)
        # the frame outputs written beside every history frame, in this order: (producer(der) ->
        # device tensor, None off rank 0; writer on rank 0, else None; host tensor -> the writer's array)
        frames = []
        if hist is not None:
            wattrs = {"config": self.config, "N": self.layout.N}
            as_f64 = lambda h: h.double().numpy()                       # noqa: E731
            if io.latlon is not None:
                # the same frames on the lat-lon grid: the selected fields, or the
                # prognostic ones plus the winds of the shallow-water model
                lfields = list(hfields) if io.history_fields is not None else (
                    self.fields + (list(LATLON_WINDS) if self.physics.name == "swe" and not self.layers() else []))
                hll = LatLonHistoryWriter(os.path.join(out, "history_latlon.zarr"), lfields, io.latlon[0],
                                          io.latlon[1], n_out, attrs=wattrs) if self.rank == 0 else None
                frames.append((lambda der: self._latlon_frame(lfields, der), hll, as_f64))
            if io.spectra is not None:
                snames = list(hfields) + (["ke"] if self.physics.name == "swe" and not self.layers() else [])
                hsp = SpectraHistoryWriter(os.path.join(out, "history_spectra.zarr"), snames, io.spectra, n_out,
                                           attrs=wattrs) if self.rank == 0 else None
                frames.append((lambda der: self._spectra_frame(list(hfields), der), hsp, as_f64))
            if particles and io.particles is not None:      # particles of a config block
                pfields = list(io.particles.get("fields") or [])
                hpa = ParticleHistoryWriter(os.path.join(out, "history_particles.zarr"), pfields, particles[0].K,
                                            n_out, attrs=wattrs) if self.rank == 0 else None
                frames.append((lambda der: self._particles_frame(pfields, der), hpa, self._particles_rows))
        metrics = MetricsLogger(os.path.join(out, "metrics.jsonl") if "metrics" in iv else None,
                                enabled=self.rank == 0)
        cells = 6 * self.layout.N ** 2
        gpu = self.device.type == "cuda"
        deferred = gpu and self.mode != "spmd"
        # (event, host work) done while the next chunks run: on a GPU by one
        # background thread (zarr / JSONL / checkpoint writes release the GIL),
        # so the loop keeps the launch queue full (a history frame's ~100 tile
        # files took ~10 ms of GPU idle per frame when written in the loop)
        pending = _HostQueue(threaded=deferred)

        def drain(block: bool = False) -> None:
            pending.drain(block)

        def chunk_at(p: int, step_ticks: int) -> int:
            nxt = min([(p // v + 1) * v for v in iv.values()] + [end])
            return max(1, (nxt - p) // step_ticks)

        # ---- setup: graphs for the chunk lengths this run replays ------------------
        with ph("setup"):
            if ("checkpoint" in iv and "watchdog" in iv
                    and self.step_count not in ckpt.list_checkpoints(self.checkpoint_root())):
                self.save_checkpoint()      # the watchdog can always roll back to the run's start
            if hist is not None:
                self._snapshot_history(hist, frames, 0, pending, async_copy=False)
                drain(block=True)
            if self._use_native() and nsteps > 0:
                lens, p, it = [], 0, 0
                while p < end and it < 100000:        # the chunk sequence of a run without recovery
                    k = chunk_at(p, SUB)
                    if k not in lens:
                        lens.append(k)
                    p += k * SUB
                    it += 1
                if self.runner is None:
                    self.runner = self._make_runner(chunks=lens)
                per = self.runner.period
                self.runner.graph_periods = max(1, min(max(lens), 512) // per)
                for k in lens[:8]:
                    self.runner.prepare(k)      # chunks shorter than a period: their remainder launch
            if nsteps > 0:
                self._graph_stepper()            # a time-dependent physics: warm-up and capture, before the clock starts
            if dissipation:
                self._dissipations()             # tables and buffers, before the clock starts
            if deferred and ("watchdog" in iv or "metrics" in iv):
                self._warm_checks(derived="metrics" in iv)
            self._sync()
        wall0 = time.perf_counter()
        recoveries = 0
        done = 0
        self._wd_pending = None
        while True:
            p = pos()
            if p >= end:
                break
            st = SUB >> level
            chunk = chunk_at(p, st)
            with ph("step"):
                self._step_model(chunk)
            done += chunk
            drain()
            p = pos()
            if dissipation and p % iv["dissipation"] == 0:
                with ph("dissipation"):
                    self.dissipate()
            if particles and p % iv["particles"] == 0:
                with ph("particles"):
                    self._particles_advance()
            due = {k for k, v in iv.items() if p % v == 0 or p >= end}
            ok, checked = True, False
            if "watchdog" in due:
                with ph("watchdog"):
                    sync_check = not (deferred and "checkpoint" not in due and p < end)
                    ok = self._watchdog(pending, not sync_check)
                    checked = sync_check
            if ok and "checkpoint" in due and p % iv["checkpoint"] == 0 and "watchdog" in iv and not checked:
                # a checkpoint between watchdog intervals: resolve the deferred
                # check and test the state itself, so no checkpoint ever holds a
                # state the watchdog would reject
                with ph("watchdog"):
                    drain(block=True)
                    ok = self._watchdog(pending, False)
            if not ok:
                drain(block=True)                   # checkpoints still being written
                saved = [s for s in ckpt.list_checkpoints(self.checkpoint_root())]
                if recoveries < 3 and saved:
                    recoveries += 1
                    pending.clear()
                    self._wd_pending = None
                    # go back further on each repeated failure (recent checkpoints may
                    # already hold a growing instability)
                    last = ckpt.step_dir(self.checkpoint_root(), saved[-min(recoveries, len(saved))])
                    dt_cur = self.dt
                    self._log(f"watchdog: non-finite state at step {self.step_count}; restarting from {last} "
                              f"with dt/2")
                    self.restore_checkpoint(last)
                    level += 1
                    self.set_dt(dt_cur * 0.5)
                    if abs(self.dt * (1 << level) - dt0) > 1e-9 * dt0:
                        self.set_dt(dt0 / (1 << level))
                    if dissipation:              # tau stays put: twice the steps between applications
                        self._dinterval = self._dspec["interval"] << level
                    if particles:                # the particle times stay put: twice the steps between them
                        for P in particles:
                            P.interval = self._pinterval << level
                        self._particles_stage(1)
                    continue
                raise FloatingPointError(f"non-finite state detected at step {self.step_count}")
            if hist is not None and "history" in due and p % iv["history"] == 0:
                with ph("history"):
                    self._snapshot_history(hist, frames, p // iv["history"], pending, async_copy=deferred)
            if "checkpoint" in due and p % iv["checkpoint"] == 0:
                with ph("checkpoint"):
                    if deferred:
                        self._checkpoint_async(pending)
                    else:
                        drain(block=True)
                        self.save_checkpoint()
            if "metrics" in due:                 # every interval and the end of the run
                with ph("metrics"):
                    self._snapshot_metrics(metrics, pending, deferred, cells, done, wall0, p)
        with ph("drain"):
            self._sync()
            pending.close()
            if self.runner is not None:
                # a producer wait or xGMI poll that timed out sets the kernel's
                # error word and the kernel carries on with stale cells: never
                # report such a run
                self.runner.check()
        wall = time.perf_counter() - wall0
        summary = {"steps": nsteps, "steps_run": done, "wall_s": wall, "setup_s": ph.times.get("setup", 0.0),
                   "sim_days": self.time / DAY,
                   "cell_updates_per_s": cells * done / max(wall, 1e-12),
                   "sim_days_per_day": ((self.time - t0) / DAY) / max(wall / DAY, 1e-30),
                   "recoveries": recoveries, "dt_final": self.dt,
                   "graph_steps": (self.runner.stats["graph_steps"] if self.runner is not None else
                                   self._gstepper.graph_steps if self._gstepper is not None else 0),
                   "runtime": ("fused" if getattr(self, "fused", None) is not None else
                               "native" if self.runner is not None else
                               "graph" if self._gstepper is not None else "eager"),
                   "fused_direct_steps": (self.runner.stats["direct_steps"] if self.runner is not None else 0),
                   "kernel_launches": (self.runner.stats["launches"] if self.runner is not None else 0),
                   "phase_s": dict(ph.times)}
        summary.update(self.diagnostics())
        if self.physics.time_dependent:      # the deformational-flow tests: extrema and the mass against the start
            q = self.global_field(0)
            if q is not None:
                area = self.grid.areas()
                m0 = float((self.physics.initial_global(self.grid) * area).sum())
                summary.update(q_min=float(q.min()), q_max=float(q.max()),
                               mass_drift=float(((q * area).sum() - m0) / m0))
        norms = self.error_norms()
        if norms is not None:
            summary.update({f"err_{k}": v for k, v in norms.items()})
        for j in range(getattr(self.physics, "nq", 0)):
            tn = self.tracer_error_norms(j)
            if tn is not None:
                summary.update({f"tracer{j}_err_{k}": v for k, v in tn.items()})
        self._log(f"Run complete: {done} steps, {summary['sim_days']:.3f} days, "
                  f"{summary['cell_updates_per_s']:.3e} cell-updates/s (setup {summary['setup_s']:.3f} s excluded)")
        if self.physics.time_dependent and "err_l2" in summary:
            self._log(f"Error norms at t = {self.time / self.physics.period:.3f} T: l1 {summary['err_l1']:.4e}, "
                      f"l2 {summary['err_l2']:.4e}, linf {summary['err_linf']:.4e}; q in [{summary['q_min']:.4f}, "
                      f"{summary['q_max']:.4f}], relative mass drift {summary['mass_drift']:.2e}")
        return summary

    # ---- run-loop helpers ----------------------------------------------------------
    def _snapshot_history(self, hist: HistoryWriter, frames, k: int, pending: "_HostQueue",
                          async_copy: bool) -> None:
        """History frame k: the interior values are copied to host memory on
        the stepping stream; the zarr chunks are written when the copy is done
        (``pending``), i.e. while the next chunk steps.  The frame outputs
        ``frames`` (``run``: lat-lon, spectra, particles) follow the same way:
        computed on the stepping stream, staged, written by the host queue.
        Collective under SPMD."""
        t, sc = self.time, self.step_count
        sel = self.cfg.io.history_fields
        # selected fields: the derived ones are computed here, on the stepping stream
        der = self._derived_all() if sel is not None and any(f in DERIVED_FIELDS for f in sel) else None
        vals = []
        mix = self.mix_names()
        for j, e in enumerate(self.engines):
            v = e.tiles_view().detach()
            if sel is not None:
                mq = self._mixing_tiles(e) if any(f in mix for f in sel) else None
                v = torch.stack([der[j][0][DERIVED_FIELDS.index(f)] if f in DERIVED_FIELDS
                                 else mq[mix.index(f)] if f in mix
                                 else v[self.fields.index(f)] for f in sel])
            vals.append(v)
        ev, hs = stage(vals, async_copy)
        snaps = [(e.plan.tiles, h) for e, h in zip(self.engines, hs)]

        def work():
            parts = [(list(tiles), h.double().numpy()) for tiles, h in snaps]
            if hist.frame_chunks and len(parts) > 1:      # every engine of this process in one frame
                parts = [(sum((p_[0] for p_ in parts), []), np.concatenate([p_[1] for p_ in parts], 1))]
            for tiles, arr in parts:
                hist.write_tiles(k, tiles, self.layout.tile_origin, arr)
            if self.rank == 0:
                hist.write_time(k, t, sc)
        pending.append((ev, work))
        for produce, writer, finish in frames:
            v = produce(der)
            if v is None or writer is None:
                continue
            ev, h = stage(v, async_copy)
            pending.append((ev, lambda writer=writer, finish=finish, h=h: writer.write_frame(k, finish(h), t, sc)))

    def _snapshot_metrics(self, metrics: MetricsLogger, pending: List[Any], deferred: bool, cells: int,
                          done: int, wall0: float, p: int) -> None:
        rec = dict(step=self.step_count, time_s=self.time, sim_days=self.time / DAY, dt=self.dt)
        wall = time.perf_counter() - wall0
        rec["cell_updates_per_s"] = cells * done / max(wall, 1e-12)
        swe = self.physics.name == "swe" and not self.layers()      # a layered run: mass0, mass1, energy only
        nq = getattr(self.physics, "nq", 0)
        if not deferred:
            extra = {}
            if swe:
                inv = self.invariants()
                extra = {k: inv[k] for k in METRIC_INVARIANTS}
            if nq:
                extra.update(self.tracer_extrema())
            metrics.log(**rec, **_fold_tracers(self.diagnostics(), nq), **extra)
            return
        keys, vals = [], []
        for e in self.engines:
            for k, v in e.physics.diagnostics(e.tiles_view(), e.tens).items():
                keys.append(k)
                vals.append(v.reshape(()).to(torch.float64))
            if nq:      # extrema of the mixing ratios, through the same pinned copy
                q = self._mixing_tiles(e).reshape(nq, -1).to(torch.float64)
                for k in range(nq):
                    keys += [f"tracer_min_{k}", f"tracer_max_{k}"]
                    vals += [q[k].min(), q[k].max()]
        if swe:      # the one-launch reduction (ops/derived.py), through the same pinned copy
            for _, inv in self._derived_all():
                for k in METRIC_INVARIANTS:
                    keys.append(k)
                    vals.append(inv[INVARIANTS.index(k)])
        ev, h = stage(torch.stack(vals), True)

        def work():
            tot: Dict[str, float] = {}
            for k, v in zip(keys, h.tolist()):
                if k in tot and (k == "max_courant" or k.startswith("tracer_max_")):
                    tot[k] = max(tot[k], v)
                elif k in tot and k.startswith("tracer_min_"):
                    tot[k] = min(tot[k], v)
                else:
                    tot[k] = tot.get(k, 0.0) + v
            metrics.log(**rec, **_fold_tracers(tot, nq))
        pending.append((ev, work))

    def _warm_checks(self, derived: bool = False) -> None:
        """Run the watchdog and metrics reductions once before the clock
        starts.  Their first use in a process loads the kernels' code objects
        and the first pinned host blocks: measured on a 2-day C48 run
        (tools/run_phase_probe.py, profiles/r2_run_phases) that cost ~15 ms
        and took the run from 14.6 to 156 us/step with only the watchdog on."""
        flag = torch.stack([torch.isfinite(e.tiles_view()).all() for e in self.engines]).all()
        vals = [v.reshape(()).to(torch.float64) for e in self.engines
                for v in e.physics.diagnostics(e.tiles_view(), e.tens).values()]
        stage([flag, torch.stack(vals)], True)
        if derived and self.physics.name == "swe" and not self.layers():      # the derived-field kernels of the metrics records
            self._derived_all()
        torch.cuda.current_stream().synchronize()

    def _watchdog(self, pending: List[Any], deferred: bool) -> bool:
        """True while the state is finite.  Deferred (single process): the
        check of this interval is queued and the previous interval's result is
        returned, so the host never waits for the GPU here (a failure is seen
        one interval late; checkpoints drain the queue first, so a checkpoint
        never holds a state the watchdog has not passed)."""
        if not deferred:
            prev, self._wd_pending = self._wd_pending, None
            ok = self.all_finite()
            if prev is not None:
                ok = self._wd_result(prev) and ok
            return ok
        # [finite, no kernel error word set]: the error words of the fused step's
        # producer waits and the xGMI polls travel in the same pinned copy, so a
        # timed-out wait (the kernel then computes on stale cells) is seen one
        # interval late like a non-finite state, and raises
        finite = torch.stack([torch.isfinite(e.tiles_view()).all() for e in self.engines]).all()
        errs = self.runner.err_words() if self.runner is not None else []
        clean = torch.stack([(w[0] == 0) for w in errs]).all() if errs else torch.ones_like(finite)
        prev, self._wd_pending = self._wd_pending, stage(torch.stack([finite, clean]), True)
        if prev is None:
            return True
        return self._wd_result(prev)

    def _wd_result(self, prev) -> bool:
        """Finite flag of a deferred watchdog copy; raises if a kernel error
        word was set (not a numerical failure: no rollback)."""
        prev[0].synchronize()
        if not bool(prev[1][1].item()):
            self.runner.check()
            raise RuntimeError("kernel error word set during the run")
        return bool(prev[1][0].item())

    def set_dt(self, dt: float) -> None:
        self.dt = dt
        for e in self.engines:
            e.dt = dt
        self._gstepper = None        # its graph bakes dt in
        if self.runner is not None:
            self.runner.set_dt(dt)   # graphs bake dt in: the runner re-records

    def _barrier(self) -> None:
        if self.mode == "spmd":
            import torch.distributed as dist
            dist.barrier()

    def _write_history(self, hist: HistoryWriter, k: int) -> None:
        parts = [(list(e.plan.tiles), e.tiles_view().detach().cpu().double().numpy()) for e in self.engines]
        if hist.frame_chunks and len(parts) > 1:
            parts = [(sum((p_[0] for p_ in parts), []), np.concatenate([p_[1] for p_ in parts], 1))]
        for tiles, arr in parts:
            hist.write_tiles(k, tiles, self.layout.tile_origin, arr)
        if self.rank == 0:
            hist.write_time(k, self.time, self.step_count)

    def _checkpoint_async(self, pending: "_HostQueue") -> None:
        """Checkpoint of the current state without stopping the GPU (single
        process): the interior values are copied to pinned host memory on the
        stepping stream and the background writer commits the step directory
        once the copy is done (in order with the history frames before it)."""
        root = self.checkpoint_root()
        step, t, dt = self.step_count, self.time, self.dt
        vals = [e.tiles_view().detach() for e in self.engines]
        if self._particles:
            vals.append(self._particles[0].st.x.detach())
        ev, hs = stage(vals, True)
        snaps = [(e.plan.tiles, h) for e, h in zip(self.engines, hs)]
        px = hs[-1] if self._particles else None

        def work():
            self._write_checkpoint(root, step, t, dt, [(tiles, h.double().numpy()) for tiles, h in snaps],
                                   particles=None if px is None else px.numpy())
        pending.append((ev, work))

    def _write_checkpoint(self, root: str, step: int, t: float, dt: float, parts, particles=None) -> str:
        d = ckpt.step_dir(root, step)
        meta = {"step": step, "time": t, "dt": dt, "N": self.layout.N,
                "tiles_per_edge": self.layout.t, "num_ranks": self.layout.num_ranks,
                "owner": self.layout.owner, "fields": self.fields, "dtype": self.cfg.grid.dtype,
                "integrator": self.cfg.time.integrator, "physics": self.physics.name,
                "config": self.config, "format": "stsphere-ckpt-v1"}
        ckpt.begin(root, step, meta, self.fields, self.layout.N, self.layout.n, np.float64)
        for tiles, arr in parts:
            ckpt.write_tiles(d, self.fields, tiles, self.layout.tile_origin, arr, self.layout.n)
        if particles is not None:
            np.save(os.path.join(d, "particles.npy"), particles)
        ckpt.commit(d)
        ckpt.prune(root, self.cfg.io.keep_checkpoints)
        return d

    # ---- checkpoint / restart ------------------------------------------------------
    def checkpoint_root(self) -> str:
        return self.cfg.io.checkpoint_dir or os.path.join(self.cfg.io.output_dir, "checkpoints")

    def save_checkpoint(self, root: Optional[str] = None) -> str:
        root = root or self.checkpoint_root()
        self._sync()
        step = self.step_count
        d = ckpt.step_dir(root, step)
        if self.rank == 0:
            meta = {"step": step, "time": self.time, "dt": self.dt, "N": self.layout.N,
                    "tiles_per_edge": self.layout.t, "num_ranks": self.layout.num_ranks,
                    "owner": self.layout.owner, "fields": self.fields, "dtype": self.cfg.grid.dtype,
                    "integrator": self.cfg.time.integrator, "physics": self.physics.name,
                    "config": self.config, "format": "stsphere-ckpt-v1"}
            ckpt.begin(root, step, meta, self.fields, self.layout.N, self.layout.n, np.float64)
        self._barrier()
        for e in self.engines:
            ckpt.write_tiles(d, self.fields, e.plan.tiles, self.layout.tile_origin,
                             e.tiles_view().detach().cpu().double().numpy(), self.layout.n)
        self._barrier()
        if self.rank == 0:
            if self._particles:
                np.save(os.path.join(d, "particles.npy"), self._particles[0].st.x.detach().cpu().numpy())
            ckpt.commit(d)
            ckpt.prune(root, self.cfg.io.keep_checkpoints)
        self._barrier()
        return d

    def restore_checkpoint(self, path: str) -> None:
        meta = ckpt.read_meta(path)
        arrs = ckpt.read_fields(path, self.fields)
        if meta["N"] != self.layout.N:
            raise ValueError(f"checkpoint grid C{meta['N']} != configured C{self.layout.N}")
        glob = np.stack([arrs[f] for f in self.fields])           # [F,6,N,N]
        for e in self.engines:
            loc = np.stack([e.geo.gather_global(glob[k]) for k in range(len(self.fields))])
            e.set_state(torch.as_tensor(loc, dtype=self.dtype))
            e.time = float(meta["time"])
            e.step_count = int(meta["step"])
        if self.xgmi is not None:
            self.xgmi.prime()      # remote ghosts of the restored state (collective)
        self.set_dt(float(meta["dt"]))
        pfile = os.path.join(path, "particles.npy")
        self._restored_particles = np.load(pfile) if os.path.exists(pfile) else None
        self._restore_particles()
        self._log(f"Restored {path} (step {meta['step']}, t = {meta['time'] / DAY:.4f} days, "
                  f"written by {meta['num_ranks']} rank(s), tiles_per_edge {meta['tiles_per_edge']})")
