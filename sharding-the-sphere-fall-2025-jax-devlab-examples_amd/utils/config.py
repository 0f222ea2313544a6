"""YAML configuration ("Tile Specification (config.yaml)", PDF s.7 / s.8).

The reference reads ``self.config['parallelization']`` with ``.get`` defaults
``device_type='cpu'``, ``num_devices=6``, ``tiles_per_edge=1`` (PY:21-24); its
slide shows the same three keys in ``config.yaml`` (PDF s.8 img).  Those keys and
their validation semantics are kept exactly; the other sections (grid, physics,
time, io, runtime) configure the parts the reference only describes.

    parallelization:
      tiles_per_edge: 1      # 6 t^2 tiles: 1 -> 6, 2 -> 24, 3 -> 54
      num_devices: 6         # <= 6 t^2 and must divide it
      device_type: 'gpu'     # or 'cpu' for testing (virtual devices / gloo)
      partition: auto        # contiguous | corner | auto
    grid:    {N: 96, halo: 2, dtype: float64}
    physics: {model: swe, case: tc5, limiter: mc}
    time:    {integrator: ssprk3, dt: null, cfl: 0.9, nsteps: 100, days: null}
    io:      {output_dir: run, history_interval: 0, checkpoint_interval: 0,
              geometry: grid.zarr, initial_condition: ic.zarr, ...}
    runtime: {backend: auto, graph: true, steps_per_graph: 30, comm: auto, ...}
"""
from __future__ import annotations

import copy
import dataclasses
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Union

import yaml


@dataclass
class ParallelConfig:
    tiles_per_edge: int = 1
    num_devices: int = 6
    device_type: str = "cpu"
    partition: str = "auto"


@dataclass
class GridConfig:
    N: int = 48
    halo: int = 2
    dtype: str = "float64"
    radius: Optional[float] = None


@dataclass
class PhysicsConfig:
    model: str = "swe"            # swe | advection | diffusion | planar_swe (single flat panel)
    case: Optional[str] = None    # tc2 | tc5 | tc6 | galewsky | galewsky_balanced | rest | cosine_bell | gaussian | lima_flag | harmonic | harmonic32
    limiter: str = "mc"
    alpha: float = 0.0
    # advection only: the prescribed wind.  solid_body (steady) | deform_nd | deform_nd_static |
    # deform_div: the deformational flows of Nair & Lauritzen (2010) / Lauritzen et al. (2012),
    # which depend on time, reverse at period / 2 and return the tracer at `period_days`
    # (cases cosine_bells | gaussian_hills | slotted_cylinders); null = solid_body, 12 days
    flow: Optional[str] = None
    period_days: Optional[float] = None
    kappa: float = 2.0e6
    # diffusion only: the Laplacian.  two_point: the flux kappa L / d across every edge
    # (conservative, monotone, not consistent: the error does not fall under
    # refinement); consistent: the corrected flux of models/dissipation.py (second
    # order, conservative, not monotone; two launches per stage, eager stepping)
    operator: str = "two_point"
    # shallow water only: initial conditions of up to 4 passive tracers carried by
    # the flow (models/initial_conditions.py::tracer_field: constant | cosine_bell |
    # cap | gradient); null or empty = none
    tracers: Optional[List[str]] = None
    # with tracers: null = the mixing ratios use `limiter`; ppm = the mixing ratios
    # alone on the monotone PPM (halo 3) while (h, v) keep `limiter`
    tracer_limiter: Optional[str] = None
    # shallow water only: scale-selective dissipation applied between model steps
    # (models/dissipation.py): {order: 1 | 2, nu: m^2/s (order 1) or m^4/s (order 2),
    # interval: steps between applications (default 1), depth: diffuse the free
    # surface too (default true; false with tracers)}; null = off
    dissipation: Optional[Dict[str, Any]] = None
    # shallow water only: stacked (isopycnal) layers, models/swe.py::LayeredShallowWater:
    # {depths: [H_0, H_1] resting depths from the top (m), density_ratio: rho_0 / rho_1
    # (default 0.9), winds: [w_0, w_1] layer winds of case tc2 as fractions of TC2's u0,
    # jet_scale: the Galewsky wind's factor in layered_jet (default 0.25)}; cases tc2 |
    # rest | tc5 | layered_jet | layered_jet_balanced; null = one homogeneous layer
    layers: Optional[Dict[str, Any]] = None


@dataclass
class TimeConfig:
    integrator: str = "ssprk3"
    dt: Optional[float] = None
    cfl: Optional[float] = None
    nsteps: Optional[int] = None
    days: Optional[float] = None


@dataclass
class IOConfig:
    output_dir: str = "run"
    history_interval: int = 0          # steps; 0 = off
    history_fields: Optional[List[str]] = None
    checkpoint_interval: int = 0       # steps; 0 = off
    checkpoint_dir: Optional[str] = None
    keep_checkpoints: int = 3
    metrics_interval: int = 0          # steps; 0 = off
    restore: Optional[str] = None      # checkpoint path or "latest"
    # pipeline stages of PDF s.6 ("Geometry: jax.zarr", "Initial Conditions:
    # jax.zarr"): a zarr group written on the first run, read when present
    geometry: Optional[str] = None
    initial_condition: Optional[str] = None
    # [nlat, nlon]: every history frame is also written on the cell-centred
    # lat-lon grid, to history_latlon.zarr (models/latlon.py); null = off
    latlon: Optional[List[int]] = None
    # L: every history frame's power per degree 0 .. L (and the kinetic-energy
    # spectrum of the shallow-water model) goes to history_spectra.zarr
    # (models/spectra.py); null = off
    spectra: Optional[int] = None
    # passive particles of the shallow-water model (models/points.py):
    # {count: K, seed: s} (uniform on the sphere) or {lat: [...], lon: [...]}
    # (radians), optional interval (steps per particle advance, default 1) and
    # fields (sampled at the particles); every history frame's positions go to
    # history_particles.zarr; null = off
    particles: Optional[Dict[str, Any]] = None


@dataclass
class RuntimeConfig:
    backend: str = "auto"              # auto | hip | torch
    graph: bool = True
    steps_per_graph: int = 30
    comm: str = "auto"                 # auto | xgmi | ipc | rccl | torch | staged  (auto: xgmi on GPUs)
    watchdog_interval: int = 0         # steps; 0 = off
    canary: bool = False               # NaN-prefill ghost slots and check after exchanges (debug)
    block: Optional[List[int]] = None
    # fused SSP-RK3 step (ops/fused.py, one launch for several steps): auto = where
    # the shallow-water setup supports it and every block of a rank is resident
    fused: str = "auto"                # auto | on | off
    steps_per_launch: int = 0          # fused multi-step launches; 0 = from the run's chunk length
    # pipelined streaming step (ops/march3.py: one march launch per step for the
    # tile interiors + two band launches) on one GPU where the streaming stage
    # applies (large grids): auto | on | off
    march3: str = "auto"
    march3_rows: int = 32


@dataclass
class Config:
    parallelization: ParallelConfig = field(default_factory=ParallelConfig)
    grid: GridConfig = field(default_factory=GridConfig)
    physics: PhysicsConfig = field(default_factory=PhysicsConfig)
    time: TimeConfig = field(default_factory=TimeConfig)
    io: IOConfig = field(default_factory=IOConfig)
    runtime: RuntimeConfig = field(default_factory=RuntimeConfig)

    def to_dict(self) -> Dict[str, Any]:
        return dataclasses.asdict(self)


_SECTIONS = {"parallelization": ParallelConfig, "grid": GridConfig, "physics": PhysicsConfig,
             "time": TimeConfig, "io": IOConfig, "runtime": RuntimeConfig}


def _build(cls, d: Optional[Dict[str, Any]]):
    d = dict(d or {})
    names = {f.name for f in dataclasses.fields(cls)}
    unknown = set(d) - names
    if unknown:
        raise ValueError(f"unknown keys in {cls.__name__}: {sorted(unknown)}")
    return cls(**d)


def load_config(src: Union[str, Dict[str, Any], Config, None] = None) -> Config:
    """Parse a YAML path, YAML text, dict or Config into a Config."""
    if src is None:
        return Config()
    if isinstance(src, Config):
        return copy.deepcopy(src)
    if isinstance(src, str):
        if os.path.exists(src):
            with open(src) as f:
                d = yaml.safe_load(f)
        else:
            d = yaml.safe_load(src)
            if not isinstance(d, dict):
                raise FileNotFoundError(src)
    else:
        d = copy.deepcopy(src)
    d = d or {}
    unknown = set(d) - set(_SECTIONS)
    if unknown:
        raise ValueError(f"unknown config sections: {sorted(unknown)}")
    return Config(**{k: _build(cls, d.get(k)) for k, cls in _SECTIONS.items()})


def save_config(cfg: Config, path: str) -> None:
    with open(path, "w") as f:
        yaml.safe_dump(cfg.to_dict(), f, sort_keys=False)


def default_case(model: str) -> str:
    return {"swe": "tc5", "advection": "cosine_bell", "diffusion": "lima_flag", "planar_swe": "gaussian"}[model]
