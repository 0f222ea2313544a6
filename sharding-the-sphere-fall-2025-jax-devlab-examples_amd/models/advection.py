"""Tracer advection with a prescribed wind (PDF s.13 / s.18: "Cosine Bell
Advection - Equatorial Band (PLR 2nd-Order)", "Cartesian Velocity Exchange").

    dq/dt + div(q v) = 0

PLR reconstruction + upwind edge flux  F = U * (U > 0 ? q_L : q_R),
U = (v . m) L evaluated from the Cartesian wind at each edge midpoint.
Default case: Williamson TC1 (cosine bell, alpha = 0, bell at 270 E / 0 N
starting on face 3 and moving east onto face 4, as in PDF s.18).

``flow`` selects the wind.  ``solid_body`` is steady: its transports are
evaluated once, in ``setup``.  The deformational flows of Nair & Lauritzen
(2010) and Lauritzen et al. (2012) depend on time (``time_dependent``): the
engine calls ``update`` before every Runge-Kutta stage with the stage time
t_s = (step_count + c_s) dt and the tables ``ex`` / ``ey`` are refilled in place.

* ``deform_nd`` / ``deform_nd_static`` are given by a streamfunction, and the
  transport through an edge is the difference of psi at the edge's two
  vertices: every cell's four transports then sum to zero to rounding, so a
  constant stays constant (the midpoint rule's divergence is O(h^2)).
* ``deform_div`` is divergent: the midpoint rule U = (v . m) L.

At t = m T the initial condition is the exact solution (``exact``).
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from .base import Physics, RankGeometry, reconstruct, recon_halo
from .geometry import DAY, CubedSphereGrid
from . import initial_conditions as ic


class Advection(Physics):
    name = "advection"
    kernel_id = 0
    fields = ["q"]

    @property
    def halo(self) -> int:
        return recon_halo(self.limiter)

    def __init__(self, case: str = "cosine_bell", alpha: float = 0.0, limiter: int = 2, u0: float = None,
                 flow: str = "solid_body", period: float = 12 * DAY):
        if flow != "solid_body" and flow not in ic.DEFORM_FLOWS:
            raise ValueError(f"unknown flow {flow!r}; choose from {['solid_body'] + list(ic.DEFORM_FLOWS)}")
        if not period > 0:
            raise ValueError(f"period must be positive, not {period!r}")
        self.case = case
        self.alpha = alpha
        self.limiter = limiter
        self.u0 = u0
        self.flow = flow
        self.period = float(period)
        self.time_dependent = flow != "solid_body"

    def _u0(self, grid):
        return self.u0 if self.u0 is not None else 2.0 * math.pi * grid.radius / (12.0 * DAY)

    def wind(self, grid, p, t: float = 0.0):
        if self.time_dependent:
            return ic.deform_wind(p, t, self.flow, grid.radius, self.period)
        return ic.solid_body_wind(p, self._u0(grid), self.alpha, grid.radius)

    def initial_global(self, grid: CubedSphereGrid):
        p = grid.centers()
        if self.case == "cosine_bell":
            return ic.cosine_bell(p, radius=grid.radius)
        if self.case == "gaussian":
            return ic.gaussian_hill(p, center=(0.0, -1.0, 0.0), width=0.4, amp=1.0)
        if self.case == "constant":
            return np.ones(p.shape[:-1])
        if self.case in ic.DEFORM_CASES:
            return ic.deform_tracer(p, self.case)
        raise ValueError(self.case)

    def initial_state(self, geo: RankGeometry) -> np.ndarray:
        return geo.gather_global(self.initial_global(geo.grid))[None]

    def exact(self, grid: CubedSphereGrid, t: float, dt: float = None):
        """TC1: the bell rotated rigidly about the tilted axis; None for
        cases without a closed form.  A deformational flow returns every field
        to its start: the initial field when t is within dt / 2 (default: of
        ``max_dt``) of a multiple of the period, else None."""
        if self.time_dependent:
            m = round(t / self.period)
            if abs(t - m * self.period) > 0.5 * (self.max_dt(grid) if dt is None else dt):
                return None
            return self.initial_global(grid)
        if self.case != "cosine_bell":
            return None
        return ic.cosine_bell_exact(grid.centers(), t, self.alpha, radius=grid.radius, u0=self._u0(grid))

    def vertex_lonlat(self, geo: RankGeometry):
        """(lon, lat) [T, n+1, n+1] of the rank's tile vertices, sliced from the
        global vertex array: a vertex shared by tiles or ranks of one panel
        carries the same bits on each."""
        if getattr(geo, "_vertex_lonlat", None) is None:      # kept on the geometry it belongs to
            from .geometry import xyz_to_lonlat
            n = geo.n
            lon, lat = xyz_to_lonlat(geo.grid.vertices())
            vl = np.empty((geo.T, n + 1, n + 1))
            vt = np.empty((geo.T, n + 1, n + 1))
            for li, tid in enumerate(geo.plan.tiles):
                f, I0, J0 = geo.layout.tile_origin(tid)
                vl[li] = lon[f, J0:J0 + n + 1, I0:I0 + n + 1]
                vt[li] = lat[f, J0:J0 + n + 1, I0:I0 + n + 1]
            geo._vertex_lonlat = (vl, vt)
        return geo._vertex_lonlat

    def midpoint_transports(self, geo: RankGeometry, t: float = 0.0):
        """U = (v . m) L at the edge midpoints: (ex [T, n, n+1], ey [T, n+1, n]), float64."""
        ux = np.sum(self.wind(geo.grid, geo.xmid, t) * geo.mx[:, None, :, :], axis=-1) * geo.lx
        uy = np.sum(self.wind(geo.grid, geo.ymid, t) * geo.my[:, :, None, :], axis=-1) * geo.ly
        return ux, uy

    def streamfunction(self, geo: RankGeometry, t: float = 0.0) -> np.ndarray:
        """psi [T, n+1, n+1] at the rank's tile vertices (the streamfunction flows)."""
        lon, lat = self.vertex_lonlat(geo)
        return ic.deform_streamfunction(lon, lat, t, self.flow, geo.grid.radius, self.period)

    def transports(self, geo: RankGeometry, t: float = 0.0):
        """Edge transports (ex [T, n, n+1], ey [T, n+1, n]) at time t, float64:
        vertex differences of psi for the streamfunction flows, else the
        midpoint rule."""
        if self.flow in ic.STREAM_FLOWS:
            psi = self.streamfunction(geo, t)
            return -(psi[:, 1:, :] - psi[:, :-1, :]), psi[:, :, 1:] - psi[:, :, :-1]
        return self.midpoint_transports(geo, t)

    def update(self, geo: RankGeometry, tens: Dict[str, torch.Tensor], t: float) -> None:
        """Refill ``ex`` / ``ey`` in place with the transports at time t."""
        for key, u in zip(("ex", "ey"), self.transports(geo, t)):
            tens[key].copy_(torch.as_tensor(np.ascontiguousarray(u)))

    def setup(self, geo: RankGeometry, dtype, device) -> Dict[str, torch.Tensor]:
        ux, uy = self.transports(geo, 0.0) if self.time_dependent else self.midpoint_transports(geo)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)
        return {"area": t(geo.area), "invA": t(1.0 / geo.area), "ex": t(ux), "ey": t(uy),
                "pedge": torch.as_tensor(geo.pedge, device=device),   # [T] panel-edge side bits
                "pe_base": torch.as_tensor(geo.pe_base, device=device),   # [T,4,3,n] panel-edge ghost stencils
                "pe_t": t(geo.pe_t)}

    def kernel_params(self):
        return {"limiter": self.limiter}

    def rhs(self, qe, qi, tens, n, g):
        (qL, qR, _, _), (yL, yR, _, _) = reconstruct(qe, tens, g, n, self.limiter)
        U = tens["ex"]
        Fx = U * torch.where(U > 0, qL, qR)
        qL, qR = yL, yR
        V = tens["ey"]
        Gy = V * torch.where(V > 0, qL, qR)
        return -((Fx[..., 1:] - Fx[..., :-1]) + (Gy[..., 1:, :] - Gy[..., :-1, :])) * tens["invA"]

    def max_dt(self, grid: CubedSphereGrid, cfl: float = 0.9) -> float:
        """2-D unsplit bound dt * |v| * (1/dx + 1/dy) <= cfl."""
        if self.time_dependent:      # |v| <= k + 2 pi R / T
            vmax = ic.deform_amplitude(self.flow, grid.radius, self.period) + 2.0 * math.pi * grid.radius / self.period
            return cfl * grid.min_spacing() / (2.0 * vmax)
        return cfl * grid.min_spacing() / (2.0 * self._u0(grid))
