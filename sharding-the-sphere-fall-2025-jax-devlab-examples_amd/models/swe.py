"""Shallow-water equations on the cubed sphere (PY:2 "FV Cubed-Sphere Shallow
Water Solver").

Formulation (chosen here; the reference does not show one):

* state per cell: depth h and **Cartesian momentum** M = h v (3 components),
  panel-invariant, so halos need no basis rotation (PDF s.18, "Cartesian
  Velocity Exchange");
* flux form  d(h, M)/dt + div(h v, M v + g h^2/2 I) = S,  FV with PLR on the
  primitive variables (h, v) and a Rusanov (local Lax-Friedrichs) edge flux
  along the exact great-circle edge normals; the Rusanov speed is
  max(|v.m| + sqrt(g h)) over the two adjacent cell averages;
* sources: Coriolis  -f r x M  (f = 2 Omega z/R), topography  -g h grad b, and
  the curvature balance  +g h_c^2 / 2 * (sum m L) / A, which makes a constant
  depth exactly force-free on the curved cell;
* after each stage M is projected onto the tangent plane at the cell centre
  (removes the radial "constraint force" of motion on the sphere).
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch

from .base import PPM, Physics, RankGeometry, reconstruct, recon_halo
from .geometry import GRAVITY, OMEGA, CubedSphereGrid
from . import initial_conditions as ic


class ShallowWater(Physics):
    name = "swe"
    kernel_id = 2
    fields = ["h", "mx", "my", "mz"]

    @property
    def halo(self) -> int:
        return recon_halo(self.limiter)

    def __init__(self, case: str = "tc5", limiter: int = 2, g: float = GRAVITY, omega: float = OMEGA,
                 alpha: float = 0.0):
        self.case = case
        self.limiter = limiter
        self.g = g
        self.omega = omega
        self.alpha = alpha
        self._b_global = None

    # ---- initial conditions --------------------------------------------
    def global_fields(self, grid: CubedSphereGrid):
        p = grid.centers()
        if self.case == "tc2":
            h, wind, b = ic.williamson_tc2(p, alpha=self.alpha, radius=grid.radius, omega=self.omega, g=self.g)
        elif self.case == "tc5":
            h, wind, b = ic.williamson_tc5(p, radius=grid.radius, omega=self.omega, g=self.g)
        elif self.case == "tc6":
            h, wind, b = ic.williamson_tc6(p, radius=grid.radius, omega=self.omega, g=self.g)
        elif self.case in ("galewsky", "galewsky_balanced"):
            h, wind, b = ic.galewsky(p, perturbed=self.case == "galewsky", radius=grid.radius, omega=self.omega,
                                     g=self.g)
        elif self.case == "rest":
            h = np.full(p.shape[:-1], 1000.0)
            wind = np.zeros(p.shape)
            b = np.zeros(p.shape[:-1])
        else:
            raise ValueError(f"unknown SWE case {self.case!r}")
        return h, wind, b

    def exact(self, grid: CubedSphereGrid, t: float):
        """True depth h(t) where the case has one: TC2 (steady geostrophic
        flow) and the lake at rest keep their initial depth; else None."""
        if self.case in ("tc2", "rest"):
            return self.global_fields(grid)[0]
        return None

    def initial_state(self, geo: RankGeometry) -> np.ndarray:
        h, wind, b = self.global_fields(geo.grid)
        hl = geo.gather_global(h)
        wl = geo.gather_global(wind)
        q = np.empty((4,) + hl.shape)
        q[0] = hl
        q[1:] = np.moveaxis(hl[..., None] * wl, -1, 0)
        return q

    # ---- geometry ---------------------------------------------------------
    def setup(self, geo: RankGeometry, dtype, device) -> Dict[str, torch.Tensor]:
        _, _, b = self.global_fields(geo.grid)
        gb = geo.fv_gradient(b)
        # curvature balance  g/2 * sum_e(+-L_e m_e) / A  per cell (metric term)
        mlx = geo.lx[..., None] * geo.mx[:, None, :, :]
        mly = geo.ly[..., None] * geo.my[:, :, None, :]
        S = (mlx[:, :, 1:] - mlx[:, :, :-1]) + (mly[:, 1:] - mly[:, :-1])
        sbal = 0.5 * self.g * S / geo.area[..., None]
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)
        return {
            "area": t(geo.area),
            "invA": t(1.0 / geo.area),
            "ex": t(geo.lx),
            "ey": t(geo.ly),
            "mx": t(np.moveaxis(geo.mx, -1, 1)),           # [T,3,n+1]
            "my": t(np.moveaxis(geo.my, -1, 1)),
            "ctr": t(np.moveaxis(geo.center, -1, 0)),      # [3,T,n,n]
            "gradb": t(np.moveaxis(gb, -1, 0)),            # [3,T,n,n]
            "sbal": t(np.moveaxis(sbal, -1, 0)),           # [3,T,n,n]
            # HIP kernel: one 16-byte-aligned record per cell (1/A, centre, grad b, 0)
            "cgeo": t(np.concatenate([(1.0 / geo.area)[..., None], geo.center, gb,
                                      np.zeros(geo.area.shape + (1,))], axis=-1)),   # [T,n,n,8]
            "b": t(geo.gather_global(b)),
            "pedge": torch.as_tensor(geo.pedge, device=device),   # [T] panel-edge side bits
            "pe_base": torch.as_tensor(geo.pe_base, device=device),   # [T,4,3,n] panel-edge ghost stencils
            "pe_t": t(geo.pe_t),
        }

    def kernel_params(self):
        return {"g": self.g, "omega2": 2.0 * self.omega, "limiter": self.limiter}

    # ---- reference RHS ------------------------------------------------------
    def _flux(self, wL, wR, cL, cR, m, L):
        g = self.g
        hL, hR = wL[0], wR[0]
        vL, vR = wL[1:], wR[1:]
        vnL = (vL * m).sum(0)
        vnR = (vR * m).sum(0)
        sL = ((cL[1:] * m).sum(0)).abs() + torch.sqrt(g * cL[0])
        sR = ((cR[1:] * m).sum(0)).abs() + torch.sqrt(g * cR[0])
        c = torch.maximum(sL, sR)
        Fh = 0.5 * (hL * vnL + hR * vnR) - 0.5 * c * (hR - hL)
        Fm = 0.5 * (hL * vL * vnL + hR * vR * vnR + 0.5 * g * (hL * hL + hR * hR) * m) - 0.5 * c * (hR * vR - hL * vL)
        return torch.cat([Fh[None], Fm], 0) * L

    def rhs(self, qe, qi, tens, n, g):
        h = qe[0]
        safe = torch.where(h != 0, h, torch.ones_like(h))
        w = torch.stack([h, qe[1] / safe, qe[2] / safe, qe[3] / safe])
        (wL, wR, cL, cR), (yL, yR, dL, dR) = reconstruct(w, tens, g, n, self.limiter)   # x: [4,T,n,n+1]
        mx = tens["mx"].permute(1, 0, 2)[:, :, None, :]              # [3,T,1,n+1]
        Fx = self._flux(wL, wR, cL, cR, mx, tens["ex"])
        wL, wR, cL, cR = yL, yR, dL, dR                             # y: [4,T,n+1,n]
        my = tens["my"].permute(1, 0, 2)[:, :, :, None]              # [3,T,n+1,1]
        Gy = self._flux(wL, wR, cL, cR, my, tens["ey"])
        invA = tens["invA"]
        dq = -((Fx[..., 1:] - Fx[..., :-1]) + (Gy[..., 1:, :] - Gy[..., :-1, :])) * invA
        hc = qi[0]
        M = qi[1:4]
        r = tens["ctr"]
        f = self.omega * 2.0 * r[2]
        cor = torch.stack([r[1] * M[2] - r[2] * M[1], r[2] * M[0] - r[0] * M[2], r[0] * M[1] - r[1] * M[0]])
        dq[1:] += -f * cor + (hc * hc) * tens["sbal"] - self.g * hc * tens["gradb"]
        return dq

    def finalize(self, out, tens):
        r = tens["ctr"]
        M = out[1:4]
        d = (M * r).sum(0)
        out[1:4] = M - d * r
        return out

    def max_dt(self, grid: CubedSphereGrid, cfl: float = 0.9) -> float:
        """2-D unsplit bound: dt * speed * (1/dx + 1/dy) <= cfl."""
        h, wind, b = self.global_fields(grid)
        speed = np.linalg.norm(wind, axis=-1) + np.sqrt(self.g * np.maximum(h, 0))
        return cfl * grid.min_spacing() / (2.0 * float(speed.max()))

    def derived(self, q, recv, gmap, cmap, tens, tabs, order, T, n, ng, dt):
        """Relative vorticity, divergence, potential vorticity [3, T, n, n] and
        the invariants [8] of the padded state q [4, S] (models/derived.py:
        the PyTorch twin of ops/csrc/derived_kernel.hip).  ``tabs`` / ``order``:
        ``derived.derived_tables`` / ``derived.face_order`` of the rank."""
        from .derived import derived_twin
        return derived_twin(q, recv, gmap, cmap, tens, tabs, order, T, n, ng, self.g, 2.0 * self.omega, dt)

    def diagnostics(self, qi, tens):
        A = tens["area"]
        h = qi[0]
        M = qi[1:4]
        b = tens["b"]
        ke = 0.5 * (M * M).sum(0) / h
        pe = 0.5 * self.g * h * h + self.g * h * b
        return {"mass": (h * A).sum(), "energy": ((ke + pe) * A).sum()}


MAX_TRACERS = 4


class ShallowWaterTracers(ShallowWater):
    """Shallow water carrying NQ passive tracers (1 <= NQ <= 4).

    State (h, M, hq_0 .. hq_{NQ-1}) with hq_k = h q_k, tracer mass per unit
    area.  The mixing ratios q_k = hq_k / h (0 where h = 0) are reconstructed
    like h and v (same limiter, same panel-edge treatment) and ride the depth
    flux of the same stage:  F_hq = F_h (F_h > 0 ? qL : qR).  Hence sum(hq A) is
    conserved like the mass and q = const stays constant, which no scheme that
    advects q with winds sampled from the SWE state can offer.  No source term,
    no tangent projection.  The SWE rows are the parent's operations in the
    parent's order: bit-identical to ``ShallowWater``.

    ``tracers``: initial conditions, names of ``initial_conditions.tracer_field``
    (or numbers: a constant mixing ratio).  PLR limiters only for (h, v).

    ``tracer_limiter``: None (the mixing ratios use ``limiter``) or "ppm" / 4:
    the mixing ratios alone are reconstructed by the monotone PPM
    (``base.ppm_faces(..., monotone=True)``: interface values confined between
    their two cells, then the Colella-Woodward limiter) on a three-layer window,
    while (h, v) keep ``limiter``; (h, M) stay bit-for-bit those of a plain
    run."""
    kernel_id = 3

    def __init__(self, case: str = "tc5", tracers=("cap",), tracer_limiter=None, **kw):
        super().__init__(case, **kw)
        if tracer_limiter in ("ppm", PPM):
            self.tracer_limiter = PPM
        elif tracer_limiter is None:
            self.tracer_limiter = None
        else:
            raise ValueError(f"shallow water with tracers: tracer_limiter is None or 'ppm', got {tracer_limiter!r}")
        tracers = list(tracers)
        if not 1 <= len(tracers) <= MAX_TRACERS:
            raise ValueError(f"shallow water with tracers: 1 to {MAX_TRACERS} tracers, got {len(tracers)}")
        if self.limiter == PPM:
            raise ValueError("shallow water with tracers: PPM (limiter 4) is not supported, the tracer "
                             "stage kernel reconstructs with the PLR limiters 0 to 3 only")
        for name in tracers:
            if isinstance(name, str) and name not in ic.TRACER_FIELDS:
                raise ValueError(f"unknown tracer initial condition {name!r}; choose from {list(ic.TRACER_FIELDS)}")
        self.tracers = tracers
        self.nq = len(tracers)
        self.fields = ["h", "mx", "my", "mz"] + [f"hq{k}" for k in range(self.nq)]

    def tracer_fields(self, grid: CubedSphereGrid) -> np.ndarray:
        """Initial mixing ratios [NQ, 6, N, N]."""
        p = grid.centers()
        return np.stack([ic.tracer_field(name, p, radius=grid.radius) for name in self.tracers])

    def initial_state(self, geo: RankGeometry) -> np.ndarray:
        q4 = super().initial_state(geo)
        q = self.tracer_fields(geo.grid)
        return np.concatenate([q4] + [(q4[0] * geo.gather_global(q[k]))[None] for k in range(self.nq)], 0)

    @property
    def halo(self) -> int:
        return 3 if self.tracer_limiter == PPM else recon_halo(self.limiter)

    def kernel_params(self):
        return dict(super().kernel_params(), nq=self.nq, tracer_limiter=self.tracer_limiter or 0)

    def tracer_exact(self, grid: CubedSphereGrid, t: float, k: int):
        """True mixing ratio q_k(t) [6, N, N] where it has a closed form: a
        ``cosine_bell`` on TC2, whose wind is TC1's solid-body rotation, is the
        rotated bell; else None."""
        if not 0 <= int(k) < self.nq:
            raise ValueError(f"tracer_exact({k}): this physics carries {self.nq} tracer(s)")
        if self.case == "tc2" and self.tracers[int(k)] == "cosine_bell":
            return ic.cosine_bell_exact(grid.centers(), t, self.alpha, radius=grid.radius, h0=1.0)
        return None

    def rhs(self, qe, qi, tens, n, g):
        h = qe[0]
        safe = torch.where(h != 0, h, torch.ones_like(h))
        w = torch.cat([h[None], qe[1:] / safe])                      # h, v, q_k (0 where h = 0)
        if self.tracer_limiter == PPM:    # (h, v): the parent's call; q_k: monotone PPM on the same window
            (wL, wR, cL, cR), (yL, yR, dL, dR) = reconstruct(w[:4], tens, g, n, self.limiter)
            (tL, tR, _, _), (uL, uR, _, _) = reconstruct(w[4:], tens, g, n, PPM, monotone=True)
            wL, wR, yL, yR = torch.cat([wL, tL]), torch.cat([wR, tR]), torch.cat([yL, uL]), torch.cat([yR, uR])
        else:
            (wL, wR, cL, cR), (yL, yR, dL, dR) = reconstruct(w, tens, g, n, self.limiter)
        mx = tens["mx"].permute(1, 0, 2)[:, :, None, :]
        Fx = self._flux(wL[:4], wR[:4], cL[:4], cR[:4], mx, tens["ex"])
        my = tens["my"].permute(1, 0, 2)[:, :, :, None]
        Gy = self._flux(yL[:4], yR[:4], dL[:4], dR[:4], my, tens["ey"])
        Tx = Fx[0] * torch.where(Fx[0] > 0, wL[4:], wR[4:])          # upwind mixing ratio on the depth flux
        Ty = Gy[0] * torch.where(Gy[0] > 0, yL[4:], yR[4:])
        Fx = torch.cat([Fx, Tx])
        Gy = torch.cat([Gy, Ty])
        invA = tens["invA"]
        dq = -((Fx[..., 1:] - Fx[..., :-1]) + (Gy[..., 1:, :] - Gy[..., :-1, :])) * invA
        hc = qi[0]
        M = qi[1:4]
        r = tens["ctr"]
        f = self.omega * 2.0 * r[2]
        cor = torch.stack([r[1] * M[2] - r[2] * M[1], r[2] * M[0] - r[0] * M[2], r[0] * M[1] - r[1] * M[0]])
        dq[1:4] += -f * cor + (hc * hc) * tens["sbal"] - self.g * hc * tens["gradb"]
        return dq

    def mixing_ratio(self, qi, k: int):
        """q_k = hq_k / h of an interior state [F, ...] (0 where h = 0)."""
        h = qi[0]
        return torch.where(h != 0, qi[4 + k] / torch.where(h != 0, h, torch.ones_like(h)), torch.zeros_like(h))

    def diagnostics(self, qi, tens):
        d = super().diagnostics(qi, tens)
        A = tens["area"]
        for k in range(self.nq):
            d[f"tracer_mass_{k}"] = (qi[4 + k] * A).sum()
        return d
