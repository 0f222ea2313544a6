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


class LayeredShallowWater(ShallowWater):
    """Stacked (isopycnal) shallow water: L layers of constant density, layer 0
    on top, rho_0 < ... < rho_{L-1}.

    State (h_0, M_0, h_1, M_1, ...), field-major, M_k = h_k v_k Cartesian.  Layer
    k is the parent's layer (PLR on (h_k, v_k), panel-edge treatment, Rusanov
    flux, curvature balance, Coriolis, static -g h_k grad b, tangent projection,
    the h = 0 guard of the primitive division) over a topography that moves, the
    other layers:

    * the momentum source gains  -g h_k grad(c_k)  with
      c_k = sum_{j<k} (rho_j / rho_k) h_j + sum_{j>k} h_j  (layers above press
      with their density ratio, layers below lift with weight 1), so that
      b + c_k + h_k is the layer's Montgomery height.  grad(c_k) is the Gauss
      sum over the four faces of (cbar_face - c_cell) m L / A with the face's
      sign, projected onto the tangent plane at the cell centre; cbar_face is
      the mean (hL + hR) / 2 of the contributing layers' reconstructed edge
      states, the states the flux uses (single-valued across a cube edge).
      c_cell is subtracted before anything is multiplied: uniform layers give
      exactly zero;
    * the Rusanov speed of every layer is |v_k . m| + sqrt(g H), H = sum_j h_j
      of the cell averages, the larger of the two adjacent cells: sqrt(g H)
      bounds the external and all internal wave speeds while the densities
      increase downwards.

    With one layer every operation is the parent's in the parent's order:
    bit-identical to ``ShallowWater``.  PLR limiters only.

    ``depths``: resting depths [H_0, ..]; None = one layer with the case's own
    depth (the parent's cases).  Two layers take the cases of
    ``initial_conditions.layered_fields``; more than two only ``rest``.
    ``density_ratio`` r = rho_k / rho_{k+1} of adjacent layers.

    Diagnostics: mass_k = sum(h_k A) and one energy
    sum_k (rho_k / rho_{L-1}) [ |M_k|^2 / (2 h_k) + g h_k (b + sum_{j>k} h_j + h_k / 2) ] A,
    whose derivative by h_k is (rho_k / rho_{L-1}) g times the Montgomery height
    b + c_k + h_k above."""
    kernel_id = 4

    def __init__(self, case: str = "tc2", depths=None, density_ratio: float = 0.9, winds=None, jet_scale=None, **kw):
        super().__init__(case, **kw)
        if self.limiter == PPM:
            raise ValueError("layered shallow water: PPM (limiter 4) is not supported, the layer stage kernel "
                             "reconstructs with the PLR limiters 0 to 3 only")
        self.depths = None if depths is None else [float(H) for H in depths]
        self.nl = 1 if self.depths is None else len(self.depths)
        if self.nl < 1:
            raise ValueError("layered shallow water: depths needs at least one layer")
        self.density_ratio = float(density_ratio)
        if self.nl > 1 and not 0.0 < self.density_ratio < 1.0:
            raise ValueError(f"layered shallow water: density_ratio = rho_0 / rho_1 in (0, 1) expected, "
                             f"not {density_ratio!r}")
        self.winds = None if winds is None else [float(w) for w in winds]
        self.jet_scale = None if jet_scale is None else float(jet_scale)
        if self.nl == 2 and case not in ic.LAYER_CASES:
            raise ValueError(f"unknown layered shallow-water case {case!r}; choose from {list(ic.LAYER_CASES)}")
        if self.nl > 2 and case != "rest":
            raise ValueError(f"layered shallow water with {self.nl} layers has the case 'rest' only, not {case!r}")
        L = self.nl
        self.rho = [self.density_ratio ** (L - 1 - k) for k in range(L)]     # relative to the bottom layer
        # coupling weights: c_k = sum_j cw[k][j] h_j
        self.cw = [[(self.rho[j] / self.rho[k] if j < k else 1.0) if j != k else 0.0 for j in range(L)]
                   for k in range(L)]
        self.fields = [f"{name}{k}" for k in range(L) for name in ("h", "mx", "my", "mz")]

    # ---- initial conditions --------------------------------------------
    def global_fields(self, grid: CubedSphereGrid):
        """(h, wind, b): the parent's arrays with one layer, else h [L, 6, N, N]
        and wind [L, 6, N, N, 3]."""
        if self.nl == 1:
            return super().global_fields(grid)
        p = grid.centers()
        if self.nl == 2:
            return ic.layered_fields(self.case, p, self.depths, self.density_ratio, self.winds, self.jet_scale,
                                     alpha=self.alpha, radius=grid.radius, omega=self.omega, g=self.g)
        zero = np.zeros(p.shape[:-1])
        return np.stack([zero + H for H in self.depths]), np.zeros((self.nl,) + p.shape), zero

    def layer_fields(self, grid: CubedSphereGrid):
        """(h [L, 6, N, N], wind [L, 6, N, N, 3], b) for any L."""
        h, wind, b = self.global_fields(grid)
        return (h[None], wind[None], b) if self.nl == 1 else (h, wind, b)

    def exact(self, grid: CubedSphereGrid, t: float):
        """True depths where the case is steady (tc2, rest): [6, N, N] with one
        layer, else [L, 6, N, N]; else None."""
        if self.case in ("tc2", "rest"):
            return self.global_fields(grid)[0]
        return None

    def initial_state(self, geo: RankGeometry) -> np.ndarray:
        if self.nl == 1:
            return super().initial_state(geo)
        h, wind, b = self.global_fields(geo.grid)
        hl = [geo.gather_global(h[k]) for k in range(self.nl)]
        q = np.empty((4 * self.nl,) + hl[0].shape)
        for k in range(self.nl):
            q[4 * k] = hl[k]
            q[4 * k + 1:4 * k + 4] = np.moveaxis(hl[k][..., None] * geo.gather_global(wind[k]), -1, 0)
        return q

    def kernel_params(self):
        return dict(super().kernel_params(), layers=self.nl, layer_r=self.density_ratio)

    # ---- reference RHS ------------------------------------------------------
    def _layer_flux(self, wL, wR, cL, cR, aL, aR, m, L):
        """The parent's ``_flux`` with the sound speeds aL, aR = sqrt(g H) of the
        two cells passed in."""
        g = self.g
        hL, hR = wL[0], wR[0]
        vL, vR = wL[1:], wR[1:]
        vnL = (vL * m).sum(0)
        vnR = (vR * m).sum(0)
        sL = ((cL[1:] * m).sum(0)).abs() + aL
        sR = ((cR[1:] * m).sum(0)).abs() + aR
        c = torch.maximum(sL, sR)
        Fh = 0.5 * (hL * vnL + hR * vnR) - 0.5 * c * (hR - hL)
        Fm = 0.5 * (hL * vL * vnL + hR * vR * vnR + 0.5 * g * (hL * hL + hR * hR) * m) - 0.5 * c * (hR * vR - hL * vL)
        return torch.cat([Fh[None], Fm], 0) * L

    def coupling_gradient(self, k, hLx, hRx, hLy, hRy, qi, tens):
        """Tangent gradient [3, T, n, n] of c_k = sum_j cw[k][j] h_j: ``hLx`` ..
        the layers' reconstructed depths [L, ...] at the x- and y-edges."""
        cw = self.cw[k]
        cbx = cby = cc = None
        for j in range(self.nl):
            if cw[j] == 0.0:
                continue
            tx, ty, tc = cw[j] * (0.5 * (hLx[j] + hRx[j])), cw[j] * (0.5 * (hLy[j] + hRy[j])), cw[j] * qi[4 * j]
            cbx, cby, cc = (tx, ty, tc) if cbx is None else (cbx + tx, cby + ty, cc + tc)
        if cbx is None:       # one layer: nothing presses or lifts
            return torch.zeros_like(tens["ctr"])
        mx = tens["mx"].permute(1, 0, 2)[:, :, None, :]
        my = tens["my"].permute(1, 0, 2)[:, :, :, None]
        ex, ey = tens["ex"], tens["ey"]
        we, ww = (cbx[..., 1:] - cc) * ex[..., 1:], (cbx[..., :-1] - cc) * ex[..., :-1]
        wn, ws = (cby[..., 1:, :] - cc) * ey[..., 1:, :], (cby[..., :-1, :] - cc) * ey[..., :-1, :]
        gc = ((we * mx[..., 1:] - ww * mx[..., :-1]) + (wn * my[..., 1:, :] - ws * my[..., :-1, :])) * tens["invA"]
        r = tens["ctr"]
        return gc - (gc * r).sum(0) * r

    def _primitives(self, qe):
        """(h_k, v_k) of every layer [4 L, ...], v_k = 0 where h_k = 0."""
        prim = []
        for k in range(self.nl):
            h = qe[4 * k]
            safe = torch.where(h != 0, h, torch.ones_like(h))
            prim.append(torch.stack([h, qe[4 * k + 1] / safe, qe[4 * k + 2] / safe, qe[4 * k + 3] / safe]))
        return prim[0] if self.nl == 1 else torch.cat(prim)

    def coupling_gradients(self, qe, qi, tens, n, g):
        """[L, 3, T, n, n]: grad(c_k) of every layer of the window ``qe`` (the
        arguments of ``rhs``)."""
        (wL, wR, _, _), (yL, yR, _, _) = reconstruct(self._primitives(qe), tens, g, n, self.limiter)
        return torch.stack([self.coupling_gradient(k, wL[0::4], wR[0::4], yL[0::4], yR[0::4], qi, tens)
                            for k in range(self.nl)])

    def rhs(self, qe, qi, tens, n, g):
        L = self.nl
        w = self._primitives(qe)
        (wL, wR, cL, cR), (yL, yR, dL, dR) = reconstruct(w, tens, g, n, self.limiter)
        mx = tens["mx"].permute(1, 0, 2)[:, :, None, :]
        my = tens["my"].permute(1, 0, 2)[:, :, :, None]

        def sound(c):      # sqrt(g H) of the cell averages
            H = c[0]
            for j in range(1, L):
                H = H + c[4 * j]
            return torch.sqrt(self.g * H)
        axL, axR, ayL, ayR = sound(cL), sound(cR), sound(dL), sound(dR)
        invA = tens["invA"]
        r = tens["ctr"]
        f = self.omega * 2.0 * r[2]
        out = []
        for k in range(L):
            s = slice(4 * k, 4 * k + 4)
            Fx = self._layer_flux(wL[s], wR[s], cL[s], cR[s], axL, axR, mx, tens["ex"])
            Gy = self._layer_flux(yL[s], yR[s], dL[s], dR[s], ayL, ayR, my, tens["ey"])
            dq = -((Fx[..., 1:] - Fx[..., :-1]) + (Gy[..., 1:, :] - Gy[..., :-1, :])) * invA
            hc = qi[4 * k]
            M = qi[4 * k + 1:4 * k + 4]
            cor = torch.stack([r[1] * M[2] - r[2] * M[1], r[2] * M[0] - r[0] * M[2], r[0] * M[1] - r[1] * M[0]])
            dq[1:] += -f * cor + (hc * hc) * tens["sbal"] - self.g * hc * tens["gradb"]
            if L > 1:
                dq[1:] -= self.g * hc * self.coupling_gradient(k, wL[0::4], wR[0::4], yL[0::4], yR[0::4], qi, tens)
            out.append(dq)
        return out[0] if L == 1 else torch.cat(out)

    def finalize(self, out, tens):
        r = tens["ctr"]
        for k in range(self.nl):
            M = out[4 * k + 1:4 * k + 4]
            d = (M * r).sum(0)
            out[4 * k + 1:4 * k + 4] = M - d * r
        return out

    def max_dt(self, grid: CubedSphereGrid, cfl: float = 0.9) -> float:
        """The parent's bound with sqrt(g H) and the largest layer wind."""
        if self.nl == 1:
            return super().max_dt(grid, cfl)
        h, wind, b = self.global_fields(grid)
        speed = np.linalg.norm(wind, axis=-1).max(0) + np.sqrt(self.g * np.maximum(h.sum(0), 0))
        return cfl * grid.min_spacing() / (2.0 * float(speed.max()))

    def layer_state(self, q, k: int):
        """(h_k, M_k) of a state [4 L, ...]: a contiguous slice (field-major)."""
        if not 0 <= int(k) < self.nl:
            raise ValueError(f"layer {k}: this physics carries {self.nl} layer(s)")
        return q[4 * int(k):4 * int(k) + 4]

    def derived(self, q, recv, gmap, cmap, tens, tabs, order, T, n, ng, dt, layer: int = 0):
        """The parent's derived fields of layer ``layer``: its rows of the state
        and the receive buffer (PV = (zeta + f) / h_k)."""
        k = int(layer)
        rv = recv[:, 4 * k:4 * k + 4] if recv is not None and recv.numel() else recv
        return super().derived(self.layer_state(q, k), rv, gmap, cmap, tens, tabs, order, T, n, ng, dt)

    def diagnostics(self, qi, tens):
        if self.nl == 1:
            d = super().diagnostics(qi, tens)
            d["mass0"] = d["mass"]
            return d
        A = tens["area"]
        b = tens["b"]
        L = self.nl
        d = {}
        energy = None
        for k in range(L):
            h = qi[4 * k]
            M = qi[4 * k + 1:4 * k + 4]
            below = b
            for j in range(k + 1, L):
                below = below + qi[4 * j]
            e = self.rho[k] * (0.5 * (M * M).sum(0) / h + self.g * h * (below + 0.5 * h))
            energy = e if energy is None else energy + e
            d[f"mass{k}"] = (h * A).sum()
        d["mass"] = sum(d[f"mass{k}"] for k in range(L))
        d["energy"] = (energy * A).sum()
        return d
