"""Thermal diffusion on the sphere (PDF s.12 / s.17: "Lima Flag Temperature
Diffusion", checkerboard heat source on the top panel, day 0.4 -> day 26.7).

    dT/dt = div(kappa grad T)

Two-point flux  F = -kappa (T_R - T_L) L / d  across every edge, with d the
great-circle distance between the true cell centres on both sides (across
panel edges too), so the scheme is exactly conservative and symmetric.
Needs a one-cell halo (the reference's (N+2)^2 layout, PY:141).

The two-point flux is not consistent on the equiangular grid (the line between
two centres is not normal to their edge): on a harmonic the heat equation's
error does not fall under refinement.  ``ConsistentDiffusion`` (``physics.operator:
consistent``) integrates dT/dt = kappa L T with the consistent Laplacian L of
``models/dissipation.py`` instead: conservative, second order, not monotone.  It
needs two passes per stage with an exchange between them, so it does not go
through ``Physics.rhs``: ``ops/heat.py`` drives it, and ``heat_gradient_pass``,
``heat_flux_pass`` and ``heat_stage`` here are the PyTorch twin of
``ops/csrc/heat_kernel.hip``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from .base import Physics, RankGeometry, extend
from .geometry import CubedSphereGrid
from . import dissipation as md
from . import initial_conditions as ic

OPERATORS = ("two_point", "consistent")
HEAT_ROWS = 4            # scratch rows of the consistent operator: T, Gx, Gy, Gz


class Diffusion(Physics):
    name = "diffusion"
    kernel_id = 1
    fields = ["T"]
    halo = 1

    def __init__(self, kappa: float = 2.0e6, case: str = "lima_flag", squares: int = 8):
        self.kappa = kappa
        self.case = case
        self.squares = squares

    def initial_global(self, grid: CubedSphereGrid):
        if self.case == "lima_flag":
            return ic.lima_flag(grid.N, self.squares)
        if self.case == "gaussian":
            return ic.gaussian_hill(grid.centers())
        if self.case in ic.HARMONICS:
            return ic.harmonic_decay(self.case, grid.centers(), 0.0, self.kappa, grid.radius)
        raise ValueError(self.case)

    def exact(self, grid: CubedSphereGrid, t: float):
        """The decayed harmonic of the cases ``harmonic`` (l = 4, zonal) and
        ``harmonic32`` (l = 3, m = 2); None for cases without a closed form."""
        if self.case not in ic.HARMONICS:
            return None
        return ic.harmonic_decay(self.case, grid.centers(), t, self.kappa, grid.radius)

    def initial_state(self, geo: RankGeometry) -> np.ndarray:
        return geo.gather_global(self.initial_global(geo.grid))[None]

    def setup(self, geo: RankGeometry, dtype, device) -> Dict[str, torch.Tensor]:
        dx, dy = geo.center_distances()
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)
        self._coef = (self.kappa * geo.lx / dx, self.kappa * geo.ly / dy, geo.area)
        return {"area": t(geo.area), "invA": t(1.0 / geo.area),
                "ex": t(self.kappa * geo.lx / dx), "ey": t(self.kappa * geo.ly / dy)}

    def rhs(self, qe, qi, tens, n, g):
        c = qe[..., g:g + n, g - 1:g + n + 1]
        Fx = -tens["ex"] * (c[..., 1:] - c[..., :-1])
        c = qe[..., g - 1:g + n + 1, g:g + n]
        Gy = -tens["ey"] * (c[..., 1:, :] - c[..., :-1, :])
        return -((Fx[..., 1:] - Fx[..., :-1]) + (Gy[..., 1:, :] - Gy[..., :-1, :])) * tens["invA"]

    def max_dt(self, grid: CubedSphereGrid, cfl: float = 0.8) -> float:
        # forward-Euler bound dt * sum_e(kappa L_e / d_e) / A <= 1  ~  dx^2 / (4 kappa)
        return cfl * grid.min_spacing() ** 2 / (4.0 * self.kappa)


class ConsistentDiffusion(Diffusion):
    """dT/dt = kappa L T with the consistent Laplacian of ``models/dissipation.py``
    (least-squares cell gradient, corrected edge flux, divergence).  Two passes
    per stage: the engine steps it through ``ops.heat.ConsistentCompute``."""
    two_pass = True

    def rhs(self, qe, qi, tens, n, g):
        raise NotImplementedError("the consistent operator takes two passes with an exchange between them: "
                                  "ops.heat.ConsistentCompute, not Physics.rhs")

    @staticmethod
    def lam(grid: CubedSphereGrid) -> float:
        """max_i sum_e c_e / A_i over the whole grid (|lambda(L)| <= 2 lam), from
        the global geometry: the same number for any tiling and rank count."""
        from ..parallel.layout import TileLayout
        if getattr(grid, "_heat_lam", None) is None:
            grid._heat_lam = md.dissipation_tables(RankGeometry(grid, TileLayout(grid.N, 1, 1, ng=1), 0))["lam"]
        return grid._heat_lam

    def max_dt(self, grid: CubedSphereGrid, cfl: float = 0.8) -> float:
        # every mode's forward-Euler factor 1 + dt kappa lambda stays in [-1, 1] at cfl = 1
        return cfl / (2.0 * self.kappa * self.lam(grid))


# ---- the twin of ops/csrc/heat_kernel.hip -----------------------------------------------------

def heat_gradient_pass(q: torch.Tensor, recv: Optional[torch.Tensor], gmap: torch.Tensor,
                       tabs: Dict[str, torch.Tensor], T: int, n: int, ng: int, scratch: torch.Tensor) -> None:
    """Pass 1: row 0 of the padded buffer ``q`` [>= 1, S] and its least-squares
    gradient, in float64, into the interior of ``scratch`` [4, S]."""
    w = extend(q[:1], None if recv is None else recv[:, :1], gmap, T, n, 1, ng=ng).to(torch.float64)
    c, G = md.ls_gradient(tabs["W"], w, n)
    P = n + 2 * ng
    sv = scratch.view(HEAT_ROWS, T, P, P)[:, :, ng:ng + n, ng:ng + n]
    sv[0] = c[0]
    for k in range(3):
        sv[1 + k] = G[k][0]


def heat_flux_pass(scratch: torch.Tensor, srecv: Optional[torch.Tensor], gmap: torch.Tensor,
                   tabs: Dict[str, torch.Tensor], T: int, n: int, ng: int) -> torch.Tensor:
    """Pass 2: L T [T, n, n] (float64) from the scratch buffer alone."""
    w = extend(scratch, srecv, gmap, T, n, 1, ng=ng)                              # [4,T,n+2,n+2]
    return md.corrected_divergence(w[0:1], w[None, 1:4], tabs, n)[0]


def heat_stage(L: torch.Tensor, st, dt: float, kappa: float, X: torch.Tensor, Q: torch.Tensor,
               acc_in: Optional[torch.Tensor]) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """The stage combination of ``TorchCompute.stage`` with dq = kappa L, in
    float64 whatever the type of the interior views X, Q, acc_in: (out, acc or
    None), to be rounded once at the store."""
    f = lambda a: a.to(torch.float64)
    dq = kappa * L
    acc = None
    if st.acc_out >= 0:
        acc = st.c1 * f(X) + (st.c2 * dt) * dq
        if acc_in is not None and st.c0 != 0.0:
            acc = acc + st.c0 * f(acc_in)
    out = st.a2 * dt * dq
    if st.a1 != 0.0:
        out = out + st.a1 * f(Q)
    if st.a0 != 0.0:
        out = out + st.a0 * f(X)
    return out, acc
