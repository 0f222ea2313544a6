"""Derived shallow-water fields and invariants: relative vorticity, divergence,
potential vorticity; mass, energy, potential enstrophy, circulation and the
Courant number of the running state.

This module is the PyTorch twin (the oracle) of ``ops/csrc/derived_kernel.hip``;
both follow the same definitions.

* velocity  v = M / h  per cell, Cartesian (h == 0: M itself, as ``rhs``);
* window: one ghost layer, gathered through the ghost map, the carried corner
  ghosts and the receive buffer (``extend(..., g=1, cmap=...)``), never read
  from the padded state's ghost slots; on tile sides that lie on a panel edge
  the layer-0 strip is replaced by the Putman-Lin interpolation along the
  neighbouring panel's grid lines (``panel_edge_tables``, layer 0), the same
  pair as ``reconstruct``.  Without it the midpoint of the two cell centres
  across a panel edge sits up to 0.22 cell widths off the edge midpoint and
  the divergence error at panel-edge cells does not converge;
* edge value  v_e = (v_left + v_right) / 2  on every x- and y-edge;
* relative vorticity  zeta = (1/A) sum v_e . d_e  counter-clockwise, d_e the
  chord between the edge's two vertices times the radius (for a constant
  Cartesian vector the line integral along any path is v . (P1 - P0), so the
  chord is exact); in index terms S + E - N - W with the x-chords running
  south to north and the y-chords west to east;
* divergence  delta = (1/A) sum +- (v_e . m_e) L_e;
* potential vorticity  q = (zeta + f) / h,  f = 2 Omega r_z;
* invariants [8]: mass = sum h A, energy (as ``ShallowWater.diagnostics``),
  potential enstrophy = 1/2 sum q^2 h A, circulation = sum zeta A,
  abs_circulation = sum |zeta| A, max_courant = dt max (|v| + sqrt(g h))
  (1/dx + 1/dy) with dx, dy the means of the cell's two opposite edge lengths
  (the 2-D unsplit bound of ``max_dt`` on the running state), two spare.

Every per-cell expression has a fixed association and the sums run over each
panel's cells in global (j, i) order, panels folded in ascending order, so the
fields and the sums of one rank do not depend on the decomposition bit for bit.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from .base import RankGeometry, _interp, _strip, _strip_ext, extend, interior

FIELDS = ("vorticity", "divergence", "pv")
INVARIANTS = ("mass", "energy", "potential_enstrophy", "circulation", "abs_circulation", "max_courant")
NINV = 8                 # record width: 5 sums, 1 max, 2 spare
_MAX = INVARIANTS.index("max_courant")


def derived_tables(geo: RankGeometry, dtype, device) -> Dict[str, torch.Tensor]:
    """Per-tile tables of the derived fields (built on first use, kept off
    ``Physics.setup``'s dict): chord vectors of the x-edges ``cdx`` [T,3,n,n+1]
    (south to north) and y-edges ``cdy`` [T,3,n+1,n] (west to east) in metres,
    and ``idxy`` [T,n,n] = 1/dx + 1/dy per cell."""
    lay, n = geo.layout, geo.n
    V = geo.grid.vertices()
    R = geo.grid.radius
    cdx = np.empty((geo.T, 3, n, n + 1))
    cdy = np.empty((geo.T, 3, n + 1, n))
    for li, tid in enumerate(geo.plan.tiles):
        f, I0, J0 = lay.tile_origin(tid)
        v = V[f, J0:J0 + n + 1, I0:I0 + n + 1]                      # [n+1, n+1, 3]
        cdx[li] = np.moveaxis((v[1:, :] - v[:-1, :]) * R, -1, 0)
        cdy[li] = np.moveaxis((v[:, 1:] - v[:, :-1]) * R, -1, 0)
    dx = 0.5 * (geo.ly[:, :-1, :] + geo.ly[:, 1:, :])
    dy = 0.5 * (geo.lx[:, :, :-1] + geo.lx[:, :, 1:])
    idxy = 1.0 / dx + 1.0 / dy
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=device)
    return {"cdx": t(cdx), "cdy": t(cdy), "idxy": t(idxy)}


def face_order(geo: RankGeometry, device) -> List[torch.Tensor]:
    """Per panel this rank holds cells of: indices into the rank's flattened
    [T, n, n] cells in the panel's global (j, i) order (the summation order)."""
    lay, n, N = geo.layout, geo.n, geo.layout.N
    gid = np.empty((geo.T, n, n), dtype=np.int64)
    jj, ii = np.mgrid[0:n, 0:n]
    for li, tid in enumerate(geo.plan.tiles):
        f, I0, J0 = lay.tile_origin(tid)
        gid[li] = lay.global_flat(f, I0 + ii, J0 + jj)
    gid = gid.reshape(-1)
    order = np.argsort(gid, kind="stable")
    face = gid[order] // (N * N)
    return [torch.as_tensor(order[face == f], device=device) for f in np.unique(face)]


def window(q: torch.Tensor, recv: Optional[torch.Tensor], gmap: torch.Tensor, cmap: torch.Tensor,
           tens: Dict[str, torch.Tensor], T: int, n: int, ng: int, interp: bool = True) -> torch.Tensor:
    """(h, v) window [4, T, n+2, n+2] of the padded state q [4, S]: ghost layer
    0 pulled through the maps, panel-edge strips interpolated (``interp``)."""
    w = extend(q, recv, gmap, T, n, 1, ng=ng, cmap=cmap)
    h = w[0]
    safe = torch.where(h != 0, h, torch.ones_like(h))
    w = torch.stack([h, w[1] / safe, w[2] / safe, w[3] / safe])
    pe = tens.get("pedge")
    if not interp or pe is None or "pe_base" not in tens:
        return w
    wi = w.clone()
    for side in range(4):
        m = ((pe >> side) & 1) != 0
        if not bool(m.any()):
            continue
        x = _strip(w, side, 0, 1, n)
        xi = _interp(_strip_ext(w, side, 0, 1, n), tens["pe_base"][:, side, 0] + 1, tens["pe_t"][:, side, 0])
        _strip(wi, side, 0, 1, n).copy_(torch.where(m[:, None], xi, x))
    return wi


def _dot(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def fields_from_window(w: torch.Tensor, tens: Dict[str, torch.Tensor], tabs: Dict[str, torch.Tensor], n: int,
                       omega2: float) -> torch.Tensor:
    """[3, T, n, n] (zeta, delta, q) from the (h, v) window."""
    v = w[1:4]
    ve_x = 0.5 * (v[:, :, 1:n + 1, 0:n + 1] + v[:, :, 1:n + 1, 1:n + 2])      # [3,T,n,n+1]
    ve_y = 0.5 * (v[:, :, 0:n + 1, 1:n + 1] + v[:, :, 1:n + 2, 1:n + 1])      # [3,T,n+1,n]
    cx = _dot(ve_x, tabs["cdx"].movedim(1, 0))                               # [T,n,n+1]
    cy = _dot(ve_y, tabs["cdy"].movedim(1, 0))                               # [T,n+1,n]
    invA = tens["invA"]
    zeta = (((cy[:, :-1, :] + cx[:, :, 1:]) - cy[:, 1:, :]) - cx[:, :, :-1]) * invA
    mx = tens["mx"].permute(1, 0, 2)[:, :, None, :]                           # [3,T,1,n+1]
    my = tens["my"].permute(1, 0, 2)[:, :, :, None]                           # [3,T,n+1,1]
    fx = _dot(ve_x, mx) * tens["ex"]
    fy = _dot(ve_y, my) * tens["ey"]
    delta = ((fx[:, :, 1:] - fx[:, :, :-1]) + (fy[:, 1:, :] - fy[:, :-1, :])) * invA
    h = w[0, :, 1:n + 1, 1:n + 1]
    pv = (zeta + omega2 * tens["ctr"][2]) / h
    return torch.stack([zeta, delta, pv])


def invariant_terms(qi: torch.Tensor, w: torch.Tensor, fields: torch.Tensor, tens: Dict[str, torch.Tensor],
                    tabs: Dict[str, torch.Tensor], n: int, g: float):
    """Per-cell float64 terms of the five sums [5, T, n, n] and of the Courant
    maximum [T, n, n] (qi: interior state [4, T, n, n])."""
    h, v = qi[0], w[1:4, :, 1:n + 1, 1:n + 1]
    zeta, pv = fields[0], fields[2]
    d = lambda a: a.to(torch.float64)
    A = d(tens["area"])
    v2 = _dot(v, v)
    M = d(qi[1:4])
    ke = 0.5 * _dot(M, M) / d(h)
    pe = 0.5 * g * d(h) * d(h) + g * d(h) * d(tens["b"])
    terms = torch.stack([d(h) * A, (ke + pe) * A, 0.5 * d(pv) * d(pv) * d(h) * A, d(zeta) * A, d(zeta).abs() * A])
    cour = d((torch.sqrt(v2) + torch.sqrt(g * h)) * tabs["idxy"])
    return terms, cour


def fold(terms: torch.Tensor, cour: torch.Tensor, order: List[torch.Tensor], dt: float) -> torch.Tensor:
    """[8] float64: each panel's cells summed in global order, the panels
    folded in ascending order."""
    flat = terms.reshape(terms.shape[0], -1)
    out = torch.zeros(NINV, dtype=torch.float64, device=terms.device)
    acc = None
    for idx in order:
        s = torch.stack([flat[k][idx].contiguous().sum() for k in range(flat.shape[0])])
        acc = s if acc is None else acc + s
    if acc is not None:
        out[:flat.shape[0]] = acc
    out[_MAX] = dt * cour.max() if cour.numel() else 0.0
    return out


def derived_twin(q: torch.Tensor, recv: Optional[torch.Tensor], gmap: torch.Tensor, cmap: torch.Tensor,
                 tens: Dict[str, torch.Tensor], tabs: Dict[str, torch.Tensor], order: List[torch.Tensor],
                 T: int, n: int, ng: int, g: float, omega2: float, dt: float, interp: bool = True):
    """(fields [3, T, n, n], inv [8] float64) of the padded state q [4, S]."""
    w = window(q, recv, gmap, cmap, tens, T, n, ng, interp=interp)
    fields = fields_from_window(w, tens, tabs, n, omega2)
    terms, cour = invariant_terms(interior(q, T, n, ng), w, fields, tens, tabs, n, g)
    return fields, fold(terms, cour, order, dt)
