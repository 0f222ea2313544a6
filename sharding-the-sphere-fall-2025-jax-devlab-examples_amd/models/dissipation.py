"""Scale-selective dissipation of the shallow-water state: a consistent
Laplacian on the cubed sphere, applied once (order 1, ``nu lap``) or twice
(order 2, ``-nu lap lap``), by first-order splitting between model steps.

This module is the PyTorch twin (the oracle) of ``ops/csrc/dissipation_kernel.hip``
and holds the host tables both read; ``ops/dissipation.py`` drives either.

The two-point flux of ``models/diffusion.py`` (``kappa L / d`` across each edge)
is symmetric and conservative but not consistent on the equiangular grid: the
line between two cell centres is not normal to their edge, and at a panel edge
it has a kink.  The operator here corrects the flux with a cell gradient.

Pass 1, cell gradient.  For a scalar s, cell i with unit centre c_i and the
four face neighbours k = W, E, S, N (the real cells across each face: raw
ghosts across panel edges, no interpolation, no corner ghost):

    d_k  = tangent part at c_i of  R (c_k - c_i)
    G_i  = sum_k W_ik (s_k - s_i),   W_ik = (sum_k d_k d_k^T + rho c_i c_i^T)^-1 d_k

with rho = R^2 / N^2.  G_i is tangent and exact for linear fields.  It is a
global Cartesian vector: a neighbour's G needs no rotation anywhere.

Pass 2, corrected edge flux.  With the edge's unit normal m, length L, the
chord dvec = R (c_R - c_L) between the two real centres and dn = dvec . m:

    Phi_e   = L [ (s_R - s_L) / dn + 1/2 (G_L + G_R) . (m - dvec / dn) ]
            = c_e (s_R - s_L) + 1/2 (G_L + G_R) . k_e
    (L s)_i = ((Phi_x[i+1] - Phi_x[i]) + (Phi_y[j+1] - Phi_y[j])) / A_i

Both passes run over a scratch buffer [16, S] in the padded layout of the state:
rows 0..3 the four scalars, rows 4 + 3 c + k component k of G of scalar c.  Pass
2 reads nothing else, so the update may overwrite the state in place; a
neighbour is addressed through the ghost map (a same-rank source cell, or a
slot of the scratch's receive buffer), never through a ghost slot.

Shallow water: the scalars are w = (h, vx, vy, vz), v = M / h.  The depth
equation diffuses the free surface eta = h + b: G(eta) = G(h) + G(b) and
eta_R - eta_L = (h_R - h_L) + (b_R - b_L) with the b terms from host tables, so
a lake at rest is a fixed point and no ghost value of b is read.  Order 1:
dw = tau nu L w.  Order 2: dw = -tau nu L (L w), the inner field (L eta, L v)
without b terms in the second application.  Update: h' = h + dh, v' = P (v + dv)
(tangent projection), M' = h' v'.  ``depth`` false leaves h (and every tracer
row) untouched.

All arithmetic is float64 whatever the state's type; every expression has a
fixed association and every cell evaluates its own four fluxes from per-edge
tables that do not depend on the decomposition, so the result is the same bit
for bit for any tiling and any number of ranks.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from .base import RankGeometry, extend

ROWS = 16                # scratch rows: 4 scalars + 4 x 3 gradient components
MAX_SUBSTEPS = 64


def _dot3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def dissipation_tables(geo: RankGeometry, b_global: Optional[np.ndarray] = None) -> Dict[str, np.ndarray]:
    """Host tables of one rank, float64 numpy, elementwise from the global grid
    (the same numbers for any tiling):

    ``W`` [T, n, n, 4, 3] least-squares weights; ``cx`` [T, n, n+1], ``cy``
    [T, n+1, n] = L / dn; ``kx`` [T, n, n+1, 3], ``ky`` [T, n+1, n, 3] =
    L (m - dvec / dn); ``invA`` [T, n, n]; ``ctr`` [T, n, n, 3]; with a
    topography ``gb`` [T, n, n, 3] = G(b), ``dbx`` / ``dby`` = b_R - b_L per
    edge (zero without one); ``lam`` = max_i sum_e c_e / A_i of this rank."""
    n, R, N = geo.n, geo.grid.radius, geo.layout.N
    ce = geo.neighbor_values(geo.grid.centers())                    # [T,n+2,n+2,3], corners unused
    c = ce[:, 1:n + 1, 1:n + 1]
    nbr = (ce[:, 1:n + 1, 0:n], ce[:, 1:n + 1, 2:n + 2], ce[:, 0:n, 1:n + 1], ce[:, 2:n + 2, 1:n + 1])
    d = []
    for ck in nbr:
        e = (ck - c) * R
        d.append(e - _dot3(e, c)[..., None] * c)
    rho = R * R / (N * N)

    def mom(i, j):
        s = rho * c[..., i] * c[..., j]
        for dk in d:
            s = s + dk[..., i] * dk[..., j]
        return s
    a, b_, c_, e_, f_, i_ = mom(0, 0), mom(0, 1), mom(0, 2), mom(1, 1), mom(1, 2), mom(2, 2)
    # inverse of the symmetric matrix [[a, b, c], [b, e, f], [c, f, i]] by cofactors
    A00, A01, A02 = e_ * i_ - f_ * f_, c_ * f_ - b_ * i_, b_ * f_ - c_ * e_
    A11, A12, A22 = a * i_ - c_ * c_, b_ * c_ - a * f_, a * e_ - b_ * b_
    det = (a * A00 + b_ * A01) + c_ * A02
    W = np.empty(c.shape[:-1] + (4, 3))
    for k, dk in enumerate(d):
        W[..., k, 0] = ((A00 * dk[..., 0] + A01 * dk[..., 1]) + A02 * dk[..., 2]) / det
        W[..., k, 1] = ((A01 * dk[..., 0] + A11 * dk[..., 1]) + A12 * dk[..., 2]) / det
        W[..., k, 2] = ((A02 * dk[..., 0] + A12 * dk[..., 1]) + A22 * dk[..., 2]) / det

    def edge(cl, cr, m, L):
        dv = (cr - cl) * R
        m = np.broadcast_to(m, dv.shape)
        dn = _dot3(dv, m)
        return L / dn, L[..., None] * (m - dv / dn[..., None])
    cx, kx = edge(ce[:, 1:n + 1, 0:n + 1], ce[:, 1:n + 1, 1:n + 2], geo.mx[:, None, :, :], geo.lx)
    cy, ky = edge(ce[:, 0:n + 1, 1:n + 1], ce[:, 1:n + 2, 1:n + 1], geo.my[:, :, None, :], geo.ly)
    out = {"W": W, "cx": cx, "cy": cy, "kx": kx, "ky": ky, "invA": 1.0 / geo.area, "ctr": geo.center.copy()}
    gb = np.zeros(c.shape)
    dbx, dby = np.zeros(cx.shape), np.zeros(cy.shape)
    if b_global is not None and np.any(b_global != 0):
        be = geo.neighbor_values(b_global)                         # [T,n+2,n+2]
        bc = be[:, 1:n + 1, 1:n + 1]
        db = (be[:, 1:n + 1, 0:n] - bc, be[:, 1:n + 1, 2:n + 2] - bc, be[:, 0:n, 1:n + 1] - bc,
              be[:, 2:n + 2, 1:n + 1] - bc)
        for k in range(3):
            gb[..., k] = ((W[..., 0, k] * db[0] + W[..., 1, k] * db[1]) + W[..., 2, k] * db[2]) + W[..., 3, k] * db[3]
        dbx = be[:, 1:n + 1, 1:n + 2] - be[:, 1:n + 1, 0:n + 1]
        dby = be[:, 1:n + 2, 1:n + 1] - be[:, 0:n + 1, 1:n + 1]
    out.update(gb=gb, dbx=dbx, dby=dby)
    csum = ((cx[:, :, :-1] + cx[:, :, 1:]) + cy[:, :-1, :]) + cy[:, 1:, :]
    out["lam"] = float((csum / geo.area).max()) if csum.size else 0.0
    return out


def device_tables(tabs: Dict[str, np.ndarray], device) -> Dict[str, torch.Tensor]:
    """The tables as contiguous float64 tensors, vectors component-major (one
    plane per component, so a wave reads each plane with unit stride): ``W``
    [4, 3, T, n, n], ``kx`` [3, T, n, n+1], ``ky`` [3, T, n+1, n], ``gb`` and
    ``ctr`` [3, T, n, n]; the scalars as they are."""
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)
    return {"W": t(np.transpose(tabs["W"], (3, 4, 0, 1, 2))),
            "kx": t(np.moveaxis(tabs["kx"], -1, 0)), "ky": t(np.moveaxis(tabs["ky"], -1, 0)),
            "gb": t(np.moveaxis(tabs["gb"], -1, 0)), "ctr": t(np.moveaxis(tabs["ctr"], -1, 0)),
            "cx": t(tabs["cx"]), "cy": t(tabs["cy"]), "dbx": t(tabs["dbx"]), "dby": t(tabs["dby"]),
            "invA": t(tabs["invA"])}


def substeps(tau: float, nu: float, lam: float, order: int) -> int:
    """The smallest m with (tau / m) nu lam <= 1/2 (order 1) or (tau / m) nu
    (2 lam)^2 <= 1 (order 2): with |lambda| <= 2 lam measured for L, every mode's
    Euler factor then stays in [0, 1].  More than ``MAX_SUBSTEPS`` raises."""
    rate = 2.0 * nu * lam if order == 1 else nu * (2.0 * lam) ** 2
    m = max(1, int(math.ceil(tau * rate * (1.0 - 1e-12))))
    if m > MAX_SUBSTEPS:
        nu_max = MAX_SUBSTEPS / (tau * rate / nu)
        raise ValueError(f"dissipation: tau = {tau:g} s with nu = {nu:g} needs {m} sub-steps, more than "
                         f"{MAX_SUBSTEPS}; the largest admissible nu is {nu_max:.6g}")
    return m


# ---- the twin: pass 1, pass 2, update ---------------------------------------------------------

def primitives(q: torch.Tensor) -> torch.Tensor:
    """(h, M / h) in float64 of (h, M) [4, ...] (h == 0: M itself)."""
    q = q.to(torch.float64)
    h = q[0]
    safe = torch.where(h != 0, h, torch.ones_like(h))
    return torch.stack([h, q[1] / safe, q[2] / safe, q[3] / safe])


def ls_gradient(W: torch.Tensor, w: torch.Tensor, n: int):
    """The shared arithmetic of pass 1: of the one-ring window w [C, T, n+2, n+2]
    (corners unused) the interior values c [C, T, n, n] and the three Cartesian
    components of G = sum_k W_k (w_k - w_i), each [C, T, n, n]."""
    c = w[:, :, 1:n + 1, 1:n + 1]
    d = (w[:, :, 1:n + 1, 0:n] - c, w[:, :, 1:n + 1, 2:n + 2] - c, w[:, :, 0:n, 1:n + 1] - c,
         w[:, :, 2:n + 2, 1:n + 1] - c)
    return c, [((W[0, k] * d[0] + W[1, k] * d[1]) + W[2, k] * d[2]) + W[3, k] * d[3] for k in range(3)]


def corrected_divergence(s: torch.Tensor, G: torch.Tensor, tabs: Dict[str, torch.Tensor], n: int,
                         db=None) -> torch.Tensor:
    """The shared arithmetic of pass 2: L s [C, T, n, n] of the one-ring windows
    s [C, T, n+2, n+2] and G [C, 3, T, n+2, n+2] (corners unused); ``db`` =
    (dbx, dby): the topography differences added to scalar 0."""
    kx, ky = tabs["kx"], tabs["ky"]
    dx = s[:, :, 1:n + 1, 1:n + 2] - s[:, :, 1:n + 1, 0:n + 1]                    # [C,T,n,n+1]
    dy = s[:, :, 1:n + 2, 1:n + 1] - s[:, :, 0:n + 1, 1:n + 1]
    if db is not None:
        dx = torch.cat([(dx[0] + db[0])[None], dx[1:]])
        dy = torch.cat([(dy[0] + db[1])[None], dy[1:]])
    gx = G[:, :, :, 1:n + 1, 0:n + 1] + G[:, :, :, 1:n + 1, 1:n + 2]            # [C,3,T,n,n+1]
    gy = G[:, :, :, 0:n + 1, 1:n + 1] + G[:, :, :, 1:n + 2, 1:n + 1]
    px = tabs["cx"] * dx + 0.5 * ((gx[:, 0] * kx[0] + gx[:, 1] * kx[1]) + gx[:, 2] * kx[2])
    py = tabs["cy"] * dy + 0.5 * ((gy[:, 0] * ky[0] + gy[:, 1] * ky[1]) + gy[:, 2] * ky[2])
    return ((px[..., 1:] - px[..., :-1]) + (py[..., 1:, :] - py[..., :-1, :])) * tabs["invA"]


def gradient_pass(src: torch.Tensor, recv: Optional[torch.Tensor], gmap: torch.Tensor, tabs: Dict[str, torch.Tensor],
                  T: int, n: int, ng: int, swe: bool, use_b: bool, scratch: torch.Tensor) -> None:
    """Pass 1: the four scalars of the padded buffer ``src`` [>= 4, S] (``swe``:
    a state (h, M), read as (h, M / h); else the rows as they are) and their
    gradients into the interior of ``scratch`` [16, S]."""
    w = extend(src[:4], None if recv is None else recv[:, :4], gmap, T, n, 1, ng=ng).to(torch.float64)
    if swe:
        w = primitives(w)
    c, G = ls_gradient(tabs["W"], w, n)
    P = n + 2 * ng
    sv = scratch.view(ROWS, T, P, P)[:, :, ng:ng + n, ng:ng + n]
    sv[0:4] = c
    for k in range(3):
        g = G[k]                                                                       # [4,T,n,n]
        if use_b:
            g = torch.cat([(g[0] + tabs["gb"][k])[None], g[1:]])
        for s in range(4):
            sv[4 + 3 * s + k] = g[s]


def flux_pass(scratch: torch.Tensor, srecv: Optional[torch.Tensor], gmap: torch.Tensor,
              tabs: Dict[str, torch.Tensor], T: int, n: int, ng: int, use_b: bool) -> torch.Tensor:
    """Pass 2: L of the four scalars [4, T, n, n] from the scratch buffer."""
    w = extend(scratch, srecv, gmap, T, n, 1, ng=ng)                            # [16,T,n+2,n+2]
    return corrected_divergence(w[0:4], w[4:].reshape(4, 3, T, n + 2, n + 2), tabs, n,
                                (tabs["dbx"], tabs["dby"]) if use_b else None)


def update(q: torch.Tensor, Lw: torch.Tensor, coef: float, tabs: Dict[str, torch.Tensor], depth: bool) -> None:
    """h' = h + coef L_0 (``depth``), v' = P (v + coef L_1..3), M' = h' v' on the
    interior view q [F >= 4, T, n, n] of the state, in place, rounded once to its
    type; rows beyond the fourth (and h without ``depth``) are not written."""
    w = primitives(q[:4])
    h = w[0] + coef * Lw[0] if depth else w[0]
    u = w[1:4] + coef * Lw[1:4]
    r = tabs["ctr"]
    dd = (u[0] * r[0] + u[1] * r[1]) + u[2] * r[2]
    v = u - dd * r
    if depth:
        q[0] = h.to(q.dtype)
    q[1:4] = (h * v).to(q.dtype)
