"""Point sampling and Lagrangian particles: definitions and the twin (numpy
location, PyTorch arithmetic) of ``ops/csrc/points_kernel.hip``.

Points are unit vectors ``p[K, 3]``, float64 whatever the state's type.  A point
is located on the dual mesh of the cell centres by ``models.latlon.locate_points``
(panel, snapping, tie rules, candidates as for the lat-lon tables): four source
cells (global ids) and four float64 weights.  The dual mesh reads no ghost cell.

Sampling (``sample_terms`` / ``sample``, ``velocity_terms`` / ``velocity``).  With
x_s the value of a channel at source slot s converted to float64,

    scalar      t_s = w_s * x_s
    velocity    t_s,c = w_s * (M_c,s / d_s),  d_s = h_s if h_s != 0 else 1,  c = 0, 1, 2
    a slot the rank does not own (index -1) reads nothing:  t_s = 0
    value       ((t_0 + t_1) + t_2) + t_3

so sampling a float32 state differs from sampling its float64 copy only through
the loads.  Several ranks exchange the terms [C, 4, K]; one rank owns each term,
the arrays add exactly, and the fold of the sum is the one-rank expression.

Particles: Heun's scheme in the tangent plane, step ``dtp = interval * dt``,
sphere radius R.  With dot(a, b) = (a_0 b_0 + a_1 b_1) + a_2 b_2:

    tangent(v, x) = v - dot(v, x) * x                     (per component)
    V(x)          = tangent(folded velocity at x, x)
    move(x, d):     e = tangent(d, x);  n = sqrt(dot(e, e))
                    n == 0:  x' = x
                    else     theta = n / R;  y = cos(theta) * x + sin(theta) * (e / n)
                             x' = y / sqrt(dot(y, y))

    start:          v0 = V(x);                    xs = move(x, dtp * v0)         (predictor)
    advance, once the model has reached the next particle time:
                    v1 = V(xs)                    on the new state
                    x  = move(x, (0.5 * dtp) * (v0 + v1))                        (corrector)
                    v0 = V(x)                     on the same state
                    xs = move(x, dtp * v0)                                       (predictor)

An advance reads the current state only.  A position that is not finite is
"lost": it reads nothing, stays NaN, and so does everything sampled there.
``ParticleState`` holds x, xs, v0 ([K, 3] float64 each).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ..parallel.layout import TileLayout
from . import latlon as ml
from .geometry import CubedSphereGrid


def lonlat_points(lat, lon) -> np.ndarray:
    """Unit vectors [K, 3] of lat / lon [K] in radians."""
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    lon = np.asarray(lon, dtype=np.float64).reshape(-1)
    if lat.shape != lon.shape:
        raise ValueError(f"points: lat [{lat.size}] and lon [{lon.size}] differ in length")
    with np.errstate(invalid="ignore"):       # a non-finite angle gives a non-finite point: the callers reject it
        cl = np.cos(lat)
        return np.stack([cl * np.cos(lon), cl * np.sin(lon), np.sin(lat)], 1)


def points_lonlat(p) -> Tuple[np.ndarray, np.ndarray]:
    """(lat, lon) [K] in radians of unit vectors [K, 3]; lon in [0, 2 pi)."""
    p = np.asarray(p, dtype=np.float64)
    lat = np.arcsin(np.clip(p[:, 2], -1.0, 1.0))
    lon = np.mod(np.arctan2(p[:, 1], p[:, 0]), 2.0 * np.pi)
    return np.where(np.isfinite(p).all(1), lat, np.nan), np.where(np.isfinite(p).all(1), lon, np.nan)


def random_points(K: int, seed: int = 0) -> np.ndarray:
    """K points uniform on the sphere (normalised Gaussian triples)."""
    g = np.random.default_rng(seed).standard_normal((int(K), 3))
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def check_seeds(p) -> np.ndarray:
    """Seeds [K, 3]: finite and non-zero (``ValueError`` otherwise), normalised."""
    p = np.array(p, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3 or p.shape[0] < 1:
        raise ValueError(f"particles: seeds [K, 3] with K >= 1 expected, not {p.shape}")
    nrm = np.linalg.norm(p, axis=1, keepdims=True)
    if not np.isfinite(p).all() or not (nrm > 0).all():
        raise ValueError("particles: seeds must be finite, non-zero vectors")
    return p / nrm


# ----------------------------------------------------------------------------
# tables
# ----------------------------------------------------------------------------

class PointTables:
    """What the kernel reads besides the state, for C<N> (no table of O(N^2)
    doubles): ``eid`` [6, 4, N-1], ``bcell`` [12 (N-1) + 8, 4] cells of the border
    elements (edge quads, then corner triangles with -1 in the fourth slot),
    ``ctri`` [6, 4], all int32, and ``bctr`` [12 (N-1) + 8, 4, 3] float64, the
    centres of those cells laid out beside ``bcell`` (a triangle's fourth row
    repeats its first)."""

    def __init__(self, N: int):
        self.N = int(N)
        m = self.mesh = ml.DualMesh(self.N)
        self.nq = len(m.equad)
        cells = m.element_cells()[m.nint:]
        ctr = CubedSphereGrid(self.N).centers().reshape(-1, 3)
        self.eid = np.ascontiguousarray(m.eid, dtype=np.int32)
        self.bcell = np.ascontiguousarray(cells, dtype=np.int32)
        self.ctri = np.ascontiguousarray(m.ctri, dtype=np.int32)
        self.bctr = np.ascontiguousarray(ctr[np.where(cells >= 0, cells, cells[:, :1])])
        self.ncell = 6 * self.N * self.N


def rank_maps(layout: TileLayout, rank: int) -> Tuple[np.ndarray, np.ndarray]:
    """The rank's cell maps (``TileLayout.cell_maps``)."""
    return layout.cell_maps(rank)


@dataclass
class Located:
    """Location of K points for one source layout: ``idx`` [K, 4] int64 index
    inside a channel (-1: skipped), ``w`` [K, 4] float64 (NaN for a lost point),
    ``elem`` / ``margin`` [K] (numpy; -1 / NaN for a lost point)."""
    idx: torch.Tensor
    w: torch.Tensor
    elem: np.ndarray
    margin: np.ndarray


def locate(N: int, p, cmap: Optional[np.ndarray] = None, mesh: Optional[ml.DualMesh] = None,
           device="cpu") -> Located:
    """Locate p [K, 3] (tensor or array); ``cmap``: the rank's map from
    ``rank_maps`` (default: global cell ids, for a source [..., 6 N N])."""
    pn = p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)
    pn = np.ascontiguousarray(pn, dtype=np.float64).reshape(-1, 3)
    K = len(pn)
    ok = np.isfinite(pn).all(1)
    src = np.zeros((K, 4), dtype=np.int64)
    w = np.full((K, 4), np.nan)
    elem = np.full(K, -1, dtype=np.int64)
    margin = np.full(K, np.nan)
    if ok.any():
        src[ok], w[ok], elem[ok], margin[ok] = ml.locate_points(N, pn[ok], mesh)
    idx = src if cmap is None else cmap[src].astype(np.int64)
    idx = np.where(ok[:, None], idx, -1)
    return Located(torch.as_tensor(idx, device=device), torch.as_tensor(w, device=device), elem, margin)


# ----------------------------------------------------------------------------
# sampling
# ----------------------------------------------------------------------------

fold_terms = ml.fold_terms      # [C, 4, K] -> [C, K]: ((t0 + t1) + t2) + t3


def _lost(loc: Located) -> torch.Tensor:
    return torch.isnan(loc.w[:, 0])


def sample_terms(fields: torch.Tensor, loc: Located) -> torch.Tensor:
    """[C, 4, K] float64 terms of the scalar channels ``fields`` [C, ...]
    (flattened per channel to the layout ``loc.idx`` indexes); 0 for a skipped
    slot, NaN for a lost point."""
    x = fields.reshape(fields.shape[0], -1)
    m = loc.idx >= 0
    i = torch.where(m, loc.idx, torch.zeros_like(loc.idx))
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=x.device)
    lost = _lost(loc)
    t = [torch.where(lost, nan, torch.where(m[:, s], loc.w[:, s] * x[:, i[:, s]].to(torch.float64), zero))
         for s in range(4)]
    return torch.stack(t, 1)


def sample(fields: torch.Tensor, loc: Located) -> torch.Tensor:
    """[C, K] float64 of the scalar channels ``fields`` at the points."""
    return fold_terms(sample_terms(fields, loc))


def velocity_terms(q: torch.Tensor, loc: Located) -> torch.Tensor:
    """[3, 4, K] float64 terms of the Cartesian velocity of the shallow-water
    state ``q`` [4, ...] (h, M): v = M / h per source cell (h == 0: M itself)."""
    q = q.reshape(4, -1)
    m = loc.idx >= 0
    i = torch.where(m, loc.idx, torch.zeros_like(loc.idx))
    zero = torch.zeros((), dtype=torch.float64, device=q.device)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=q.device)
    lost = _lost(loc)
    t = []
    for s in range(4):
        hs = q[0, i[:, s]].to(torch.float64)
        d = torch.where(hs != 0, hs, torch.ones_like(hs))
        v = loc.w[:, s] * (q[1:4, i[:, s]].to(torch.float64) / d)
        t.append(torch.where(lost, nan, torch.where(m[:, s], v, zero)))
    return torch.stack(t, 1)


def velocity(q: torch.Tensor, loc: Located) -> torch.Tensor:
    """[3, K] float64 Cartesian velocity at the points."""
    return fold_terms(velocity_terms(q, loc))


# ----------------------------------------------------------------------------
# particles
# ----------------------------------------------------------------------------

def _dot(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def tangent(v: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """[K, 3]: v - dot(v, x) x."""
    return v - _dot(v, x)[:, None] * x


def move(x: torch.Tensor, d: torch.Tensor, radius: float) -> torch.Tensor:
    """[K, 3]: x carried along the great circle of the tangent part of d (m)."""
    e = tangent(d, x)
    n = torch.sqrt(_dot(e, e))
    still = n == 0
    n1 = torch.where(still, torch.ones_like(n), n)
    th = n1 / radius
    y = torch.cos(th)[:, None] * x + torch.sin(th)[:, None] * (e / n1[:, None])
    y = y / torch.sqrt(_dot(y, y))[:, None]
    return torch.where(still[:, None], x, y)


@dataclass
class ParticleState:
    x: torch.Tensor       # [K, 3] positions
    xs: torch.Tensor      # [K, 3] predicted positions at the next particle time
    v0: torch.Tensor      # [K, 3] V(x)


def corrector(st: ParticleState, vel: torch.Tensor, dtp: float, radius: float) -> None:
    """x <- move(x, dtp/2 (v0 + v1)) with v1 the tangent part at xs of the
    folded velocity ``vel`` [3, K] (or terms [3, 4, K]) sampled at xs."""
    v = (fold_terms(vel) if vel.dim() == 3 else vel).T
    v1 = tangent(v, st.xs)
    st.x = move(st.x, (0.5 * dtp) * (st.v0 + v1), radius)


def predictor(st: ParticleState, vel: torch.Tensor, dtp: float, radius: float) -> None:
    """v0 <- V(x) from the velocity sampled at x; xs <- move(x, dtp v0)."""
    v = (fold_terms(vel) if vel.dim() == 3 else vel).T
    st.v0 = tangent(v, st.x)
    st.xs = move(st.x, dtp * st.v0, radius)


class TwinParticles:
    """Particles on a global state [4, 6, N, N] (h, M), one rank: the reference
    the tests advance.  ``margins`` collects the margin of every point that was
    located (predictor and corrector points alike)."""

    def __init__(self, N: int, p, dtp: float, radius: float):
        self.N, self.dtp, self.radius = int(N), float(dtp), float(radius)
        self.mesh = ml.DualMesh(self.N)
        x = torch.as_tensor(check_seeds(p))
        self.st = ParticleState(x, x.clone(), torch.zeros_like(x))
        self.margins = []

    def _velocity(self, q: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
        loc = locate(self.N, p, mesh=self.mesh)
        self.margins.append(loc.margin)
        return velocity(q, loc)

    def start(self, q: torch.Tensor) -> None:
        predictor(self.st, self._velocity(q, self.st.x), self.dtp, self.radius)

    def advance(self, q: torch.Tensor) -> None:
        corrector(self.st, self._velocity(q, self.st.xs), self.dtp, self.radius)
        predictor(self.st, self._velocity(q, self.st.x), self.dtp, self.radius)
