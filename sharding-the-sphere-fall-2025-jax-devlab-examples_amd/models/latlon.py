"""Longitude-latitude regridding of cubed-sphere fields: host tables and the
PyTorch twin (the oracle) of ``ops/csrc/latlon_kernel.hip``.

Target grid: a rectilinear grid of 1-D ``lat[nlat]``, ``lon[nlon]`` in radians
(``default_grid``: cell-centred; any ascending arrays are allowed, a latitude
band and the rows lat = +-pi/2 included), K = nlat nlon points, k = j nlon + i.

Interpolation mesh: the dual mesh of the cell centres.  It tiles the sphere with

    6 (N-1)^2   interior quads   four neighbouring centres of one panel
    12 (N-1)    edge quads       two border cells of each of two panels (cells
                                 match one to one along a cube edge; the partner
                                 of a border cell is its layer-0 ghost source,
                                 ``TileLayout.ghost_sources``)
    8           corner triangles the three corner cells that meet at a cube corner

numbered in that order (the element id; ties between elements that share a
boundary go to the lowest id).  Lines of constant alpha or beta are great
circles, so every side of every element is a great-circle arc, and the border
between a panel's interior quads and its edge quads is the grid line through
the border centres exactly.

Weights:
* interior quad: bilinear in the panel's equiangular (alpha, beta), where the
  centres are uniform;
* edge quad: the inverse of the bilinear map of the quad in the gnomonic plane
  tangent at the target point (great circles are straight lines there), by
  Newton from (1/2, 1/2);
* corner triangle: barycentric in the same plane, fourth slot weight 0.
A point beyond the border centres of its panel (within half a cell of the
panel border) lies in an edge quad or a corner triangle; since the cross sides
of the edge quads do not follow the panel's grid lines, the neighbouring
candidates are tested and the lowest id that contains the point is taken.
Only elements on the point's own side of the sphere are considered (an
antipodal element projects to a false hit).

``LatLonTables``: ``src[K, 4]`` global cell ids, ``w[K, 4]`` fp64 weights,
``east[K, 3]`` / ``north[K, 3]`` unit vectors from lat / lon (at a pole: the
formula's limit for that lon).  ``rank_index`` derives, per rank, the indices
of the sources in the padded state [F, T P P] and in the unpadded [C, T, n, n]
layout; a source the rank does not own is -1.  Sources are real cells, never
ghost slots.

Twin: ``regrid`` (scalar channels), ``velocity`` (v = M / h per source cell,
three Cartesian components), ``project`` (onto east / north), ``winds`` and
``zonal_mean``.  Every sum has the fixed association ((t0 + t1) + t2) + t3 with
t = w x (0 for a slot of index -1), so the one-rank result is a defined
expression and does not depend on the decomposition bit for bit.  Several
ranks exchange the terms themselves (``regrid_terms``, ``velocity_terms``): each
term is owned by one rank, the ranks' arrays add exactly, and ``fold_terms`` on
the sum is the one-rank expression again.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ..parallel.layout import TileLayout
from ..parallel.topology import FACE_FRAMES
from .geometry import CubedSphereGrid

CONTAIN_TOL = 1e-12


def default_grid(nlat: int, nlon: int) -> Tuple[np.ndarray, np.ndarray]:
    """Cell-centred lat [nlat], lon [nlon] in radians."""
    lat = -0.5 * math.pi + (np.arange(nlat) + 0.5) * (math.pi / nlat)
    lon = (np.arange(nlon) + 0.5) * (2.0 * math.pi / nlon)
    return lat, lon


# ----------------------------------------------------------------------------
# the dual mesh
# ----------------------------------------------------------------------------

class DualMesh:
    """Edge quads and corner triangles of the C<N> dual mesh (the interior
    quads need no table).  ``equad[E, 4]``: cells A0, A1 (own panel, along the
    edge), B0, B1 (their partners); ``eid[f, side, j]``: index into ``equad`` of
    the quad between border cells j, j + 1 of panel f, side W, E, S, N;
    ``tri[8, 3]`` ascending cell ids, ``ctri[f, quadrant]`` (quadrant = (x side
    E) | 2 (y side N)) index into ``tri``."""

    def __init__(self, N: int):
        if N < 2:
            raise ValueError("the dual mesh needs N >= 2")
        self.N = N
        lay = TileLayout(N, 1, 1, ng=1)
        gs = lay.ghost_sources(0)[:, :, 0, :]                     # [6, 4, N] partner across W, E, S, N
        pos = np.arange(N)
        own = np.empty((6, 4, N), dtype=np.int64)
        for f in range(6):
            own[f, 0] = lay.global_flat(f, 0, pos)
            own[f, 1] = lay.global_flat(f, N - 1, pos)
            own[f, 2] = lay.global_flat(f, pos, 0)
            own[f, 3] = lay.global_flat(f, pos, N - 1)
        self.nint = 6 * (N - 1) ** 2
        quads, key = [], {}
        eid = np.full((6, 4, max(N - 1, 1)), -1, dtype=np.int64)
        for f in range(6):
            for s in range(4):
                for j in range(N - 1):
                    q = (own[f, s, j], own[f, s, j + 1], gs[f, s, j], gs[f, s, j + 1])
                    k = frozenset(q)
                    if k not in key:              # first seen from the lower panel: its orientation
                        key[k] = len(quads)
                        quads.append(q)
                    eid[f, s, j] = key[k]
        self.equad = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
        self.eid = eid
        assert len(quads) == 12 * (N - 1) and len({c for q in quads for c in q}) == 24 * (N - 1)
        tris, tkey = [], {}
        ctri = np.empty((6, 4), dtype=np.int64)
        for f in range(6):
            for quad in range(4):
                xs, ys = quad & 1, quad >> 1                      # E / N end
                px = N - 1 if ys else 0                           # position along the W / E strip
                py = N - 1 if xs else 0                           # position along the S / N strip
                c = own[f, xs, px]
                assert c == own[f, 2 + ys, py]
                t = tuple(sorted({int(c), int(gs[f, xs, px]), int(gs[f, 2 + ys, py])}))
                assert len(t) == 3
                if t not in tkey:
                    tkey[t] = len(tris)
                    tris.append(t)
                ctri[f, quad] = tkey[t]
        assert len(tris) == 8
        self.tri = np.asarray(tris, dtype=np.int64)
        self.ctri = ctri
        self.nelem = self.nint + len(quads) + 8

    def element_cells(self) -> np.ndarray:
        """[nelem, 4] cells of every element in id order (-1 in a triangle's
        fourth slot); interior quads as (j, i), (j, i+1), (j+1, i), (j+1, i+1)."""
        N = self.N
        f, j, i = np.meshgrid(np.arange(6), np.arange(N - 1), np.arange(N - 1), indexing="ij")
        c = ((f * N + j) * N + i).reshape(-1)
        inter = np.stack([c, c + 1, c + N, c + N + 1], 1)
        tri = np.concatenate([self.tri, np.full((8, 1), -1, dtype=np.int64)], 1)
        return np.concatenate([inter, self.equad, tri])


def _tangent_basis(p: np.ndarray):
    a = np.where((np.abs(p[:, 0]) < 0.9)[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    e1 = np.cross(a, p)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    return e1, np.cross(p, e1)


def _gnomonic(v: np.ndarray, p: np.ndarray, e1: np.ndarray, e2: np.ndarray):
    """Coordinates of unit vectors v [M, m, 3] in the plane tangent at p [M, 3]
    (p at the origin) and the mask of vectors on p's side of the sphere."""
    d = np.einsum("mkc,mc->mk", v, p)
    ok = d > 1e-3
    g = v / np.where(ok, d, 1.0)[..., None]
    return np.stack([np.einsum("mkc,mc->mk", g, e1), np.einsum("mkc,mc->mk", g, e2)], -1), ok


def quad_weights(P: np.ndarray):
    """(bilinear weights [M, 4], inside measure min(s, 1-s, t, 1-t) [M]) of the
    origin in the plane quads P [M, 4, 2] (vertices 00, 10, 01, 11): Newton on
    the inverse bilinear map from (1/2, 1/2)."""
    A, B, C, D = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], P[:, 0] - P[:, 1] - P[:, 2] + P[:, 3]
    s = np.full(len(P), 0.5)
    t = np.full(len(P), 0.5)
    for _ in range(12):
        r = A + B * s[:, None] + C * t[:, None] + D * (s * t)[:, None]
        js = B + D * t[:, None]
        jt = C + D * s[:, None]
        det = js[:, 0] * jt[:, 1] - js[:, 1] * jt[:, 0]
        det = np.where(det == 0, 1.0, det)
        s = s - (r[:, 0] * jt[:, 1] - r[:, 1] * jt[:, 0]) / det
        t = t - (js[:, 0] * r[:, 1] - js[:, 1] * r[:, 0]) / det
    return np.stack([(1 - s) * (1 - t), s * (1 - t), (1 - s) * t, s * t], 1), np.minimum(np.minimum(s, 1 - s),
                                                                                     np.minimum(t, 1 - t))


def tri_weights(P: np.ndarray):
    """(barycentric weights [M, 4], fourth 0; their minimum [M]) of the origin in
    the triangles P [M, 3, 2]."""
    a, b, c = P[:, 0], P[:, 1], P[:, 2]
    cr = lambda u, v: u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    area = cr(b - a, c - a)
    area = np.where(area == 0, 1.0, area)
    w1 = cr(-a, c - a) / area
    w2 = cr(b - a, -a) / area
    w0 = (1.0 - w1) - w2
    w = np.stack([w0, w1, w2, np.zeros_like(w0)], 1)
    return w, np.minimum(w0, np.minimum(w1, w2))


def _element_weights(cells: np.ndarray, p: np.ndarray, ctr: np.ndarray):
    """(w [M, 4], inside measure [M]) of the points p [M, 3] in the border
    elements ``cells`` [M, 4] (fourth -1: triangle); inside < 0: the point is
    outside (or the element is on the far side of the sphere: -inf)."""
    e1, e2 = _tangent_basis(p)
    tri = cells[:, 3] < 0
    v = ctr[np.where(cells >= 0, cells, cells[:, :1])]
    P, ok = _gnomonic(v, p, e1, e2)
    w = np.zeros((len(p), 4))
    ins = np.full(len(p), -np.inf)
    m = ~tri
    if m.any():
        w[m], ins[m] = quad_weights(P[m])
    if tri.any():
        w[tri], ins[tri] = tri_weights(P[tri, :3])
    ins[~ok.all(1)] = -np.inf
    return w, ins


def _best(cells, cand, p, ctr):
    """Per point: weights, inside measure and index of the lowest candidate
    that contains it (none does: the candidate nearest to containing it)."""
    M, nc = cand.shape
    w = np.zeros((M, 4))
    ins = np.full(M, -np.inf)
    el = np.zeros(M, dtype=np.int64)
    found = np.zeros(M, dtype=bool)
    order = np.sort(np.where(cand >= 0, cand, np.iinfo(np.int64).max), 1)
    for c in range(nc):
        e = order[:, c]
        m = np.nonzero((e != np.iinfo(np.int64).max) & ~found)[0]
        if c and m.size:
            m = m[e[m] != order[m, c - 1]]
        if not m.size:
            continue
        wc, ic = _element_weights(cells[e[m]], p[m], ctr)
        better = ic > ins[m]
        mb = m[better]
        w[mb], ins[mb], el[mb] = wc[better], ic[better], e[m][better]
        found[m[ic >= -CONTAIN_TOL]] = True
    return w, ins, el


def locate_points(N: int, p: np.ndarray, mesh: Optional[DualMesh] = None):
    """(src [K, 4] global cell ids, w [K, 4] weights, elem [K] element ids,
    margin [K]) of the unit vectors p [K, 3] on the C<N> dual mesh (see the
    module docstring).  ``margin`` is the distance of the point from the border
    of the element that holds it: min(tx, 1 - tx, ty, 1 - ty) in cell units for
    an interior quad, the inside measure (``quad_weights`` / ``tri_weights``) for
    an edge quad or a corner triangle."""
    mesh = DualMesh(N) if mesh is None else mesh
    K = len(p)
    dn = p @ FACE_FRAMES[:, 0].T                               # [K, 6]
    face = np.argmax(dn, 1)                                    # ties: the lowest panel
    fr = FACE_FRAMES[face]
    d = np.einsum("kc,kc->k", p, fr[:, 0])
    da = 0.5 * math.pi / N
    x = (np.arctan(np.einsum("kc,kc->k", p, fr[:, 1]) / d) + 0.25 * math.pi) / da - 0.5
    y = (np.arctan(np.einsum("kc,kc->k", p, fr[:, 2]) / d) + 0.25 * math.pi) / da - 0.5
    # a point within rounding of a dual grid line is on it: the tie rule decides
    x = np.where(np.abs(x - np.round(x)) <= CONTAIN_TOL, np.round(x), x)
    y = np.where(np.abs(y - np.round(y)) <= CONTAIN_TOL, np.round(y), y)
    src = np.zeros((K, 4), dtype=np.int64)
    w = np.zeros((K, 4))
    elem = np.zeros(K, dtype=np.int64)
    margin = np.zeros(K)
    xlo, xhi, ylo, yhi = x < 0, x > N - 1, y < 0, y > N - 1
    inner = ~(xlo | xhi | ylo | yhi)
    # interior quads: bilinear in (alpha, beta); a point on a dual grid line goes to
    # the lower quad (the lowest id)
    k = np.nonzero(inner)[0]
    i0 = np.clip(np.ceil(x[k]) - 1, 0, N - 2).astype(np.int64)
    j0 = np.clip(np.ceil(y[k]) - 1, 0, N - 2).astype(np.int64)
    tx, ty = x[k] - i0, y[k] - j0
    c = (face[k] * N + j0) * N + i0
    src[k] = np.stack([c, c + 1, c + N, c + N + 1], 1)
    w[k] = np.stack([(1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty], 1)
    elem[k] = (face[k] * (N - 1) + j0) * (N - 1) + i0
    margin[k] = np.minimum(np.minimum(tx, 1 - tx), np.minimum(ty, 1 - ty))
    # border band: candidates are the edge quads next to the point on each side it
    # is beyond, and the nearest corner triangle
    k = np.nonzero(~inner)[0]
    if k.size:
        cells = mesh.element_cells()[mesh.nint:]
        nq = len(mesh.equad)
        f, xk, yk = face[k], x[k], y[k]
        cand = np.full((k.size, 7), -1, dtype=np.int64)
        jy = np.clip(np.floor(yk), 0, N - 2).astype(np.int64)
        jx = np.clip(np.floor(xk), 0, N - 2).astype(np.int64)
        xs = np.where(xhi[k], 1, 0)
        ys = np.where(yhi[k], 3, 2)
        bx, by = xlo[k] | xhi[k], ylo[k] | yhi[k]
        for o in (-1, 0, 1):
            cand[:, 1 + o] = np.where(bx, mesh.eid[f, xs, np.clip(jy + o, 0, N - 2)], -1)
            cand[:, 4 + o] = np.where(by, mesh.eid[f, ys, np.clip(jx + o, 0, N - 2)], -1)
        cand[:, 6] = nq + mesh.ctri[f, (xk > 0.5 * (N - 1)) * 1 + (yk > 0.5 * (N - 1)) * 2]
        ctr = CubedSphereGrid(N).centers().reshape(-1, 3)
        bw, bins, bel = _best(cells, cand, p[k], ctr)
        if (bins < -1e-9).any():
            raise RuntimeError("lat-lon tables: a target point lies in none of its neighbouring elements")
        cc = cells[bel]
        src[k] = np.where(cc >= 0, cc, cc[:, :1])
        w[k] = bw
        elem[k] = mesh.nint + bel
        margin[k] = bins
    return src, w, elem, margin


class LatLonTables:
    """Sources and weights of a lat-lon target grid on C<N> (see the module
    docstring).  ``elem[K]`` is the id of the element that holds each point."""

    def __init__(self, N: int, lat: np.ndarray, lon: np.ndarray):
        lat = np.ascontiguousarray(lat, dtype=np.float64).reshape(-1)
        lon = np.ascontiguousarray(lon, dtype=np.float64).reshape(-1)
        if lat.size == 0 or lon.size == 0:
            raise ValueError("lat-lon grid: empty lat or lon")
        if (np.diff(lat) <= 0).any() or (np.diff(lon) <= 0).any():
            raise ValueError("lat-lon grid: lat and lon must be ascending")
        if np.abs(lat).max() > 0.5 * math.pi + 1e-12:
            raise ValueError("lat-lon grid: |lat| beyond pi/2")
        self.N, self.lat, self.lon = int(N), lat, lon
        self.nlat, self.nlon = lat.size, lon.size
        self.K = self.nlat * self.nlon
        la, lo = np.meshgrid(lat, lon, indexing="ij")
        la, lo = la.reshape(-1), lo.reshape(-1)
        cl = np.cos(la)
        self.p = np.stack([cl * np.cos(lo), cl * np.sin(lo), np.sin(la)], 1)
        self.east = np.stack([-np.sin(lo), np.cos(lo), np.zeros_like(lo)], 1)
        self.north = np.stack([-np.sin(la) * np.cos(lo), -np.sin(la) * np.sin(lo), cl], 1)
        self.mesh = DualMesh(self.N)
        self._locate()

    # ---- location and weights ------------------------------------------------------
    def _locate(self) -> None:
        self.src, self.w, self.elem, _ = locate_points(self.N, self.p, self.mesh)

    # ---- per-rank index tables -------------------------------------------------------
    def rank_index(self, layout: TileLayout, rank: int) -> Tuple[np.ndarray, np.ndarray]:
        """(padded [K, 4], unpadded [K, 4]) int32 indices of the sources in the
        rank's padded storage [T P P] and in its [T, n, n] tiles; -1 where the
        rank does not own the source."""
        if layout.N != self.N:
            raise ValueError(f"tables are for C{self.N}, the layout is C{layout.N}")
        pad, unp = layout.cell_maps(rank)
        return pad[self.src], unp[self.src]


_TABLES: Dict[tuple, LatLonTables] = {}


def tables_for(N: int, lat: np.ndarray, lon: np.ndarray) -> LatLonTables:
    """Cached ``LatLonTables`` (built once per (N, lat, lon))."""
    lat = np.ascontiguousarray(lat, dtype=np.float64)
    lon = np.ascontiguousarray(lon, dtype=np.float64)
    key = (int(N), lat.tobytes(), lon.tobytes())
    if key not in _TABLES:
        if len(_TABLES) >= 8:
            _TABLES.pop(next(iter(_TABLES)))
        _TABLES[key] = LatLonTables(N, lat, lon)
    return _TABLES[key]


# ----------------------------------------------------------------------------
# the PyTorch twin
# ----------------------------------------------------------------------------

@dataclass
class RegridTables:
    """What the twin and the kernel read for one source layout: ``idx`` [K, 4]
    int32 (-1: skipped), ``w`` [K, 4] float64, ``east`` / ``north`` [K, 3]
    float64, all on one device."""
    idx: torch.Tensor
    w: torch.Tensor
    east: torch.Tensor
    north: torch.Tensor
    nlat: int
    nlon: int


def regrid_tables(tab: LatLonTables, idx: Optional[np.ndarray] = None, device="cpu") -> RegridTables:
    """``RegridTables`` of an index table (default: the global cell ids, for a
    source [..., 6 N N])."""
    if idx is None:
        idx = tab.src.astype(np.int32)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)
    return RegridTables(t(idx), t(tab.w), t(tab.east), t(tab.north), tab.nlat, tab.nlon)


def _slots(tb: RegridTables, dtype):
    m = tb.idx >= 0
    return torch.where(m, tb.idx, torch.zeros_like(tb.idx)).long(), m, tb.w.to(dtype)


def fold_terms(t: torch.Tensor) -> torch.Tensor:
    """[C, 4, K] terms -> [C, K]: ((t0 + t1) + t2) + t3."""
    return ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]


def regrid_terms(fields: torch.Tensor, tb: RegridTables) -> torch.Tensor:
    """[C, 4, K] the terms t = w x of the scalar channels ``fields`` [C, ...]
    (flattened per channel to the layout ``tb.idx`` indexes); 0 for a skipped
    slot.  The terms of several ranks add exactly (one rank owns each)."""
    x = fields.reshape(fields.shape[0], -1)
    i, m, w = _slots(tb, x.dtype)
    zero = torch.zeros((), dtype=x.dtype, device=x.device)
    return torch.stack([torch.where(m[:, s], w[:, s] * x[:, i[:, s]], zero) for s in range(4)], 1)


def regrid(fields: torch.Tensor, tb: RegridTables) -> torch.Tensor:
    """[C, nlat, nlon] of the scalar channels ``fields`` [C, ...]."""
    return fold_terms(regrid_terms(fields, tb)).reshape(fields.shape[0], tb.nlat, tb.nlon)


def velocity_terms(h: torch.Tensor, M: torch.Tensor, tb: RegridTables) -> torch.Tensor:
    """[3, 4, K] terms of the Cartesian velocity: v = M / h at each source cell
    (h == 0: M itself, as the derived fields) times its weight."""
    h = h.reshape(-1)
    M = M.reshape(3, -1)
    i, m, w = _slots(tb, h.dtype)
    zero = torch.zeros((), dtype=h.dtype, device=h.device)
    t = []
    for s in range(4):
        hs = h[i[:, s]]
        safe = torch.where(hs != 0, hs, torch.ones_like(hs))
        t.append(torch.where(m[:, s], w[:, s] * (M[:, i[:, s]] / safe), zero))
    return torch.stack(t, 1)


def velocity(h: torch.Tensor, M: torch.Tensor, tb: RegridTables) -> torch.Tensor:
    """[3, nlat, nlon] Cartesian velocity interpolated from v = M / h."""
    return fold_terms(velocity_terms(h, M, tb)).reshape(3, tb.nlat, tb.nlon)


def project(vc: torch.Tensor, tb: RegridTables) -> torch.Tensor:
    """[2, nlat, nlon] (u, v): the Cartesian triple onto east and north."""
    v = vc.reshape(3, -1)
    e, n = tb.east.to(v.dtype).T, tb.north.to(v.dtype).T
    u = (v[0] * e[0] + v[1] * e[1]) + v[2] * e[2]
    nv = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]
    return torch.stack([u, nv]).reshape(2, tb.nlat, tb.nlon)


def winds(h: torch.Tensor, M: torch.Tensor, tb: RegridTables) -> torch.Tensor:
    """[2, nlat, nlon] zonal and meridional wind of the state (h, M)."""
    return project(velocity(h, M, tb), tb)


def zonal_mean(x: torch.Tensor) -> torch.Tensor:
    """[..., nlat] float64 mean over longitude of [..., nlat, nlon]."""
    return x.to(torch.float64).sum(-1) / x.shape[-1]
