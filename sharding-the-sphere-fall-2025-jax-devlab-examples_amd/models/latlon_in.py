"""Lat-lon input: cubed-sphere states from gridded h, u, v and scalars.  The
definitions and the numpy twin (the oracle) of ``ops/csrc/latlon_in_kernel.hip``;
the inverse direction of ``models/latlon.py``.

Source grid (``source_grid``): ``lat[nlat]`` ascending and uniform, either with
both poles (lat[0] = -pi/2, lat[-1] = pi/2) or cell-centred (first and last row
half a spacing from the poles); ``lon[nlon]`` uniform over the full circle, nlon
even and >= 8, nlat >= 4.  The twin and the kernel read the grid as (lat0, dlat,
lon0, dlon): node j, i lies at lat0 + j dlat, lon0 + i dlon.

Channels (``channel_plan``, ``prepare``): scalars go in as they are; (u, v) (east,
north, m/s) becomes the Cartesian V = u e(lon) + v n(lat, lon) at every node
before anything is interpolated, and on a pole row (where every longitude names
the same vector) the row is replaced by the mean of its nlon vectors, summed in
ascending longitude, ((V_0 + V_1) + V_2) + ...  From there Vx, Vy, Vz are
scalars: nothing is divided by cos(lat) and crossing a pole flips no sign.  The
work copy is [C, nlat, nlon], ordered h, Vx, Vy, Vz, tracers (whichever are given).

Indexing: the longitude index wraps modulo nlon; a latitude index beyond a pole
reflects across it (j -> -j with pole rows, j -> -1 - j cell-centred, likewise in
the north) and the longitude index of that row shifts by nlon / 2.

Interpolation (``tap_weights``) at x = (lon - lon0) / dlon, y = (lat - lat0) / dlat,
base index floor, fraction t: order 1 is bilinear (2 x 2 taps, monotone), order 3
the piecewise cubic Lagrange polynomial through the nodes -1, 0, 1, 2 (4 x 4 taps,
fourth order, not monotone).  Both are continuous across source grid lines.  A
value is  sum_a wy_a (sum_b wx_b f_ab), both sums left to right.

Cell value (``ingest``), quadrature q in {1, 2, 4}: the q x q Gauss-Legendre points
of the cell in its equiangular (alpha, beta), alpha = ((2 I + 1 - N) + g) dalpha / 2
(exactly 0 at the centre of an odd panel, so a polar cell centre has longitude 0
by atan2(+0, +0)), unit vectors by the gnomonic map of ``models/geometry.py``,
weights w = w_a w_b (1 + X^2)(1 + Y^2) / (1 + X^2 + Y^2)^(3/2).  The weighted values
and the weights are folded pairwise (point 2k with 2k + 1, then pairs of pairs: the
kernel's lane butterfly) and divided, so a constant is reproduced to rounding.
q = 1 is the value at the cell centre.

Shallow water: the averaged V is projected onto the tangent plane at the cell
centre, M = h V_t and hq_k = h q_k, with h the ingested depth when ``h`` is
given and the state's present depth otherwise.  h is the layer depth and the
topography stays the case's: a free-surface height or a topography field is not
ingested.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from ..parallel.topology import FACE_FRAMES

ORDERS = (1, 3)
QUADRATURES = (1, 2, 4)
MAX_CHANNELS = 8
GRID_TOL = 1e-9                       # relative to the spacing

# Gauss-Legendre nodes and weights on [-1, 1] as float64 constants (the kernel's)
GAUSS = {
    1: ((0.0,), (2.0,)),
    2: ((-0.5773502691896257, 0.5773502691896257), (1.0, 1.0)),
    4: ((-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526),
        (0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538)),
}


@dataclass(frozen=True)
class SourceGrid:
    nlat: int
    nlon: int
    lat0: float
    dlat: float
    lon0: float
    dlon: float
    poles: bool


def source_grid(lat, lon) -> SourceGrid:
    """The checked source grid of ``lat`` / ``lon`` (radians); ``ValueError``
    naming the reason for anything the ingest does not take."""
    lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    lon = np.asarray(lon, dtype=np.float64).reshape(-1)
    if lat.size < 4:
        raise ValueError(f"lat-lon input: nlat = {lat.size}; at least 4 latitude rows are needed")
    if lon.size < 8 or lon.size % 2:
        raise ValueError(f"lat-lon input: nlon = {lon.size}; an even nlon >= 8 is needed (odd nlon: a row has no "
                         f"partner column across the pole)")
    dlat, dlon = (lat[-1] - lat[0]) / (lat.size - 1), (lon[-1] - lon[0]) / (lon.size - 1)
    if not dlat > 0 or not dlon > 0:
        raise ValueError("lat-lon input: lat and lon must be ascending")
    if np.abs(np.diff(lat) - dlat).max() > GRID_TOL * dlat:
        raise ValueError("lat-lon input: non-uniform latitudes (a Gaussian grid, for one) are not supported")
    if np.abs(np.diff(lon) - dlon).max() > GRID_TOL * dlon:
        raise ValueError("lat-lon input: non-uniform longitudes are not supported")
    if abs(lon.size * dlon - 2.0 * math.pi) > GRID_TOL * dlon * lon.size or abs(lon[0]) > 2.0 * math.pi:
        raise ValueError("lat-lon input: a regional grid is not supported (lon must cover the full circle once)")
    south, north = lat[0] + 0.5 * math.pi, 0.5 * math.pi - lat[-1]
    if abs(south) <= GRID_TOL * dlat and abs(north) <= GRID_TOL * dlat:
        poles = True
    elif abs(south - 0.5 * dlat) <= GRID_TOL * dlat and abs(north - 0.5 * dlat) <= GRID_TOL * dlat:
        poles = False
    else:
        raise ValueError("lat-lon input: a regional grid is not supported (lat must reach both poles, or end half a "
                         "spacing from each)")
    return SourceGrid(lat.size, lon.size, float(lat[0]), float(dlat), float(lon[0]), float(dlon), poles)


@dataclass(frozen=True)
class ChannelPlan:
    """What a call ingests: ``inputs`` the array names in input order (h, u, v,
    tracers), ``has_h`` / ``has_wind``, ``qfields`` the state field of each tracer
    channel; the work copy holds ``C`` channels."""
    inputs: Tuple[str, ...]
    has_h: bool
    has_wind: bool
    qfields: Tuple[int, ...]

    @property
    def C(self) -> int:
        return int(self.has_h) + 3 * int(self.has_wind) + len(self.qfields)


def channel_plan(physics, names: Sequence[str]) -> ChannelPlan:
    """The ``ChannelPlan`` of the arrays ``names`` for ``physics``; ``ValueError``
    for what it does not carry."""
    names = list(names)
    if not names:
        raise ValueError("lat-lon input: no arrays given")
    if getattr(physics, "kernel_id", None) == 4:
        raise ValueError("lat-lon input: layered runs are not supported (a gridded analysis does not say how its "
                         "depth splits over the layers)")
    if ("u" in names) != ("v" in names):
        raise ValueError("lat-lon input: u and v must be given together")
    swe = physics.name == "swe"
    if "u" in names and not swe:
        raise ValueError(f"lat-lon input: u, v are the wind of the shallow-water model, not of {physics.name!r}")
    nq = getattr(physics, "nq", 0) if swe else 0
    scalar0 = "h" if swe else physics.fields[0]
    known = [scalar0] + (["u", "v"] + [f"q{k}" for k in range(nq)] if swe else [])
    unknown = [n for n in names if n not in known]
    if unknown:
        raise ValueError(f"lat-lon input: {unknown} not among the fields {known} of this run")
    qs = [k for k in range(nq) if f"q{k}" in names]
    inputs = ([scalar0] if scalar0 in names else []) + (["u", "v"] if "u" in names else []) + [f"q{k}" for k in qs]
    return ChannelPlan(tuple(inputs), scalar0 in names, "u" in names, tuple(4 + k for k in qs))


def prepare(g: SourceGrid, plan: ChannelPlan, arrays: Dict[str, np.ndarray], ft=np.float64) -> np.ndarray:
    """The work copy [C, nlat, nlon] in ``ft`` (see the module docstring)."""
    a = {k: np.asarray(arrays[k], dtype=ft) for k in plan.inputs}
    for k, v in a.items():
        if v.shape != (g.nlat, g.nlon):
            raise ValueError(f"lat-lon input: {k} has shape {v.shape}, the grid is {(g.nlat, g.nlon)}")
    out: List[np.ndarray] = [a[plan.inputs[0]]] if plan.has_h else []
    if plan.has_wind:
        lat = (ft(g.lat0) + np.arange(g.nlat).astype(ft) * ft(g.dlat))[:, None]
        lon = (ft(g.lon0) + np.arange(g.nlon).astype(ft) * ft(g.dlon))[None, :]
        sp, cp, sl, cl = np.sin(lat), np.cos(lat), np.sin(lon), np.cos(lon)
        u, v = a["u"], a["v"]
        V = np.stack([-(u * sl) - v * (sp * cl), u * cl - v * (sp * sl), v * cp + np.zeros_like(u)])
        if g.poles:
            for j in (0, g.nlat - 1):
                s = V[:, j, 0].copy()
                for i in range(1, g.nlon):
                    s = s + V[:, j, i]
                V[:, j, :] = (s / ft(g.nlon))[:, None]
        out += list(V)
    out += [a[f"q{f - 4}"] for f in plan.qfields]
    return np.stack(out)


def _pi(ft):
    return ft(math.pi) if ft is np.float64 else np.arccos(ft(-1))


def tap_weights(t: np.ndarray, order: int) -> List[np.ndarray]:
    """The 2 (order 1) or 4 (order 3) weights of the fraction ``t``."""
    if order == 1:
        return [1.0 - t, t]
    tm, tp, t2 = t - 1.0, t + 1.0, t - 2.0
    return [-(t * tm * t2) / 6.0, (tp * tm * t2) / 2.0, -(tp * t * t2) / 2.0, (tp * t * tm) / 6.0]


def interpolate(g: SourceGrid, work: np.ndarray, lat: np.ndarray, lon: np.ndarray, order: int) -> np.ndarray:
    """[C, ...] the channels of ``work`` at the points ``lat`` / ``lon``."""
    ft = work.dtype.type
    x, y = (lon - ft(g.lon0)) / ft(g.dlon), (lat - ft(g.lat0)) / ft(g.dlat)
    i0 = np.floor(x)
    j0 = np.clip(np.floor(y), -1, g.nlat - 1)
    wx, wy = tap_weights(x - i0, order), tap_weights(y - j0, order)
    i0, j0 = i0.astype(np.int64), j0.astype(np.int64)
    first = 0 if order == 1 else -1
    cols = [np.mod(i0 + first + b, g.nlon) for b in range(len(wx))]
    val = None
    for a in range(len(wy)):
        j = j0 + first + a
        lo, hi = j < 0, j > g.nlat - 1
        r = np.where(lo, -j if g.poles else -1 - j, np.where(hi, (2 * g.nlat - 2 if g.poles else 2 * g.nlat - 1) - j, j))
        row = None
        for b in range(len(wx)):
            c = np.where(lo | hi, np.mod(cols[b] + g.nlon // 2, g.nlon), cols[b])
            term = wx[b] * work[:, r, c]
            row = term if row is None else row + term
        val = wy[a] * row if val is None else val + wy[a] * row
    return val


def cell_points(N: int, face: np.ndarray, I: np.ndarray, J: np.ndarray, q: int, ft=np.float64):
    """(p [..., q q, 3] unit vectors, w [..., q q] weights) of the Gauss points of
    the cells (face, I, J) (arrays of one shape); point l = b q + a, a along alpha."""
    gn, gw = (np.asarray(v, dtype=ft) for v in GAUSS[q])
    half = ft(0.25) * _pi(ft) / ft(N)
    ga, gb = np.tile(gn, q), np.repeat(gn, q)
    X = np.tan(((2 * I + 1 - N)[..., None].astype(ft) + ga) * half)
    Y = np.tan(((2 * J + 1 - N)[..., None].astype(ft) + gb) * half)
    fr = FACE_FRAMES.astype(ft)[face][..., None, :, :]
    p = fr[..., 0, :] + X[..., None] * fr[..., 1, :] + Y[..., None] * fr[..., 2, :]
    r2 = ft(1) + X * X + Y * Y
    r = np.sqrt(r2)
    w = (np.tile(gw, q) * np.repeat(gw, q)) * (((ft(1) + X * X) * (ft(1) + Y * Y)) / (r2 * r))
    return p / r[..., None], w


def _fold(v: np.ndarray) -> np.ndarray:
    """Pairwise fold of the last axis (1, 4 or 16 long): the kernel's butterfly."""
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def ingest(g: SourceGrid, plan: ChannelPlan, work: np.ndarray, N: int, face, I, J, order: int = 3, quadrature: int = 1,
           h_now: Optional[np.ndarray] = None) -> Dict[int, np.ndarray]:
    """{state field: values of the shape of ``face``} for the cells (face, I, J)
    of C<N>; ``h_now``: the state's present depth there (used when ``h`` is not given
    and a wind or tracer needs one)."""
    if order not in ORDERS or quadrature not in QUADRATURES:
        raise ValueError(f"lat-lon input: order in {ORDERS} and quadrature in {QUADRATURES} expected, not "
                         f"{order!r}, {quadrature!r}")
    ft = work.dtype.type
    face, I, J = (np.asarray(v, dtype=np.int64) for v in (face, I, J))
    p, w = cell_points(N, face, I, J, quadrature, ft)
    lat = np.arcsin(np.clip(p[..., 2], -1, 1))
    lon = np.arctan2(p[..., 1], p[..., 0])
    lon = np.where(lon < 0, lon + ft(2) * _pi(ft), lon)
    val = interpolate(g, work, lat, lon, order)                 # [C, ..., q q]
    val = _fold(val * w) / _fold(w)
    out: Dict[int, np.ndarray] = {}
    c = 0
    h = None if h_now is None else np.asarray(h_now, dtype=ft)
    if plan.has_h:
        h = out[0] = val[0]
        c = 1
    if plan.has_wind:
        ctr = cell_points(N, face, I, J, 1, ft)[0][..., 0, :]
        V = np.moveaxis(val[c:c + 3], 0, -1)
        d = (V[..., 0] * ctr[..., 0] + V[..., 1] * ctr[..., 1]) + V[..., 2] * ctr[..., 2]
        for k in range(3):
            out[1 + k] = h * (V[..., k] - d * ctr[..., k])
        c += 3
    for f in plan.qfields:
        out[f] = h * val[c]
        c += 1
    return out


def ingest_tiles(g: SourceGrid, plan: ChannelPlan, work: np.ndarray, layout, rank: int, order: int = 3,
                 quadrature: int = 1, h_now: Optional[np.ndarray] = None) -> Dict[int, np.ndarray]:
    """``ingest`` for the tiles [T, n, n] of a rank of ``layout``."""
    n = layout.n
    org = np.array([layout.tile_origin(t) for t in layout.rank_tiles[rank]], dtype=np.int64).reshape(-1, 3)
    jj, ii = np.mgrid[0:n, 0:n]
    face = np.broadcast_to(org[:, 0, None, None], (len(org), n, n))
    return ingest(g, plan, work, layout.N, face, org[:, 1, None, None] + ii, org[:, 2, None, None] + jj, order,
                  quadrature, h_now)
