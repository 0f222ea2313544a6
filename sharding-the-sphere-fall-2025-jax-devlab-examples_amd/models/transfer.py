"""Grid transfer between equiangular cubed-sphere grids C_Ns -> C_N with N = r Ns
(refine) or Ns = r N (coarsen), r in 2, 4, 8: the definitions, the host tables and
the PyTorch float64 twin of ``ops/csrc/transfer_kernel.hip`` (``ops/transfer.py``
drives either).

The grid lines of C_N are a subset of those of C_{rN}, so a coarse cell P is the
exact union of its r x r children c, and with the exact areas of
``models/geometry.py`` sum_c a_c = A_P to rounding.  Below, a "fold" over the
children of a parent is a plain left-to-right sum in the order rows ascending,
then columns ascending; sa = fold(a_c).

Coarsen, every row:   Q_P = fold(a_c q_c) / sa;  a momentum triple is then projected
onto the tangent plane at the parent's centre, M - (M . c_P) c_P.

Refine, per coarse cell P and reconstructed scalar s (a channel, or a primitive):

1. G = sum_k W_k (s_k - s_P) over the four edge neighbours k = W, E, S, N: the
   least-squares weights of ``models/dissipation.py`` (``dissipation_tables`` on the
   bare source grid) times R, so that G acts on differences of unit vectors.  A
   neighbour across a cube edge is the real cell there (``neighbor_table``).
2. d_c = (G . (c_c - c_P)) - fold(a_c (G . (c_c - c_P))) / sa: mean-free under the areas.
3. Barth-Jespersen: phi = min(1, (max - s_P) / max_c d_c, (min - s_P) / min_c d_c)
   with min / max over P and its four neighbours (a ratio only where its d has the
   sign to matter); phi = 0 where every d_c is 0; ``limiter="none"``: phi = 1.
4. s_c = s_P + phi d_c, with ``"bj"`` clamped to [min, max] (phi d_c rounds, the
   clamp makes "no new extremum" exact; it moves a value by an ulp at most).

Kinds (``channel_kinds``): 0 a conservative scalar, s = the row; 1 the momentum
triple of a depth row h, s = the three components of v = M / h (h == 0: v = 0),
v_c projected onto the tangent plane at c_c, M_c = h_c v_c; 2 the tracer mass of a
depth row, s = q = hq / h (h == 0: 0) and hq_c = h_c (q_c + delta) with
delta = (sa hq_P - fold(a_c h_c q_c)) / fold(a_c h_c) (0 where the divisor is 0):
tracer mass is conserved to rounding and q = const stays constant; delta is second
order small and may carry q past its bounds by that much.  (sa stands for A_P: the
two agree to rounding, and with sa a refined state coarsens back to its source.)
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from ..parallel.layout import TileLayout
from ..parallel.topology import neighbor_cells
from .base import RankGeometry
from .dissipation import dissipation_tables
from .geometry import CubedSphereGrid

RATIOS = (2, 4, 8)
LIMITERS = ("bj", "none")
MAX_FIELDS = 32
MAX_SLOTS = 8               # a depth row with its dependants: h, one triple, four tracers


def channel_kinds(physics) -> Tuple[List[int], List[int]]:
    """(kind [F], depth [F]) of a physics' rows; depth is the row of h for the
    kinds 1 and 2, -1 for kind 0."""
    F = int(physics.F)
    if getattr(physics, "name", None) != "swe":
        return [0] * F, [-1] * F
    if getattr(physics, "kernel_id", None) == 4:                 # layers: (h_k, M_k) per layer
        return [0, 1, 1, 1] * (F // 4), [d for k in range(F // 4) for d in (-1, 4 * k, 4 * k, 4 * k)]
    return [0, 1, 1, 1] + [2] * (F - 4), [-1, 0, 0, 0] + [0] * (F - 4)


def direction(Ns: int, N: int) -> Tuple[str, int]:
    """("refine" | "coarsen" | "copy", r) of a transfer C_Ns -> C_N; ValueError for
    any other ratio than 1, 2, 4, 8."""
    if Ns == N:
        return "copy", 1
    for r in RATIOS:
        if N == r * Ns:
            return "refine", r
        if Ns == r * N:
            return "coarsen", r
    raise ValueError(f"grid transfer: C{Ns} -> C{N} is not a ratio of {RATIOS} in either direction "
                     f"(other ratios are not supported; chain two transfers beyond 8)")


def neighbor_table(Ns: int) -> np.ndarray:
    """[6 Ns^2, 4] global index of the cell across the W, E, S, N edge of every cell."""
    J, I = np.mgrid[0:Ns, 0:Ns]
    out = np.empty((6, Ns, Ns, 4), dtype=np.int64)
    for f in range(6):
        for k, (di, dj) in enumerate(((-1, 0), (1, 0), (0, -1), (0, 1))):
            F2, I2, J2 = neighbor_cells(Ns, f, I + di, J + dj)
            out[f, :, :, k] = (F2 * Ns + J2) * Ns + I2
    assert out.min() >= 0 and out.max() < 6 * Ns * Ns
    return out.reshape(-1, 4)


def gradient_weights(grid: CubedSphereGrid) -> np.ndarray:
    """[6 Ns^2, 4, 3]: R W of ``dissipation_tables`` on the whole grid as one rank."""
    geo = RankGeometry(grid, TileLayout(grid.N, 1, 1, ng=1), 0)
    return (dissipation_tables(geo)["W"] * grid.radius).reshape(-1, 4, 3)


def _fold(x: torch.Tensor) -> torch.Tensor:
    """[K, r r] -> [K]: left to right."""
    acc = x[:, 0]
    for k in range(1, x.shape[1]):
        acc = acc + x[:, k]
    return acc


def _children(a: torch.Tensor, r: int) -> torch.Tensor:
    """[6, r n, r n, ...] -> [6 n n, r r, ...]: the children of every parent, rows then columns."""
    n = a.shape[1] // r
    t = a.reshape((6, n, r, n, r) + a.shape[3:])
    perm = (0, 1, 3, 2, 4) + tuple(range(5, t.dim()))
    return t.permute(perm).reshape((6 * n * n, r * r) + a.shape[3:])


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def coarsen(src: torch.Tensor, kind, fine: CubedSphereGrid, coarse: CubedSphereGrid) -> torch.Tensor:
    """[F, 6, r N, r N] -> [F, 6, N, N] float64."""
    N, r = coarse.N, fine.N // coarse.N
    src = src.to(torch.float64)
    a = _children(torch.as_tensor(fine.areas()), r)
    sa = _fold(a)
    out = torch.stack([_fold(a * _children(src[f], r)) / sa for f in range(src.shape[0])])
    c = torch.as_tensor(coarse.centers()).reshape(-1, 3)
    f = 0
    while f < len(kind):
        if kind[f] == 1:
            M = out[f:f + 3].T
            out[f:f + 3] = (M - _dot3(M, c)[:, None] * c).T
            f += 3
        else:
            f += 1
    return out.reshape(-1, 6, N, N)


class RefineTwin:
    """The refinement C_Ns -> C_{r Ns} with its tables; ``phi`` of the last call is
    kept per reconstructed scalar (tests measure the share of limited cells)."""

    def __init__(self, coarse: CubedSphereGrid, fine: CubedSphereGrid):
        self.Ns, self.N, self.r = coarse.N, fine.N, fine.N // coarse.N
        self.nbr = torch.as_tensor(neighbor_table(coarse.N))
        self.W = torch.as_tensor(gradient_weights(coarse))
        self.cP = torch.as_tensor(coarse.centers()).reshape(-1, 3)
        self.cc = _children(torch.as_tensor(fine.centers()), self.r)            # [K, rr, 3]
        self.e = self.cc - self.cP[:, None, :]
        self.a = _children(torch.as_tensor(fine.areas()), self.r)
        self.sa = _fold(self.a)
        self.phi: List[torch.Tensor] = []

    def scalar(self, s: torch.Tensor, limiter: str) -> torch.Tensor:
        """Children [K, rr] of the scalar s [K]."""
        nb = s[self.nbr]
        dif = nb - s[:, None]
        W = self.W
        G = [((W[:, 0, k] * dif[:, 0] + W[:, 1, k] * dif[:, 1]) + W[:, 2, k] * dif[:, 2]) + W[:, 3, k] * dif[:, 3]
             for k in range(3)]
        e = self.e
        d = (G[0][:, None] * e[..., 0] + G[1][:, None] * e[..., 1]) + G[2][:, None] * e[..., 2]
        d = d - (_fold(self.a * d) / self.sa)[:, None]
        lo = torch.minimum(s, nb.amin(1))
        hi = torch.maximum(s, nb.amax(1))
        if limiter == "none":
            phi = torch.ones_like(s)
        else:
            dmax, dmin = d.amax(1), d.amin(1)
            one = torch.ones_like(s)
            pmax = torch.where(dmax > 0, (hi - s) / torch.where(dmax > 0, dmax, one), one)
            pmin = torch.where(dmin < 0, (lo - s) / torch.where(dmin < 0, dmin, one), one)
            phi = torch.minimum(one, torch.minimum(pmax, pmin))
            phi = torch.where((dmax == 0) & (dmin == 0), torch.zeros_like(s), phi)
        self.phi.append(phi)
        v = s[:, None] + phi[:, None] * d
        if limiter != "none":
            v = torch.minimum(torch.maximum(v, lo[:, None]), hi[:, None])
        return v

    def __call__(self, src: torch.Tensor, kind, depth, limiter: str = "bj") -> torch.Tensor:
        """[F, 6, Ns, Ns] -> [F, 6, N, N] float64."""
        if limiter not in LIMITERS:
            raise ValueError(f"grid transfer: limiter in {LIMITERS} expected, not {limiter!r}")
        F, r, Ns = src.shape[0], self.r, self.Ns
        q = src.to(torch.float64).reshape(F, -1)
        self.phi = []
        out = torch.empty((F,) + tuple(self.a.shape), dtype=torch.float64)
        prim = lambda f: torch.where(q[depth[f]] != 0, q[f] / torch.where(q[depth[f]] != 0, q[depth[f]], 1.0), 0.0)
        for f in range(F):
            if kind[f] == 0:
                out[f] = self.scalar(q[f], limiter)
        f = 0
        while f < F:
            if kind[f] == 1:
                hc = out[depth[f]]
                v = torch.stack([self.scalar(prim(f + k), limiter) for k in range(3)], -1)
                v = v - _dot3(v, self.cc)[..., None] * self.cc
                for k in range(3):
                    out[f + k] = hc * v[..., k]
                f += 3
                continue
            if kind[f] == 2:
                hc = out[depth[f]]
                qc = self.scalar(prim(f), limiter)
                w = self.a * hc
                T, Wsum = _fold(w * qc), _fold(w)
                delta = torch.where(Wsum != 0, (self.sa * q[f] - T) / torch.where(Wsum != 0, Wsum, 1.0), 0.0)
                out[f] = hc * (qc + delta[:, None])
            f += 1
        out = out.reshape(F, 6, Ns, Ns, r, r).permute(0, 1, 2, 4, 3, 5)
        return out.reshape(F, 6, self.N, self.N)


def transfer(src, physics, N: int, radius: float, limiter: str = "bj") -> torch.Tensor:
    """The twin of ``Solver.set_from_cubed``: the global state [F, 6, Ns, Ns] of
    ``physics`` on C_N, float64."""
    src = torch.as_tensor(np.asarray(src) if not isinstance(src, torch.Tensor) else src).detach().cpu().to(torch.float64)
    way, r = direction(int(src.shape[-1]), N)
    kind, depth = channel_kinds(physics)
    if limiter not in LIMITERS:
        raise ValueError(f"grid transfer: limiter in {LIMITERS} expected, not {limiter!r}")
    if way == "copy":
        return src.clone()
    gs, gt = CubedSphereGrid(int(src.shape[-1]), radius), CubedSphereGrid(N, radius)
    if way == "coarsen":
        return coarsen(src, kind, gs, gt)
    return RefineTwin(gs, gt)(src, kind, depth, limiter)
