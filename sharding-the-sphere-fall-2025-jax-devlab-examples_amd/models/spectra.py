"""Spherical-harmonic spectra of cell fields: coefficients, power per degree,
kinetic-energy spectrum.

This module holds the definitions, the host tables and the PyTorch twin (the
oracle) of ``ops/csrc/spectra_kernel.hip``.

* Real, 4 pi-normalised harmonics  Y_lm^c = P_lm(sin phi) cos m lambda,
  Y_lm^s = P_lm(sin phi) sin m lambda  with  (1 / 4 pi) int Y^2 dOmega = 1,
  so P_00 = 1 and P_10 = sqrt(3) sin phi.
* P_lm by the forward column recurrence, mu = sin phi:
      P_mm     = sqrt((2m+1) / (2m)) cos phi P_(m-1)(m-1),   P_11 = sqrt(3) cos phi
      P_(m+1)m = sqrt(2m+3) mu P_mm
      P_lm     = a_lm (mu P_(l-1)m - b_lm P_(l-2)m)
      a_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)),  b_lm = sqrt(((l-1)^2 - m^2) / (4 (l-1)^2 - 1))
  (b_(m+1)m = 0 and a_(m+1)m = sqrt(2m+3): one formula serves l > m).  The
  sectoral start is carried as  P_mm = c_m cos^m phi  with the host table
  c_m = prod_k sqrt((2k+1) / (2k)); in IEEE double the column is safe to degree
  ~1900 before P_mm underflows near the poles, and ``LMAX_CAP`` = 1023.
* Analysis: midpoint quadrature on the cubed-sphere cells,
      C_lm = sum_c w_c f_c P_lm(mu_c) cos m lambda_c,   S_lm likewise with sin,
  w_c = A_c / (4 pi R^2) from the exact cell areas, mu_c = z and lambda_c =
  atan2(y, x) of the unit cell centre.  Second order in the cell width.
  The coefficient (0, 0), the area mean sum_c w_c f_c, is summed error-free
  (``exact_sum``): within an ulp of the sum of the products however much cancels.
* Power per degree  S_l = sum_m (C_lm^2 + S_lm^2); sum_l S_l is the area-mean
  square of a band-limited field.
* Kinetic energy  E_l = R^2 / (2 l (l+1)) sum_m (|zeta_lm|^2 + |delta_lm|^2),
  E_0 = 0; sum_l E_l is the area mean of |v|^2 / 2.

All tables are float64 whatever the state's type, and so are all results.
``lmax`` is limited to min(2N - 1, LMAX_CAP): 2N is the equatorial Nyquist
wavenumber of C<N>.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

LMAX_CAP = 1023
MAX_CHANNELS = 8          # 2 C = 16 columns: one 16 x 16 matrix-core tile


def check_lmax(lmax, N: int) -> int:
    if not isinstance(lmax, (int, np.integer)) or isinstance(lmax, bool):
        raise ValueError(f"lmax: an integer expected, not {lmax!r}")
    hi = min(2 * int(N) - 1, LMAX_CAP)
    if not 0 <= lmax <= hi:
        raise ValueError(f"lmax = {lmax} outside 0 .. {hi} (min(2N - 1, {LMAX_CAP}) for C{N})")
    return int(lmax)


def recurrence_tables(lmax: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a [L+1, L+1], b [L+1, L+1], c [L+1]) float64: a[l, m], b[l, m] of the
    column recurrence for l > m (0 elsewhere), c[m] the sectoral factor."""
    L = int(lmax)
    l = np.arange(L + 1, dtype=np.float64)[:, None]
    m = np.arange(L + 1, dtype=np.float64)[None, :]
    ok = l > m
    den = np.where(ok, l * l - m * m, 1.0)
    a = np.sqrt(np.where(ok, 4.0 * l * l - 1.0, 0.0) / den)
    den = np.where(ok, 4.0 * (l - 1.0) ** 2 - 1.0, 1.0)
    b = np.where(ok, np.sqrt(np.maximum((l - 1.0) ** 2 - m * m, 0.0) / den), 0.0)
    c = np.ones(L + 1)
    for k in range(1, L + 1):
        c[k] = c[k - 1] * math.sqrt((2.0 * k + 1.0) / (2.0 * k)) if k > 1 else math.sqrt(3.0)
    return np.ascontiguousarray(a), np.ascontiguousarray(b), c


@dataclass
class SpectraTables:
    """What the twin and the kernel read: ``cell`` [cells, 4] = (mu, cos phi,
    lambda, w) per cell in the source's cell order, ``a`` / ``b`` [L+1, L+1],
    ``c`` [L+1]; all float64 on one device."""
    lmax: int
    cell: torch.Tensor
    a: torch.Tensor
    b: torch.Tensor
    c: torch.Tensor

    @property
    def cells(self) -> int:
        return self.cell.shape[0]

    def to(self, device) -> "SpectraTables":
        return SpectraTables(self.lmax, self.cell.to(device), self.a.to(device), self.b.to(device), self.c.to(device))


def make_tables(center: np.ndarray, area: np.ndarray, radius: float, lmax: int, device="cpu") -> SpectraTables:
    """Tables for the cells with unit centres ``center`` [..., 3] and areas
    ``area`` [...] (m^2) on a sphere of ``radius``."""
    p = np.asarray(center, dtype=np.float64).reshape(-1, 3)
    A = np.asarray(area, dtype=np.float64).reshape(-1)
    assert p.shape[0] == A.shape[0]
    cell = np.empty((p.shape[0], 4))
    cell[:, 0] = p[:, 2]
    cell[:, 1] = np.hypot(p[:, 0], p[:, 1])
    cell[:, 2] = np.arctan2(p[:, 1], p[:, 0])
    cell[:, 3] = A / (4.0 * math.pi * radius * radius)
    a, b, c = recurrence_tables(lmax)
    t = lambda x: torch.as_tensor(x, dtype=torch.float64, device=device)   # noqa: E731
    return SpectraTables(int(lmax), t(cell), t(a), t(b), t(c))


def grid_tables(grid, lmax: int, device="cpu") -> SpectraTables:
    """Tables of the whole C<N> grid in [6, N, N] cell order."""
    return make_tables(grid.centers(), grid.areas(), grid.radius, check_lmax(lmax, grid.N), device)


def rank_tables(geo, lmax: int, device="cpu") -> SpectraTables:
    """Tables of one rank's cells in [T, n, n] order (``RankGeometry``)."""
    return make_tables(geo.center, geo.area, geo.grid.radius, check_lmax(lmax, geo.layout.N), device)


def rank_index(plan) -> Tuple[np.ndarray, np.ndarray]:
    """(padded, unpadded) int32 [cells] position of every cell of the rank, in
    [T, n, n] order, inside one channel of the padded storage [T P P] and of an
    unpadded [T, n, n] array.  Interior slots only."""
    T, n, g = plan.T, plan.n, plan.ng
    P = n + 2 * g
    t, j, i = np.meshgrid(np.arange(T), np.arange(n), np.arange(n), indexing="ij")
    pad = ((t * P + j + g) * P + i + g).reshape(-1)
    assert pad.max(initial=0) < np.iinfo(np.int32).max
    return pad.astype(np.int32), np.arange(T * n * n, dtype=np.int32)


# ----------------------------------------------------------------------------
# the PyTorch twin
# ----------------------------------------------------------------------------

def legendre_columns(tb: SpectraTables) -> Iterator[Tuple[int, torch.Tensor]]:
    """(m, P [L+1-m, cells]) for m = 0 .. L: rows l = m .. L of column m."""
    L = tb.lmax
    mu, cphi = tb.cell[:, 0], tb.cell[:, 1]
    for m in range(L + 1):
        pmm = tb.c[m] * cphi ** m
        rows = [pmm]
        p1, p2 = pmm, torch.zeros_like(pmm)
        for l in range(m + 1, L + 1):
            p = tb.a[l, m] * (mu * p1 - tb.b[l, m] * p2)
            rows.append(p)
            p1, p2 = p, p1
        yield m, torch.stack(rows)


def exact_sum(x: torch.Tensor) -> torch.Tensor:
    """[C] sum over the last axis of ``x`` [C, n] float64, error-free: a pairwise
    tree of two-sums (hi + lo is the exact sum of the hi parts, the rounding
    errors collect in lo), hi + lo at the root.  Within an ulp of the true sum
    however much cancels."""
    hi = x
    lo = torch.zeros_like(x)
    while hi.shape[1] > 1:
        if hi.shape[1] & 1:
            z = torch.zeros_like(hi[:, :1])
            hi, lo = torch.cat([hi, z], 1), torch.cat([lo, z], 1)
        h = hi.shape[1] // 2
        a, b = hi[:, :h], hi[:, h:]
        s = a + b
        bb = s - a
        lo = (lo[:, :h] + lo[:, h:]) + ((a - (s - bb)) + (b - bb))
        hi = s
    return (hi + lo)[:, 0]


def analyse(x: torch.Tensor, tb: SpectraTables) -> torch.Tensor:
    """Coefficients [C, 2, L+1, L+1] (cos, sin; [l, m]; 0 where m > l, S_l0 = 0)
    float64 of the channels ``x`` [C, cells]."""
    if x.dim() != 2 or x.shape[1] != tb.cells:
        raise ValueError(f"analyse: [C, {tb.cells}] expected, not {tuple(x.shape)}")
    C, L = x.shape[0], tb.lmax
    if C > MAX_CHANNELS:
        raise ValueError(f"analyse: at most {MAX_CHANNELS} channels per call, not {C}")
    lam, w = tb.cell[:, 2], tb.cell[:, 3]
    wf = x.to(torch.float64) * w
    out = torch.zeros((C, 2, L + 1, L + 1), dtype=torch.float64, device=x.device)
    for m, P in legendre_columns(tb):
        ang = m * lam
        out[:, 0, m:, m] = (wf * torch.cos(ang)) @ P.T
        if m:
            out[:, 1, m:, m] = (wf * torch.sin(ang)) @ P.T
    # the area mean: its terms are w f themselves (P_00 = 1); summed error-free, so that a
    # mean that vanishes analytically is not the residue of one summation order
    out[:, 0, 0, 0] = exact_sum(wf)
    return out


def synthesise(coeffs: torch.Tensor, tb: SpectraTables) -> torch.Tensor:
    """[C, cells] float64: the band-limited field of ``coeffs`` [C, 2, L+1, L+1]
    at the cell centres."""
    C, L = coeffs.shape[0], tb.lmax
    assert coeffs.shape == (C, 2, L + 1, L + 1)
    lam = tb.cell[:, 2]
    co = coeffs.to(torch.float64)
    out = torch.zeros((C, tb.cells), dtype=torch.float64, device=coeffs.device)
    for m, P in legendre_columns(tb):
        ang = m * lam
        out += (co[:, 0, m:, m] @ P) * torch.cos(ang) + (co[:, 1, m:, m] @ P) * torch.sin(ang)
    return out


def power(coeffs: torch.Tensor) -> torch.Tensor:
    """[C, L+1] power per degree of coefficients [C, 2, L+1, L+1]."""
    return (coeffs * coeffs).sum(dim=(1, 3))


def ke_spectrum(zeta: torch.Tensor, delta: torch.Tensor, radius: float) -> torch.Tensor:
    """[L+1] kinetic energy per degree from the coefficients [2, L+1, L+1] of
    the relative vorticity and the divergence."""
    assert zeta.shape == delta.shape and zeta.dim() == 3
    L = zeta.shape[-1] - 1
    p = (zeta * zeta).sum(dim=(0, 2)) + (delta * delta).sum(dim=(0, 2))
    l = torch.arange(L + 1, dtype=torch.float64, device=zeta.device)
    f = torch.where(l > 0, radius * radius / (2.0 * l * (l + 1.0)).clamp_min(1.0), torch.zeros_like(l))
    return f * p


def sample_harmonic(tb: SpectraTables, l: int, m: int, part: str = "c") -> torch.Tensor:
    """[cells] values of Y_lm^c / Y_lm^s at the cell centres."""
    co = torch.zeros((1, 2, tb.lmax + 1, tb.lmax + 1), dtype=torch.float64, device=tb.cell.device)
    co[0, 0 if part == "c" else 1, l, m] = 1.0
    return synthesise(co, tb)[0]


# ----------------------------------------------------------------------------
# synthesis: degree factors, psi and chi, and what ops/csrc/synth_kernel.hip reads
# ----------------------------------------------------------------------------
# Sign convention: v = k x grad psi + grad chi, so zeta = lap psi and delta = lap chi;
# with lap Y_lm = -l (l+1) / R^2 Y_lm that is psi_lm = -R^2 zeta_lm / (l (l+1)) and
# likewise chi from delta.  The degree 0 of psi and chi is arbitrary and set to 0.

def _check_factor_lmax(lmax) -> int:
    if not isinstance(lmax, (int, np.integer)) or isinstance(lmax, bool) or lmax < 0:
        raise ValueError(f"lmax: a non-negative integer expected, not {lmax!r}")
    return int(lmax)


def band_factors(lmax: int, lmin: int = 0, lcut: Optional[int] = None) -> torch.Tensor:
    """[L+1] float64: 1 for lmin <= l <= lcut (default: lmax), 0 outside."""
    L = _check_factor_lmax(lmax)
    lcut = L if lcut is None else lcut
    for name, v in (("lmin", lmin), ("lcut", lcut)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValueError(f"{name}: an integer expected, not {v!r}")
    if not 0 <= lmin <= lcut:
        raise ValueError(f"band {lmin} .. {lcut}: 0 <= lmin <= lcut expected")
    l = torch.arange(L + 1)
    return ((l >= lmin) & (l <= lcut)).to(torch.float64)


def exp_factors(lmax: int, lcut: int, order: int = 2) -> torch.Tensor:
    """[L+1] float64: the exponential low-pass exp(-(l (l+1) / (lcut (lcut+1)))^order)."""
    L = _check_factor_lmax(lmax)
    if lcut < 1 or order < 1:
        raise ValueError(f"exp_factors: lcut >= 1 and order >= 1 expected, not {lcut}, {order}")
    l = torch.arange(L + 1, dtype=torch.float64)
    return torch.exp(-((l * (l + 1.0)) / (lcut * (lcut + 1.0))) ** order)


def inverse_laplacian_factors(lmax: int, radius: float) -> torch.Tensor:
    """[L+1] float64: -R^2 / (l (l+1)), 0 at l = 0."""
    L = _check_factor_lmax(lmax)
    l = torch.arange(L + 1, dtype=torch.float64)
    return torch.where(l > 0, -(radius * radius) / (l * (l + 1.0)).clamp_min(1.0), torch.zeros_like(l))


def scale_degrees(coeffs: torch.Tensor, factors) -> torch.Tensor:
    """``coeffs`` [..., L+1, L+1] ([l, m]) times ``factors`` [L+1] along l."""
    f = torch.as_tensor(factors, dtype=torch.float64, device=coeffs.device)
    if coeffs.dim() < 2 or f.shape != (coeffs.shape[-2],) or coeffs.shape[-1] != coeffs.shape[-2]:
        raise ValueError(f"scale_degrees: coefficients [..., L+1, L+1] and factors [L+1] expected, "
                         f"not {tuple(coeffs.shape)} and {tuple(f.shape)}")
    return coeffs * f[:, None]


def helmholtz(zeta: torch.Tensor, delta: torch.Tensor, radius: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(psi, chi) coefficients (m^2 / s) from those of the relative vorticity
    and the divergence, [..., L+1, L+1] each."""
    assert zeta.shape == delta.shape
    f = inverse_laplacian_factors(zeta.shape[-2] - 1, radius).to(zeta.device)
    return scale_degrees(zeta, f), scale_degrees(delta, f)


def packed_rows(lmax: int) -> int:
    return (lmax + 1) * (lmax + 2) // 2


def pack_index(lmax: int) -> Tuple[np.ndarray, np.ndarray]:
    """(l, m) int64 [R] of the packed rows: every (m, l >= m) in order of m, then
    l; R = (L+1)(L+2)/2 and the row of (m, l) is m (L+1) - m (m-1) / 2 + l - m."""
    L = int(lmax)
    m = np.repeat(np.arange(L + 1), L + 1 - np.arange(L + 1))
    start = np.arange(L + 1) * (L + 1) - np.arange(L + 1) * (np.arange(L + 1) - 1) // 2
    l = np.arange(packed_rows(L)) - start[m] + m
    return l.astype(np.int64), m.astype(np.int64)


def pack_coeffs(coeffs: torch.Tensor, index=None) -> torch.Tensor:
    """What the synthesis kernel reads: [R, 16] float64, column 2 ch + s of row
    (m, l) = ``coeffs[ch, s, l, m]``; 0 in the columns beyond 2 C and in the sine
    column of m = 0 (sin 0 = 0).  A gather of the lower triangle: entries with
    m > l and S_l0 are never read.  ``index``: ``pack_index`` as long tensors on
    the coefficients' device, when the caller keeps them."""
    C, L = coeffs.shape[0], coeffs.shape[-1] - 1
    assert coeffs.shape == (C, 2, L + 1, L + 1) and 1 <= C <= MAX_CHANNELS and coeffs.dtype == torch.float64
    if index is None:
        index = tuple(torch.as_tensor(x, device=coeffs.device) for x in pack_index(L))
    l, m = index
    out = torch.zeros((l.shape[0], 2 * MAX_CHANNELS), dtype=torch.float64, device=coeffs.device)
    out[:, :2 * C] = coeffs[:, :, l, m].permute(2, 0, 1).reshape(l.shape[0], 2 * C)
    out[:L + 1, 1::2] = 0.0                           # order 0 is the first L + 1 rows
    return out


def unpack_coeffs(packed: torch.Tensor, C: int, lmax: int) -> torch.Tensor:
    """The inverse of ``pack_coeffs``: [C, 2, L+1, L+1] with zeros at m > l and in S_l0."""
    L = int(lmax)
    l, m = (torch.as_tensor(x, device=packed.device) for x in pack_index(L))
    assert packed.shape == (l.shape[0], 2 * MAX_CHANNELS)
    out = torch.zeros((C, 2, L + 1, L + 1), dtype=torch.float64, device=packed.device)
    out[:, :, l, m] = packed[:, :2 * C].reshape(l.shape[0], C, 2).permute(1, 2, 0)
    return out


def chunk_bounds(lmax: int, chunks: int) -> list:
    """[chunks + 1] first order of each chunk of the synthesis launch, 0 = b[0] <
    b[1] < ... < b[chunks] = L + 1: contiguous, none empty, and about equal
    numbers of (degree, order) rows each (order m has L + 1 - m)."""
    L = int(lmax)
    if not isinstance(chunks, (int, np.integer)) or isinstance(chunks, bool) or not 1 <= chunks <= L + 1:
        raise ValueError(f"chunks = {chunks!r} outside 1 .. {L + 1}")
    total = packed_rows(L)
    b, m, done = [0], 0, 0
    for k in range(1, chunks):
        # at least one order, and leave one for each chunk still to come
        m, done = m + 1, done + (L + 1 - m)
        while done * chunks < k * total and m < L + 1 - (chunks - k):
            done += L + 1 - m
            m += 1
        b.append(m)
    b.append(L + 1)
    return b


def clean_coeffs(coeffs: torch.Tensor) -> torch.Tensor:
    """``coeffs`` [C, 2, L+1, L+1] with +0 at m > l and in S_l0: what a synthesis
    reads of it."""
    co = torch.tril(coeffs)
    co[:, 1, :, 0] = 0.0
    return co
