"""Local ensemble transform Kalman filter (LETKF; Hunt, Kostelich & Szunyogh
2007, Physica D 230): definitions and the PyTorch twin of
``ops/csrc/letkf_kernel.hip``.  Everything is float64.

Inputs: the members' interior states ``X [M, F, cells]``, the cell centres
``c_i`` (unit vectors) and the sphere radius R; K observations with unit vectors
``p_k``, values ``y_k``, error standard deviations ``sigma_k > 0`` and observed
field ``f_k``; a localisation length ``Lc`` (metres) or None; a multiplicative
inflation ``rho >= 1``.

Observation space:  ``Y[m, k]`` is the point sample (models/points.py) of field
f_k of member m at p_k;  ybar = ((Y_0 + Y_1) + ...) / M;  Yp = Y - ybar;
d = y - ybar.

Localisation:  s_ik = R atan2(|c_i x p_k|, c_i . p_k),  r = s_ik / Lc,
    g(r) = -r^5/4 + r^4/2 + 5r^3/8 - 5r^2/3 + 1                      0 <= r <= 1
           r^5/12 - r^4/2 + 5r^3/8 + 5r^2/3 - 5r + 4 - 2/(3r)         1 <  r <  2
           0                                                          r >= 2
(Gaspari & Cohn 1999; Lc None: g = 1, the global ETKF);  w_ik = g / sigma_k^2.

Per cell i:
    A_i  = ((M - 1) / rho) I + Yp diag(w_i) Yp^T      = Q Lam Q^T
    wbar = Q Lam^-1 Q^T Yp (w_i * d)
    Wa   = Q sqrt((M - 1) / Lam) Q^T                   (the symmetric square root)
    Xa[m, f] = xbar[f] + sum_n Xp[n, f] (wbar[n] + Wa[n, m])
with xbar the member mean and Xp = X - xbar.  A cell with no observation within
2 Lc gets xbar + sqrt(rho) Xp from the same formulas.

Hazards: the analysis does not conserve mass and does not keep h positive
(check ``h.min()``); momentum stays tangent (a linear combination of tangent
vectors at one cell); inflation acts everywhere, also where nothing is observed.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np
import torch

MIN_M, MAX_M, MAX_K = 2, 32, 65535


def gaspari_cohn(r: torch.Tensor) -> torch.Tensor:
    """g(r), r >= 0 (float64), in the Horner form of the kernel."""
    r = r.to(torch.float64)
    g1 = r * r * (r * (r * (-0.25 * r + 0.5) + 0.625) - 5.0 / 3.0) + 1.0
    rs = torch.where(r > 1.0, r, torch.ones_like(r))
    g2 = rs * (rs * (rs * (rs * (rs / 12.0 - 0.5) + 0.625) + 5.0 / 3.0) - 5.0) + 4.0 - 2.0 / (3.0 * rs)
    g = torch.where(r <= 1.0, g1, g2).clamp_min(0.0)
    return torch.where(r >= 2.0, torch.zeros_like(g), g)


def distances(centers: torch.Tensor, p: torch.Tensor, radius: float) -> torch.Tensor:
    """[cells, K] great-circle distances R atan2(|c x p|, c . p)."""
    c, q = centers[:, None, :], p[None, :, :]
    cr = torch.linalg.cross(c.expand(-1, q.shape[1], -1), q.expand(c.shape[0], -1, -1))
    return radius * torch.atan2(torch.sqrt((cr[..., 0] ** 2 + cr[..., 1] ** 2) + cr[..., 2] ** 2),
                                (c[..., 0] * q[..., 0] + c[..., 1] * q[..., 1]) + c[..., 2] * q[..., 2])


def weights(centers: torch.Tensor, p: torch.Tensor, sigma: torch.Tensor, radius: float,
            localisation: Optional[float]) -> torch.Tensor:
    """w [cells, K] = g / sigma^2."""
    inv = 1.0 / (sigma * sigma)
    if localisation is None:
        return inv[None, :].expand(centers.shape[0], -1)
    g = gaspari_cohn(distances(centers, p, radius) / float(localisation))
    return g / (sigma * sigma)[None, :]


def obs_space(Y: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(ybar [K], Yp [M, K], d [K]) of Y [M, K]; the mean adds the members in ascending order."""
    s = Y[0].clone()
    for m in range(1, Y.shape[0]):
        s = s + Y[m]
    ybar = s / Y.shape[0]
    return ybar, Y - ybar, y - ybar


def innovation_rms(Y: torch.Tensor, y: torch.Tensor, sigma: torch.Tensor) -> float:
    """RMS over the observations of (y - ybar) / sigma."""
    _, _, d = obs_space(Y, y)
    return float(torch.sqrt(((d / sigma) ** 2).mean()))


def _eigh(A: torch.Tensor, solver: str):
    if solver == "numpy":
        lam, Q = np.linalg.eigh(A.detach().cpu().numpy())
        return torch.as_tensor(lam, device=A.device), torch.as_tensor(Q, device=A.device)
    return torch.linalg.eigh(A)


def analysis(X: torch.Tensor, Y: torch.Tensor, y: torch.Tensor, sigma: torch.Tensor, centers: torch.Tensor,
             p: torch.Tensor, radius: float, localisation: Optional[float] = None, inflation: float = 1.0,
             eigh: str = "torch") -> Tuple[torch.Tensor, int]:
    """(Xa [M, F, cells] float64, the most observations with w > 0 any cell saw).

    ``X`` [M, F, cells] (any float type, converted to float64), ``Y`` [M, K],
    ``y`` / ``sigma`` [K], ``centers`` [cells, 3], ``p`` [K, 3], all on one device.
    ``eigh``: 'torch' or 'numpy' (the symmetric eigen-solver; the result does
    not depend on it beyond rounding, Wa being the unique symmetric root)."""
    X = X.to(torch.float64)
    M, F, cells = X.shape
    K = Y.shape[1]
    _, Yp, d = obs_space(Y.to(torch.float64), y)
    cdiag = float(M - 1) / float(inflation)
    eye = torch.eye(M, dtype=torch.float64, device=X.device)
    s = X[0].clone()
    for m in range(1, M):
        s = s + X[m]
    xbar = s / M                                                  # [F, cells]
    Xp = X - xbar
    Xa = torch.empty_like(X)
    nmax = 0
    step = max(1, min(cells, (1 << 24) // max(1, M * K)))
    for i0 in range(0, cells, step):
        sl = slice(i0, min(cells, i0 + step))
        w = weights(centers[sl], p, sigma, radius, localisation)  # [c, K]
        nmax = max(nmax, int((w > 0).sum(1).max()))
        Yw = Yp[None, :, :] * w[:, None, :]                       # [c, M, K]
        A = cdiag * eye + Yw @ Yp.T
        rhs = Yp @ (w * d).T                                      # [M, c]
        lam, Q = _eigh(A, eigh)
        z = torch.einsum("cnj,nc->cj", Q, rhs) / lam
        wbar = torch.einsum("cnj,cj->cn", Q, z)
        Wa = (Q * torch.sqrt(float(M - 1) / lam)[:, None, :]) @ Q.transpose(1, 2)
        T = wbar[:, :, None] + Wa                                 # [c, n, m]
        Xa[:, :, sl] = xbar[None, :, sl] + torch.einsum("nfc,cnm->mfc", Xp[:, :, sl], T)
    return Xa, nmax


def _host(a, dtype) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return torch.as_tensor(np.asarray(a, dtype=dtype))


def check_args(members: int, nfields: int, points, values, sigma, fields, localisation, inflation):
    """The observation arguments of ``Ensemble.assimilate`` as float64 / int64
    host tensors (p [K, 3], y [K], sigma [K], fields [K]); ``ValueError`` naming
    the argument otherwise."""
    if members < MIN_M:
        raise ValueError(f"members: an analysis needs at least {MIN_M} members, got {members}")
    if members > MAX_M:
        raise ValueError(f"members: at most {MAX_M} members, got {members}")
    p = _host(points, np.float64)
    if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
        raise ValueError(f"points: [K, 3] unit vectors with K >= 1 expected, not {tuple(p.shape)}")
    K = p.shape[0]
    if K > MAX_K:
        raise ValueError(f"points: {K} observations exceed the limit {MAX_K}")
    if not bool(torch.isfinite(p).all()) or not bool(((p * p).sum(1) - 1.0).abs().max() < 1e-9):
        raise ValueError("points: finite unit vectors expected")
    y = _host(values, np.float64).reshape(-1)
    if y.shape[0] != K or not bool(torch.isfinite(y).all()):
        raise ValueError(f"values: [{K}] finite values expected, not {tuple(y.shape)}")
    sg = _host(sigma, np.float64)
    sg = sg.expand(K).clone() if sg.dim() == 0 else sg.reshape(-1)
    if sg.shape[0] != K:
        raise ValueError(f"sigma: a scalar or [{K}] expected, not {tuple(sg.shape)}")
    if not bool((sg > 0).all()) or not bool(torch.isfinite(sg).all()):
        raise ValueError("sigma: every observation error must be finite and > 0")
    fl = _host(fields, np.int64)
    fl = fl.expand(K).clone() if fl.dim() == 0 else fl.reshape(-1)
    if fl.shape[0] != K:
        raise ValueError(f"fields: one index or [{K}] expected, not {tuple(fl.shape)}")
    if not bool(((fl >= 0) & (fl < nfields)).all()):
        raise ValueError(f"fields: an index outside 0 .. {nfields - 1} of a state with {nfields} fields")
    if localisation is not None and not (math.isfinite(float(localisation)) and float(localisation) > 0.0):
        raise ValueError(f"localisation: a positive length in metres or None expected, not {localisation!r}")
    if not (math.isfinite(float(inflation)) and float(inflation) >= 1.0):
        raise ValueError(f"inflation: a factor >= 1 expected, not {inflation!r}")
    return p, y, sg, fl


def fibonacci_points(K: int) -> np.ndarray:
    """K quasi-uniform unit vectors [K, 3] (Fibonacci lattice)."""
    k = np.arange(int(K), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(K)
    lon = k * (math.pi * (3.0 - math.sqrt(5.0)))
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    p = np.stack([r * np.cos(lon), r * np.sin(lon), z], 1)
    return p / np.linalg.norm(p, axis=1, keepdims=True)
