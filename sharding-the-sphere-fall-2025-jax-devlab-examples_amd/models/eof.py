"""Snapshot (method-of-snapshots) EOFs: definitions and the PyTorch twin of
``ops/csrc/eof_kernel.hip``.

For snapshots ``x_s(i)`` (s = 0 .. S-1) over the cells i and the weights
``a_i = A_i / sum(A)`` of the exact cell areas, in float64 whatever the
snapshots' type:

    mean        xbar(i) = ((x_0 + x_1) + ... + x_{S-1}) / S,  x'_s = x_s - xbar
    covariance  C[s, t] = (1 / (S-1)) sum_i a_i x'_s(i) x'_t(i)        (S x S)
    eigenpairs  C = V diag(lam) V^T, lam descending; total = trace(C)
    sign        the component of v_k of largest magnitude (lowest index on a
                tie) is positive
    pattern     e_k(i) = sum_s v_k[s] x'_s(i) / sqrt((S-1) lam_k), so that
                sum_i a_i e_k e_l = delta_kl
    pc          pc_k[s] = sqrt((S-1) lam_k) v_k[s], so that x'_s = sum_k pc_k[s] e_k
    fraction    lam_k / total

``1 <= k <= S-1`` (the anomalies have rank at most S-1) and ``2 <= S <= MAX_S``.
A mode with ``lam_k <= S eps total`` has a zero pattern and zero principal
components; nothing is divided by it.

The Gram matrix squares the condition of the snapshot matrix: two correct
evaluations agree in mode k's pattern to about ``eps lam_0 / gap_k`` with
``gap_k`` the distance of ``lam_k`` to its neighbours, not to ``eps``.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

MAX_S = 64
EPS = 2.220446049250313e-16


def default_k(S: int) -> int:
    return min(int(S) - 1, 8)


def check_args(S: int, k: Optional[int]) -> int:
    """The number of modes for S snapshots; ``ValueError`` outside the limits."""
    S = int(S)
    if S < 2:
        raise ValueError(f"eof: at least 2 snapshots are needed, got {S}")
    if S > MAX_S:
        raise ValueError(f"eof: at most {MAX_S} snapshots are taken, got {S}")
    if k is None:
        return default_k(S)
    if int(k) != k or not 1 <= int(k) <= S - 1:
        raise ValueError(f"eof: k = {k!r} outside 1 .. S-1 = {S - 1}")
    return int(k)


def weights(area: torch.Tensor) -> torch.Tensor:
    """a_i = A_i / sum(A), float64, in the shape of ``area``."""
    A = area.to(torch.float64)
    return A / A.sum()


def anomalies(x: torch.Tensor):
    """(mean, x - mean) over the leading axis of ``x`` [S, ...], float64, the
    snapshots added in ascending order."""
    x = x.to(torch.float64)
    s = x[0].clone()
    for m in range(1, x.shape[0]):
        s = s + x[m]
    mean = s / x.shape[0]
    return mean, x - mean


def signed(V: torch.Tensor) -> torch.Tensor:
    """The columns of ``V`` with their component of largest magnitude positive
    (``argmax`` takes the lowest index on a tie)."""
    j = V.abs().argmax(dim=0)
    sg = torch.sign(V[j, torch.arange(V.shape[1], device=V.device)])
    return V * torch.where(sg == 0, torch.ones_like(sg), sg)


def eofs(x: torch.Tensor, area: torch.Tensor, k: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Twin of the kernel: ``x`` [S, ...] snapshots, ``area`` [...] cell areas.
    ``values`` [k], ``fraction`` [k], ``total``, ``patterns`` [k, ...],
    ``pcs`` [k, S] and ``mean`` [...], float64 on the device of ``x``."""
    if x.dim() < 2:
        raise ValueError(f"eof: snapshots [S, cells...] expected, got shape {tuple(x.shape)}")
    S = int(x.shape[0])
    k = check_args(S, k)
    if tuple(area.shape) != tuple(x.shape[1:]):
        raise ValueError(f"eof: areas of shape {tuple(area.shape)} for snapshots of shape {tuple(x.shape[1:])}")
    a = weights(area.to(x.device)).reshape(-1)
    mean, xp = anomalies(x)
    Z = xp.reshape(S, -1)
    Zw = Z * torch.sqrt(a)
    C = (Zw @ Zw.T) / (S - 1)
    C = 0.5 * (C + C.T)
    lam, V = torch.linalg.eigh(C)
    lam, V = torch.flip(lam, (0,))[:k], signed(torch.flip(V, (1,))[:, :k])
    total = torch.diagonal(C).sum()
    live = lam > S * EPS * total
    scale = torch.sqrt((S - 1) * torch.where(live, lam, torch.ones_like(lam)))
    U = torch.where(live, 1.0 / scale, torch.zeros_like(lam)) * V                # [S, k]
    pcs = (torch.where(live, scale, torch.zeros_like(lam)) * V).T.contiguous()   # [k, S]
    patterns = (U.T @ Z).reshape((k,) + tuple(x.shape[1:]))
    return {"values": lam, "fraction": lam / total, "total": total, "patterns": patterns, "pcs": pcs, "mean": mean}
