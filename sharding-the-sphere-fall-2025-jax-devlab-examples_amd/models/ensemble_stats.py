"""Ensemble statistics of one field: definitions and the PyTorch twin of
``ops/csrc/ensemble_kernel.hip``.

For the members' values ``x_m`` (m = 0 .. M-1) of a cell, in float64 whatever
the state's type and with the members in ascending order,

    mean = ((x_0 + x_1) + ... + x_{M-1}) / M
    var  = (sum_m (x_m - mean)^2) / M

(the population variance, as ``Ensemble.spread`` uses it).  Every product and
sum rounds on its own: the squared deviation is formed, then added.  The kernel
is compiled without contraction, so its per-cell fields equal the twin's bit
for bit.  The four scalars (``SCALARS``) are sums of the cells' values weighted
by the cell area; the kernel adds them block by block in a fixed order, the
twin with ``torch.sum``, so those agree to rounding only.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

SCALARS = ("sum_area_mean", "sum_area_var", "sum_area", "max_var")


def cell_stats(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean, var) over the leading (member) axis of ``x`` [M, ...], float64."""
    x = x.to(torch.float64)
    M = x.shape[0]
    s = x[0].clone()
    for m in range(1, M):
        s = s + x[m]
    mean = s / M
    v = torch.zeros_like(mean)
    for m in range(M):
        d = x[m] - mean
        d2 = d * d
        v = v + d2
    return mean, v / M


def scalars(mean: torch.Tensor, var: torch.Tensor, area: torch.Tensor) -> torch.Tensor:
    """[4] float64 in ``SCALARS`` order."""
    A = area.to(torch.float64).reshape(mean.shape)
    return torch.stack([(A * mean).sum(), (A * var).sum(), A.sum(), var.max()])


def summary(mean: torch.Tensor, var: torch.Tensor, s) -> Dict[str, object]:
    """The dictionary ``Ensemble.stats`` returns, from the fields and the four
    scalars (host floats, ``SCALARS`` order)."""
    s0, s1, s2, s3 = (float(v) for v in s)
    return {"mean_field": mean, "var_field": var, "mean": s0 / s2, "spread_rms": (s1 / s2) ** 0.5, "max_var": s3}


def ensemble_stats(x: torch.Tensor, area: torch.Tensor) -> Dict[str, object]:
    """Twin of the kernel: ``x`` [M, T, n, n] member values of one field,
    ``area`` [T, n, n]."""
    mean, var = cell_stats(x)
    return summary(mean, var, scalars(mean, var, area).tolist())
