"""What the output-product wrappers (ops/derived.py, ops/latlon.py,
ops/points.py, ops/spectra.py) share on the host: the backend flag, and for
the last three the launch limit, the interior check of a padded index table
and the ascending-rank add."""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

MAX_K = (1 << 31) - 256           # k and the workgroup count stay in int


def use_hip(engine) -> bool:
    """The engine's products run the HIP kernels (else the PyTorch twin)."""
    return engine.backend == "hip" and engine.device.type == "cuda"


def assert_interior(plan, idx: np.ndarray) -> None:
    """The padded index table ``idx`` (any shape; -1: not this rank's)
    addresses interior cells only: a ghost slot is never a source."""
    P, g, n = plan.P, plan.ng, plan.n
    i = idx[idx >= 0].astype(np.int64) % (P * P)
    x, y = i % P, i // P
    assert bool(((x >= g) & (x < g + n) & (y >= g) & (y < g + n)).all())


def add_partials(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    """The ranks' arrays, given in ascending rank order, added in that order."""
    acc = parts[0]
    for p in parts[1:]:
        acc = acc + p
    return acc
