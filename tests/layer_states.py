"""Rough states for two-layer shallow water (a plain helper module on top of
``rough_states``: ``from layer_states import ...``).

Each layer is drawn as a shallow-water state of the ``rough`` or ``plateau``
class of ``rough_states`` from that layer's own initial state, with its own
seed: the layers are rough independently, so every slope arm and both signs of
the depth flux occur in each layer, and the coupling gradient sees an interface
that is as rough as the layers.
"""
import functools

import torch

from rough_states import global_of, grid_of, increment_error, install, swe_state   # noqa: F401
from stsphere.engine import Engine
from stsphere.models.swe import LayeredShallowWater
from stsphere.parallel.layout import TileLayout

DEPTHS = (2000.0, 5960.0)
RATIO = 0.9


def layer_physics(lim: int = 2, case: str = "tc5", **kw):
    """Two layers over the TC5 mountain (grad b != 0)."""
    kw.setdefault("depths", list(DEPTHS))
    kw.setdefault("density_ratio", RATIO)
    return LayeredShallowWater(case, limiter=lim, **kw)


def make_state(engines, cls: str, seed: int = 0) -> torch.Tensor:
    """Global state [8, 6, N, N]: layer k of class ``cls`` ("rough",
    "plateau") from the engines' current (initial) state, seed ``seed + 7 k``."""
    engines = list(engines) if isinstance(engines, (list, tuple)) else [engines]
    G0 = global_of(engines)
    centers = engines[0].grid.centers()
    return torch.cat([swe_state(G0[4 * k:4 * k + 4], centers, cls, seed + 7 * k) for k in range(G0.shape[0] // 4)])


@functools.lru_cache(maxsize=None)
def global_state(N: int, cls: str) -> torch.Tensor:
    """The global start state [8, 6, N, N] of a class: a function of the grid alone."""
    return make_state(Engine(layer_physics(2), TileLayout(N, 1, 1, ng=2), grid=grid_of(N)), cls)
