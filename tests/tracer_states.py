"""Rough states for shallow water with tracers (a plain helper module on top
of ``rough_states``: ``from tracer_states import ...``).

The SWE part is the ``rough`` or ``plateau`` class of ``rough_states``; tracer
k is the mixing ratio

    q_k ~ U(0, 1) per cell, with one plateau patch per panel (a rectangle of
    a third of the panel in each direction, at a position that depends on k,
    held at 0, 1/2 or 1)

times the depth.  The rough winds (+-20 m/s on a ~20 m/s flow) give the depth
flux F_h both signs, so both upwind arms are taken; the noise takes the
opposite-sign and steep arms of every limiter, the patch the zero-difference
arm and, at its rim, a jump of up to 1.
"""
import functools

import torch

from rough_states import (Fp32Reference, _uniform, fp32_reference, global_of, grid_of, increment_error,   # noqa: F401
                          install, swe_state)
from stsphere.engine import Engine
from stsphere.models.swe import ShallowWaterTracers
from stsphere.parallel.layout import TileLayout

TRACER_SETS = {1: ["cap"], 2: ["cap", "cosine_bell"], 3: ["cap", "cosine_bell", "gradient"], 4: ["cap", "cosine_bell", "gradient", "constant"]}


def rough_mixing_ratios(nq: int, N: int, seed: int = 0) -> torch.Tensor:
    """[nq, 6, N, N] mixing ratios in [0, 1]."""
    gen = torch.Generator().manual_seed(4000 + seed)
    q = _uniform(gen, (nq, 6, N, N), 0.0, 1.0)
    w = max(2, N // 3)
    for k in range(nq):
        for f in range(6):
            j0 = (2 * f + 3 * k) % (N - w + 1)
            i0 = (5 * f + k) % (N - w + 1)
            q[k, f, j0:j0 + w, i0:i0 + w] = 0.5 * ((f + k) % 3)
    return q


def make_state(engines, cls: str, seed: int = 0) -> torch.Tensor:
    """Global state [4 + NQ, 6, N, N]: SWE class ``cls`` ("rough", "plateau")
    from the engines' current (initial) state, and rough tracers."""
    engines = list(engines) if isinstance(engines, (list, tuple)) else [engines]
    G0 = global_of(engines)
    swe = swe_state(G0[:4], engines[0].grid.centers(), cls, seed)
    q = rough_mixing_ratios(G0.shape[0] - 4, G0.shape[-1], seed)
    return torch.cat([swe, swe[0] * q])


# ---- the fp32 reference (rough_states.fp32_twin_bound for the tracer physics) ----
def tracer_physics(nq: int, lim: int):
    return ShallowWaterTracers("tc5", tracers=TRACER_SETS[nq], limiter=lim)


@functools.lru_cache(maxsize=None)
def global_state(nq: int, N: int, cls: str) -> torch.Tensor:
    """The global start state [4 + nq, 6, N, N] of a class: a function of the
    tracer count and the grid alone."""
    return make_state(Engine(tracer_physics(nq, 2), TileLayout(N, 1, 1, ng=2), grid=grid_of(N)), cls)


def engine_of(nq, N, t, lim, cls, backend="torch", dtype=torch.float64, integ="ssprk3", block=None, dt=None,
              rounded=False, device="cuda"):
    """(one-rank tracer engine with the class's state installed, q0)."""
    e = Engine(tracer_physics(nq, lim), TileLayout(N, t, 1, ng=2), grid=grid_of(N), dtype=dtype, device=device,
               backend=backend, integrator=integ, block=block, dt=dt)
    G = global_state(nq, N, cls)
    return e, install(e, G.float().double() if rounded else G)


@functools.lru_cache(maxsize=None)
def fp32_twin_bound(nq, N, t, lim=2, cls="rough", integ="ssprk3", steps=1, device="cuda") -> Fp32Reference:
    """(ref, q0, twin, bound) per field (h, M, hq_k) of one tracer case: see
    ``rough_states.fp32_twin_bound``."""
    return fp32_reference(lambda dtype, dt: engine_of(nq, N, t, lim, cls, dtype=dtype, integ=integ, dt=dt,
                                                      rounded=True, device=device), steps)
