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
import torch

from rough_states import _uniform, global_of, increment_error, install, swe_state   # noqa: F401

TRACER_SETS = {1: ["cap"], 2: ["cap", "cosine_bell"], 4: ["cap", "cosine_bell", "gradient", "constant"]}


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
