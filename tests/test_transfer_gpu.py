"""The grid-transfer kernel (ops/csrc/transfer_kernel.hip) through
``Solver.set_from_cubed`` against the twin (models/transfer.py) on the same inputs.

fp64 metric: per row, max |kernel - twin| / max |twin increment|, the increment being
the fine value minus the coarse value of its parent (for a momentum triple the
largest of its three rows).  Bound: 10 x the same metric between two float64
evaluations of the twin that differ only in the order of its folds (ascending
against descending), measured on the CPU over the fp64 cases of this file: at most 5.64e-14 (the 3-layer
coarsening, whose depths of 4000 m stand against increments of 100 m).
fp32 state: within 2 float32 ulp of the twin's float64 result rounded once."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from rough_states import scalar_state, swe_state
from stsphere.driver import Solver
from stsphere.models import transfer as mt
from stsphere.models.geometry import CubedSphereGrid
from test_transfer import config

pytestmark = pytest.mark.gpu

REORDER_DISCREPANCY = 5.64e-14
TOL64 = 10.0 * REORDER_DISCREPANCY
PHYSICS = {"tc5": {"model": "swe", "case": "tc5"},
           "tracers": {"model": "swe", "case": "tc5", "tracers": ["constant", "cosine_bell"]},
           "layers3": {"model": "swe", "case": "tc2", "layers": {"depths": [4000.0] * 3, "density_ratio": 0.9, "winds": [0.5, 0.4, 0.3]}},
           "adv": {"model": "advection"}}
# (direction, r, coarse N, tiles per edge of the target): every ratio both ways, ragged 8 x 8 and
# 16 x 16 blocks, a one-cell stripe at the panel end (9, 17), tiles that cut a parent (N = 18, t = 2)
SHAPES = ([("refine", r, Ns, t) for r in mt.RATIOS for Ns in (4, 9, 17) for t in (1, 2)]
          + [("coarsen", r, N, 1) for r in mt.RATIOS for N in (4, 9, 17)] + [("coarsen", r, 8, 2) for r in mt.RATIOS])
VARIANTS = [("tc5", "float64", "smooth"), ("tc5", "float32", "rough"), ("tracers", "float32", "rough"),
            ("tracers", "float64", "smooth"), ("layers3", "float64", "rough"), ("adv", "float64", "rough")]


@functools.lru_cache(maxsize=None)
def source(model, N, cls):
    """Global float64 state [F, 6, N, N] of a model on C_N, chosen on the CPU: the
    case's own (smooth), or rough in every row (tracers: mixing ratios in plateaus)."""
    s = Solver(config(N, 1, PHYSICS[model]), verbose=False)
    s.initialize()
    G = torch.as_tensor(s.gather_global())
    if cls == "smooth":
        return G.numpy()
    if model == "adv":
        return scalar_state(G).numpy()
    ctr = CubedSphereGrid(N).centers()
    out = [swe_state(G[4 * k:4 * k + 4], ctr, "rough", seed=k) for k in range(len(G) // 4 if model == "layers3" else 1)]
    gen = torch.Generator().manual_seed(7)
    for _ in range(len(G) - 4 if model == "tracers" else 0):
        out.append((out[0][0] * torch.randint(0, 3, G[0].shape, generator=gen).double() / 2.0)[None])
    return torch.cat(out).numpy()


@functools.lru_cache(maxsize=None)
def twin(model, way, r, Nc, cls, limiter="bj"):
    """(twin result [F, 6, N, N], per-row increment scale, share of limited cells)."""
    Ns, N = (Nc, r * Nc) if way == "refine" else (r * Nc, Nc)
    src = source(model, Ns, cls)
    s = Solver(config(N, 1, PHYSICS[model]), verbose=False)
    s.initialize()
    tr = s.engines[0].transfer
    ref = tr.twin(torch.as_tensor(src), limiter).numpy()
    fine, coarse = (ref, src) if way == "refine" else (src, ref)
    inc = np.abs(fine - np.repeat(np.repeat(coarse, r, 2), r, 3)).reshape(len(ref), -1).max(1)
    f = 0
    while f < len(ref):
        if tr.kind[f] == 1:
            inc[f:f + 3] = inc[f:f + 3].max()
        f += 3 if tr.kind[f] == 1 else 1
    phi = torch.cat(tr._twins[Ns].phi) if way == "refine" else torch.zeros(1)
    return ref, inc, float(((phi > 0) & (phi < 1)).double().mean())


def gpu_solver(model, N, t, dtype, nd=None):
    c = config(N, t, PHYSICS[model], device="gpu", dtype=dtype)
    if nd is not None:
        c["parallelization"]["num_devices"] = nd
    s = Solver(c, verbose=False)
    s.initialize()
    return s


def check(model, dtype, cls, way, r, Nc, t):
    Ns, N = (Nc, r * Nc) if way == "refine" else (r * Nc, Nc)
    ref, inc, share = twin(model, way, r, Nc, cls)
    s = gpu_solver(model, N, t, dtype)
    s.set_from_cubed(source(model, Ns, cls))
    got = s.gather_global()
    if cls == "rough" and way == "refine":
        print(f"share of cells with 0 < phi < 1: {share:.3f}")
        assert share > 0
    if dtype == "float64":
        err = float((np.abs(got - ref).reshape(len(ref), -1).max(1) / inc).max())
        print(f"fp64 metric {err:.3e} (bound {TOL64:.1e})")
        assert err <= TOL64
    else:
        r32 = ref.astype(np.float32)
        assert (np.abs(got.astype(np.float32) - r32) <= 2 * np.spacing(np.abs(r32))).all()
    return s


@pytest.mark.parametrize("way,r,Nc,t", SHAPES)
def test_kernel_against_twin_shapes(way, r, Nc, t):
    check("tracers", "float64", "rough", way, r, Nc, t)


@pytest.mark.parametrize("way,r,Nc,t", [("refine", 4, 9, 1), ("refine", 8, 17, 2), ("coarsen", 8, 9, 1)])
@pytest.mark.parametrize("model,dtype,cls", VARIANTS)
def test_kernel_against_twin_models(model, dtype, cls, way, r, Nc, t):
    check(model, dtype, cls, way, r, Nc, t)


@pytest.mark.parametrize("way,r,Nc", [("refine", 4, 9), ("coarsen", 2, 18)])
def test_repeatable_rank_independent_and_ghosts(way, r, Nc):
    Ns, N = (Nc, r * Nc) if way == "refine" else (r * Nc, Nc)
    src = source("tracers", Ns, "rough")
    one = check("tracers", "float64", "rough", way, r, Nc, 1)
    first = one.gather_global()
    one.set_from_cubed(src)
    assert np.array_equal(first, one.gather_global())                  # two launches, the same bits
    four = gpu_solver("tracers", N, 2, "float64", nd=4)
    four.set_from_cubed(src)
    assert len(four.engines) == 4 and np.array_equal(first, four.gather_global())
    for e in four.engines:                                             # ghost slots as set_state leaves them
        after = e.state.clone()
        e.set_state(e.tiles_view().clone())
        assert torch.equal(e.state, after)


def test_launcher_validation():
    from stsphere.ops import native
    s = check("tracers", "float64", "smooth", "refine", 2, 4, 1)       # fills the descriptor
    op = s.engines[0].transfer
    assert op.lib.stsp_transfer_desc_size() == ctypes.sizeof(native.TransferDesc)
    for field, value, code in (("r", 3, 4), ("N", 9, 4), ("src", None, 1), ("F", 33, 1)):
        d = native.TransferDesc.from_buffer_copy(op.desc)
        setattr(d, field, value)
        assert op.lib.stsp_transfer_launch(1, d, None) == code, field
    for arr, f, value, code in (("kind", 0, 3, 5), ("kind", 2, 0, 5), ("depth", 1, 2, 5), ("depth", 4, 40, 6), ("depth", 1, -1, 6)):
        d = native.TransferDesc.from_buffer_copy(op.desc)
        getattr(d, arr)[f] = value
        assert op.lib.stsp_transfer_launch(1, d, None) == code, (arr, f)
    assert op.lib.stsp_transfer_launch(7, native.TransferDesc.from_buffer_copy(op.desc), None) == 2
