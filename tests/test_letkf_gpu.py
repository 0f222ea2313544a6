"""The LETKF kernel (ops/csrc/letkf_kernel.hip) through
``Ensemble(mode='batched', backend='hip').assimilate`` against the twin
(models/letkf.py) on the same inputs: the members' states and their samples Y
before the call.

fp64 metric: per field, max over cells and members of |kernel - twin| relative
to max |Xa - xbar|.  Bound: 10 x the same metric between the twin with
``numpy.linalg.eigh`` and the twin with ``torch.linalg.eigh`` on the CPU over
these cases (two reference evaluations that differ only in the eigen-solver, as
kernel and twin do; measured 2.7e-14, profiles/letkf/README.md); the margin is for
Jacobi and LAPACK distributing rounding differently.
fp32: the kernel's output equals the twin's float64 result on the same float32
inputs rounded to float32, within 2 float32 ulp of each value."""
import ctypes

import numpy as np
import pytest
import torch

from stsphere.engine import Engine
from stsphere.ensemble import Ensemble
from stsphere.models import letkf as ml
from stsphere.models.advection import Advection
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.points import random_points
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

EIGH_DISCREPANCY = 2.7e-14      # numpy against torch eigh in the twin, largest over CASES (CPU)
TOL64 = 10.0 * EIGH_DISCREPANCY
CHUNK = 64                      # staged observations of the kernel

# N, tiles per edge, M, K, placement, Lc (km; None: global), rho, dtype, physics, a field per observation
CASES = [
    (8, 1, 2, 1, "corner", None, 1.0, torch.float64, "swe", False),
    (8, 1, 5, 3, "corner", 3000.0, 1.1, torch.float64, "swe", False),
    (12, 2, 16, 5, "random", 2000.0, 1.05, torch.float64, "swe", True),
    (17, 1, 17, CHUNK + 1, "cluster", 2500.0, 1.0, torch.float64, "swe", False),
    (8, 1, 32, CHUNK + 1, "cluster", 3000.0, 1.02, torch.float64, "swe", True),
    (12, 2, 32, 40, "hemisphere", 1000.0, 1.05, torch.float64, "adv", False),
    (17, 1, 5, 300, "random", None, 1.0, torch.float64, "swe", True),
    (8, 1, 17, 140, "random", None, 1.0, torch.float64, "adv", False),
    (17, 1, 16, 40, "hemisphere", 1000.0, 1.0, torch.float64, "swe", False),
    (12, 2, 16, CHUNK + 1, "cluster", 2500.0, 1.05, torch.float32, "swe", True),
    (17, 1, 32, 5, "random", 3000.0, 1.0, torch.float32, "adv", False),
    (8, 1, 2, 3, "corner", None, 1.0, torch.float32, "swe", False),
]
IDS = [f"C{c[0]}t{c[1]}-M{c[2]}-K{c[3]}-{c[4]}-{'f64' if c[7] == torch.float64 else 'f32'}-{c[8]}" for c in CASES]


def _points(place, K):
    p = random_points(K, 11)
    if place == "corner":                      # a cube corner, then a panel edge
        p[0] = np.ones(3) / np.sqrt(3.0)
        if K > 1:
            p[1] = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    elif place == "cluster":                   # inside one localisation radius
        p = np.array([0.6, 0.64, 0.48]) + 0.05 * p
    elif place == "hemisphere":                # nothing within 2 Lc of the far side
        p[:, 2] = np.abs(p[:, 2]) + 1.0
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def build(case, device="cuda", backend="hip"):
    """The ensemble of a case after two steps (spread in every field) and its
    observation arguments (points, values, sigma, fields)."""
    N, t, M, K, place, Lc, rho, dtype, phys, per_obs = case
    factory = (lambda: ShallowWater("tc5")) if phys == "swe" else (lambda: Advection("cosine_bell"))
    ens = Ensemble(factory, TileLayout(N, t, 1, ng=2), M, amplitude=1e-2, grid=CubedSphereGrid(N), dtype=dtype,
                   device=device, backend=backend, mode="batched")
    ens.run(2)
    F = ens.engines[0].physics.F
    fields = np.arange(K) % F if per_obs else 0
    p = _points(place, K)
    dev = ens.engines[0].device
    fl = torch.as_tensor(fields * np.ones(K, dtype=np.int64), device=dev)
    Y = ens._sample_members(torch.as_tensor(p, device=dev), fl)
    scale = ens.states().abs().amax(dim=(0, 2, 3, 4)).double()[fl]
    sigma = torch.maximum(Y.std(0), 1e-3 * scale).cpu().numpy()      # comparable to the spread
    truth = Engine(factory(), ens.engines[0].layout, grid=ens.grid, dtype=dtype, device=device, backend=backend)
    y = ens.observe(truth, p, sigma, fields, seed=5)
    return ens, (p, y, sigma, fields)


def twin_of(ens, obs, case, eigh="torch"):
    """The twin's analysis [M, F, cells] (CPU, float64) of the ensemble's present state."""
    p, y, sigma, fields = obs
    F = ens.engines[0].physics.F
    pt, yt, st, ft = ml.check_args(ens.members, F, p, y.cpu(), sigma, fields, None, 1.0)
    Y = ens._sample_members(pt.to(ens.engines[0].device), ft.to(ens.engines[0].device)).cpu()
    X = ens.states().reshape(ens.members, F, -1).cpu().double()
    ctr = torch.as_tensor(ens.engines[0].geo.center).reshape(-1, 3)
    Lc = None if case[5] is None else 1e3 * case[5]
    Xa, nmax = ml.analysis(X, Y, yt, st, ctr, pt, float(ens.grid.radius), Lc, case[6], eigh=eigh)
    return X, Xa, nmax


def metric64(got, ref, X):
    xbar = X.mean(0, keepdim=True)
    return float(((got - ref).abs().amax(dim=(0, 2)) / (ref - xbar).abs().amax(dim=(0, 2))).max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_against_twin(case):
    ens, obs = build(case)
    X, ref, nmax = twin_of(ens, obs, case)
    Lc = None if case[5] is None else 1e3 * case[5]
    rec = ens.assimilate(*obs, localisation=Lc, inflation=case[6])
    got = rec["analysis"].reshape(X.shape).cpu()
    assert bool(torch.isfinite(got).all()) and rec["nobs_max"] == nmax
    if case[5] is not None and case[4] == "hemisphere":
        assert nmax < case[3]
    if case[7] == torch.float64:
        err = metric64(got, ref, X)
        print(f"fp64 metric {err:.3e} (bound {TOL64:.1e}), nobs_max {nmax}, rms {rec['rms_before']:.3f} -> "
              f"{rec['rms_after']:.3f}")
        assert err <= TOL64
    else:
        r32 = ref.float()
        ulp = (torch.nextafter(r32.abs(), torch.full_like(r32, float("inf"))) - r32.abs())
        err = float(((got - r32).abs() / ulp).max())
        print(f"fp32: {err:.2f} ulp, nobs_max {nmax}")
        assert err <= 2.0


def test_bitwise_reproducible():
    case = CASES[3]
    out = []
    for _ in range(2):
        ens, obs = build(case)
        out.append(ens.assimilate(*obs, localisation=1e3 * case[5], inflation=case[6])["analysis"].clone())
    assert torch.equal(out[0], out[1])


def test_ghost_slots_and_steps_after_analysis():
    """Every same-rank ghost slot equals its source after the call, and 4 batched
    steps after it equal 4 steps of fresh engines started from the analysed states."""
    case = CASES[2]
    ens, obs = build(case)
    ens.assimilate(*obs, localisation=1e3 * case[5], inflation=case[6])
    e0 = ens.engines[0]
    assert e0.halo_src.numel() > 0
    assert torch.equal(ens.batch[0][:, :, e0.halo_dst], ens.batch[0][:, :, e0.halo_src])
    start = [e.tiles_view().clone() for e in ens.engines]
    ens.run(4)
    torch.cuda.synchronize()
    for m in (0, ens.members - 1):
        e = Engine(ShallowWater("tc5"), e0.layout, grid=ens.grid, device="cuda", backend="hip", dt=ens.dt,
                   block=ens.block)
        e.set_state(start[m])
        e.step(4)
        assert torch.equal(e.tiles_view(), ens.engines[m].tiles_view())


def test_launcher_validation():
    from stsphere.ops.letkf import Letkf, LetkfDesc
    ens, obs = build(CASES[1])
    lk = Letkf(ens.engines[0], ens.members)
    assert lk.lib.stsp_letkf_desc_size() == ctypes.sizeof(LetkfDesc)
    ens.assimilate(*obs)                        # fills the descriptor of ens._letkf
    for field, value, code in (("M", 1, 4), ("M", 33, 4), ("Mpad", 32, 4), ("K", 0, 5), ("K", 65536, 5), ("rho", 0.5, 6)):
        d = LetkfDesc.from_buffer_copy(ens._letkf.desc)
        setattr(d, field, value)
        assert lk.lib.stsp_letkf_launch(1, d, None) == code, field
