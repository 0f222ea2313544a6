"""The EOF kernel (ops/csrc/eof_kernel.hip) against the twin (models/eof.py, on
the CPU in float64) on the snapshots of eof_snapshots.py, and through
``Ensemble.eofs`` on the batched padded state.

Deviation: ``values`` relative to values[0], ``fraction`` absolute, ``mean``
relative to its size, ``patterns`` absolute (unit area-weighted rms) and ``pcs``
relative to sqrt((S-1) values[0]), the last two per mode times min(1, gap_k /
lam_0), gap_k being the distance of lam_k to its neighbours (0 follows the last
mode of S-1).  Both sides diagonalise a Gram matrix that carries a rounding
error of eps lam_0, so mode k's vector is defined to eps lam_0 / gap_k only
(models/eof.py); the weight takes that conditioning out, and what is left is of
the order of eps for every mode.  The shapes with k = r = 47 and S = 48, 64 hold
noise modes (lam_k / lam_0 ~ 1e-12, gaps ~ 1e-13 lam_0) whose unweighted
patterns differ by 1e-3 between any two correct solvers; for the leading modes
(gap_k / lam_0 >= 1e-6) the weighted bound is an unweighted one below 1e-9.
Largest measured over CASES, the fp32 case and the batched state: values 1.53e-14
and fraction 1.17e-14 at N, S, k = 7, 48, 47; weighted patterns 2.33e-15 and pcs
4.75e-15 (unweighted there 1.5e-2 and 1.8e-9; at 6, 64, 8: 4.5e-13 and 4.1e-15);
mean 0 (profiles/eof/README.md).  TOL is 10 times the largest."""
import ctypes

import numpy as np
import pytest
import torch

from eof_snapshots import snapshots
from stsphere.engine import Engine, assemble_global
from stsphere.ensemble import Ensemble
from stsphere.models import eof as me
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

MEASURED = 1.53e-14
TOL = 10.0 * MEASURED
CASES = [(4, 3, 2), (5, 16, 8), (5, 17, 8), (7, 33, 16), (6, 64, 8), (7, 48, 47)]       # N, S, k = r


def deviation(got, ref, tail):
    """``got`` / ``ref``: dictionaries of CPU float64 tensors; ``tail``: the
    reference's eigenvalue after the last mode compared."""
    lam = torch.cat([ref["values"], tail.reshape(1)])
    S = ref["pcs"].shape[1]
    gap = torch.minimum(torch.cat([lam[:1] * 2, lam[:-2] - lam[1:-1]]), lam[:-1] - lam[1:]) / lam[0]
    wt = gap.clamp(max=1.0)
    k = len(wt)
    dp = (got["patterns"] - ref["patterns"]).reshape(k, -1).abs().amax(1)
    dc = (got["pcs"] - ref["pcs"]).abs().amax(1) / float(torch.sqrt((S - 1) * lam[0]))
    return {"values": float((got["values"] - ref["values"]).abs().max() / lam[0]),
            "fraction": float((got["fraction"] - ref["fraction"]).abs().max()),
            "mean": float((got["mean"] - ref["mean"]).abs().max() / ref["mean"].abs().max()),
            "patterns": float((wt * dp).max()), "pcs": float((wt * dc).max()),
            "patterns_unweighted": float(dp.max()), "pcs_unweighted": float(dc.max())}


def twin(x, area, k):
    """The twin's modes on the CPU and the eigenvalue that follows them."""
    S = x.shape[0]
    r = me.eofs(x.cpu().double(), area.cpu(), min(k + 1, S - 1))
    tail = r["values"][k] if k < S - 1 else torch.zeros((), dtype=torch.float64)
    return {n: (v[:k] if n in ("values", "fraction", "patterns", "pcs") else v) for n, v in r.items()}, tail


def contiguous_case(N, S, k, dtype=torch.float64):
    from stsphere.ops.eof import Eof
    e = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), device="cuda", backend="torch")
    xg, _ = snapshots(N, S, k)
    x = torch.as_tensor(np.ascontiguousarray(np.moveaxis(e.geo.gather_global(np.moveaxis(xg, 0, -1)), -1, 0)),
                        dtype=dtype, device="cuda")
    return Eof(e, S, k, padded=False), x, torch.as_tensor(e.geo.area)


def cpu(r):
    return {n: v.detach().cpu().clone() for n, v in r.items()}


def check(dev):
    print({n: f"{v:.2e}" for n, v in dev.items()})
    assert max(dev[n] for n in ("values", "fraction", "mean", "patterns", "pcs")) <= TOL


@pytest.mark.parametrize("N,S,k", CASES)
def test_kernel_against_twin(N, S, k):
    op, x, area = contiguous_case(N, S, k)
    got = cpu(op.compute(x))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    check(deviation(got, *twin(x, area, k)))
    again = cpu(op.compute(x))
    assert all(torch.equal(got[n], again[n]) for n in ("values", "patterns", "pcs"))


def test_fp32_snapshots():
    op, x, area = contiguous_case(5, 16, 8, torch.float32)
    check(deviation(cpu(op.compute(x)), *twin(x, area, 8)))


def test_batched_padded_state():
    """``Ensemble.eofs`` of both fields' kind (h and a momentum component), and the
    same from a copy of the batch whose ghost slots are all NaN."""
    cfg = {"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": "gpu"},
           "grid": {"N": 8, "halo": 2, "dtype": "float64"}, "physics": {"model": "swe", "case": "tc5"}}
    ens = Ensemble.from_config(cfg, 8, amplitude=1e-2, mode="batched")
    assert ens.native
    ens.run(3)
    e0 = ens.engines[0]
    lay, area = e0.layout, torch.as_tensor(ens.grid.areas())
    poisoned = torch.full_like(ens.batch[0], float("nan"))
    T, n, mg = e0.plan.T, e0.plan.n, e0.plan.ng
    view = lambda b: b.reshape(b.shape[0], b.shape[1], T, n + 2 * mg, n + 2 * mg)[..., mg:mg + n, mg:mg + n]
    view(poisoned).copy_(view(ens.batch[0]))
    for field in (0, 1):
        got = cpu(ens.eofs(field=field))
        glob = dict(got, patterns=torch.as_tensor(np.stack([assemble_global(lay, {0: p.numpy()})
                                                            for p in got["patterns"]])),
                    mean=torch.as_tensor(assemble_global(lay, {0: got["mean"].numpy()})))
        check(deviation(glob, *twin(torch.as_tensor(ens.global_fields(field)), area, 7)))
        other = cpu(ens._eofs.compute(poisoned, field))
        assert all(torch.equal(got[n], other[n]) for n in got)


def test_launcher_codes():
    from stsphere.ops.eof import EofDesc
    op, x, _ = contiguous_case(4, 3, 2)
    assert op.lib.stsp_eof_desc_size() == ctypes.sizeof(EofDesc)
    op.compute(x)                               # fills the descriptor
    for field, value, code in (("S", 65, 4), ("S", 1, 4), ("Spad", 32, 4), ("k", 3, 5), ("k", 0, 5), ("Kpad", 32, 5),
                               ("X", None, 1), ("mean", None, 1), ("cells", 0, 1), ("slabs", 3, 1)):
        d = EofDesc.from_buffer_copy(op.desc)
        setattr(d, field, value)
        assert op.lib.stsp_eof_launch(1, d, None) == code, field
    assert op.lib.stsp_eof_launch(7, op.desc, None) == 2
