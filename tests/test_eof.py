"""The EOF twin (models/eof.py) against a plain numpy float64 reference, the
singular value decomposition of sqrt(a) x', on snapshots with a known answer
(eof_snapshots.py), and ``Ensemble.eofs`` on the CPU against the twin.

Deviation: ``values`` relative to values[0], ``fraction`` absolute, ``patterns``
absolute (they have unit area-weighted rms), ``pcs`` relative to
sqrt((S-1) values[0]), ``mean`` relative to its size.  Largest measured over
CASES: 1.73e-12 (the patterns at N, S, k = 5, 16, 8, whose last mode has
lam_k / lam_0 = 4^-7 and is resolved by the Gram matrix to eps lam_0 / gap_k =
5e-12; values 2.1e-15, fraction 5.6e-16, pcs 7.3e-15, mean 0); TOL is 10 times
the largest."""
import numpy as np
import pytest
import torch

from eof_snapshots import snapshots
from stsphere.engine import assemble_global
from stsphere.ensemble import Ensemble
from stsphere.models import eof as me
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

MEASURED = 1.73e-12
TOL = 10.0 * MEASURED
CASES = [(4, 3, 2), (5, 16, 8), (5, 17, 8)]        # N, S, k = r


def reference(x, area, k):
    S = x.shape[0]
    a = (area / area.sum()).reshape(-1)
    mean = x.mean(0)
    U, s, Vt = np.linalg.svd(np.sqrt(a) * (x - mean).reshape(S, -1), full_matrices=False)
    sg = np.sign(U[np.abs(U).argmax(0), np.arange(S)])
    lam = s ** 2 / (S - 1)
    return {"values": lam[:k], "fraction": lam[:k] / lam.sum(), "patterns": ((Vt.T * sg).T / np.sqrt(a))[:k],
            "pcs": (U * sg * s).T[:k], "mean": mean.reshape(-1)}


def deviation(got, ref, S):
    g = {n: np.asarray(got[n].detach().cpu() if isinstance(got[n], torch.Tensor) else got[n], dtype=np.float64)
         for n in ref}
    scale = {"values": ref["values"][0], "fraction": 1.0, "patterns": 1.0, "pcs": np.sqrt((S - 1) * ref["values"][0]),
             "mean": np.abs(ref["mean"]).max()}
    return {n: float(np.abs(g[n].reshape(ref[n].shape) - ref[n]).max() / scale[n]) for n in ref}


@pytest.mark.parametrize("N,S,k", CASES)
def test_twin_against_svd(N, S, k):
    x, area = snapshots(N, S, k)
    got = me.eofs(torch.as_tensor(x), torch.as_tensor(area), k)
    dev = deviation(got, reference(x, area, k), S)
    print(dev)
    assert max(dev.values()) <= TOL
    a = torch.as_tensor(area / area.sum())
    e = got["patterns"]
    assert float(((e[:, None] * e[None] * a).sum(dim=(2, 3, 4)) - torch.eye(k)).abs().max()) <= TOL
    j = got["pcs"].abs().argmax(1)
    assert bool((got["pcs"][torch.arange(k), j] > 0).all())
    full = me.eofs(torch.as_tensor(x), torch.as_tensor(area), S - 1)
    rec = torch.einsum("ks,k...->s...", full["pcs"], full["patterns"])
    # all S-1 modes include the noise modes (lam ~ 1e-12 / (S-1)): the Gram matrix carries an
    # error of S eps lam_0, a mode's pattern one of S eps lam_0 / lam_k, and its share of the
    # reconstruction sqrt((S-1) lam_k) times that, S eps / 1e-6 for the smallest lam_k
    assert float((rec - (torch.as_tensor(x) - full["mean"])).abs().max()) <= S * me.EPS / 1e-6


def test_zero_mode_rule():
    x, area = snapshots(4, 3, 2)
    x[1] = x[0]
    got = me.eofs(torch.as_tensor(x), torch.as_tensor(area), 2)
    assert float(got["values"][0]) > 0 and float(got["values"][1].abs()) <= 3 * me.EPS * float(got["total"])
    assert float(got["patterns"][1].abs().max()) == 0.0 and float(got["pcs"][1].abs().max()) == 0.0
    assert bool(torch.isfinite(got["patterns"]).all())


@pytest.mark.parametrize("S,k", [(1, None), (65, None), (3, 0), (3, 3), (3, 1.5)])
def test_value_errors(S, k):
    area = torch.ones(6, 2, 2)
    with pytest.raises(ValueError, match="^eof:"):
        me.eofs(torch.zeros(S, 6, 2, 2), area, k)
    with pytest.raises(ValueError, match="^eof:"):
        me.eofs(torch.zeros(3, 6, 2, 2), torch.ones(6, 2, 3), 1)


@pytest.mark.parametrize("mode", ["batched", "streams"])
def test_ensemble_eofs_cpu(mode):
    N, M = 8, 4
    ens = Ensemble(lambda: ShallowWater("tc5"), TileLayout(N, 2, 1, ng=2), M, amplitude=1e-2, grid=CubedSphereGrid(N),
                   mode=mode)
    ens.run(2)
    got = ens.eofs(field=0)
    assert got["patterns"].shape == (3, 24, 4, 4) and got["pcs"].shape == (3, M)
    ref = me.eofs(torch.as_tensor(ens.global_fields(0)), torch.as_tensor(ens.grid.areas()), 3)
    ref = {n: ref[n].numpy() for n in ("values", "fraction", "patterns", "pcs", "mean")}
    lay = ens.engines[0].layout
    got = dict(got, patterns=np.stack([assemble_global(lay, {0: p.numpy()}) for p in got["patterns"]]),
               mean=assemble_global(lay, {0: got["mean"].numpy()}))
    dev = deviation(got, ref, M)
    print(dev)
    assert max(dev.values()) <= TOL
    with pytest.raises(ValueError, match="^eof:"):
        ens.eofs(field=0, k=M)
