"""The LETKF twin (models/letkf.py) and ``Ensemble.assimilate`` on the CPU."""
import numpy as np
import pytest
import torch

from stsphere.ensemble import Ensemble
from stsphere.models import letkf as ml
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.points import random_points
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout


def _ensemble(N, M, amplitude=1e-2, seed=0, mode="batched"):
    return Ensemble(lambda: ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), M, amplitude=amplitude, seed=seed,
                    grid=CubedSphereGrid(N), mode=mode)


def test_global_etkf_is_the_kalman_update():
    """C4, M = 12, K = 20 observations of h, no localisation, rho = 1: the analysis
    mean and sample covariance equal the dense Kalman update with P = Xp^T Xp / (M - 1)
    and H assembled by sampling unit states.  Tolerance: 10 x the discrepancy of two
    float64 evaluations of the dense formula that differ only in the linear solve
    (``solve`` against the explicit inverse), measured here."""
    M, K = 12, 20
    ens = _ensemble(4, M)
    e0 = ens.engines[0]
    F, cells = e0.physics.F, 6 * 16
    p, sigma = random_points(K, 3), 30.0
    truth = _ensemble(4, 2, seed=9).engines[1]
    y = ens.observe(truth, p, sigma, seed=1)
    X = ens.states().reshape(M, -1).clone()                       # [M, F cells]
    H = torch.zeros(K, F * cells, dtype=torch.float64)            # h only: the other fields' columns stay zero
    pt = torch.as_tensor(p)
    for c in range(cells):
        unit = torch.zeros(F, cells, dtype=torch.float64)
        unit[0, c] = 1.0
        e0.set_state(unit.reshape(F, 6, 4, 4))
        H[:, c] = e0.points().fields(pt)[0]
    e0.set_state(X[0].reshape(F, 6, 4, 4))
    xbar = X.mean(0)
    Xp = X - xbar
    P = Xp.T @ Xp / (M - 1)
    S = H @ P @ H.T + sigma ** 2 * torch.eye(K, dtype=torch.float64)
    G1 = torch.linalg.solve(S, H @ P).T
    G2 = P @ H.T @ torch.linalg.inv(S)
    d = y - H @ xbar
    mean = [xbar + G @ d for G in (G1, G2)]
    cov = [P - G @ H @ P for G in (G1, G2)]
    tol_mean = 10.0 * float((mean[0] - mean[1]).abs().max())
    tol_cov = 10.0 * float((cov[0] - cov[1]).abs().max())
    Xa = ens.assimilate(p, y, sigma)["analysis"].reshape(M, -1)
    am = Xa.mean(0)
    ac = (Xa - am).T @ (Xa - am) / (M - 1)
    em, ec = float((am - mean[0]).abs().max()), float((ac - cov[0]).abs().max())
    print(f"mean: {em:.3e} (tol {tol_mean:.3e}); covariance: {ec:.3e} (tol {tol_cov:.3e})")
    assert em <= tol_mean and ec <= tol_cov


def test_localisation():
    g = ml.gaspari_cohn(torch.tensor([0.0, 2.0, 1.0, 1.0 + 1e-12, 2.5], dtype=torch.float64))
    assert g[0] == 1.0 and g[1] == 0.0 and g[4] == 0.0 and abs(float(g[2] - g[3])) < 1e-11
    ens = _ensemble(8, 6)
    X = ens.states().clone()
    p = np.array([[0.0, 0.0, 1.0]])
    Lc = 1.0e6
    rec = ens.assimilate(p, [5000.0], 10.0, localisation=Lc)
    ctr = torch.as_tensor(ens.engines[0].geo.center)                              # [T, n, n, 3]
    far = ml.distances(ctr.reshape(-1, 3), torch.as_tensor(p), ens.grid.radius).reshape(6, 8, 8) > 2.0 * Lc
    assert bool(far.any()) and not bool(far.all()) and rec["nobs_max"] == 1
    diff = (rec["analysis"] - X).abs()[:, :, far]
    assert float(diff.max()) <= 4.0 * float(np.spacing(float(X.abs().max())))
    assert float((rec["analysis"] - X).abs()[:, 0][:, ~far].max()) > 1.0


def test_identical_twin_run():
    """C8 TC5, M = 8, 60 observations of h (sigma 10 m) every 4 steps for 40 steps,
    Lc = 3000 km, rho = 1.05; members perturbed with amplitude 1e-2, the truth a
    member of another seed.  Measured: RMSE of the ensemble-mean height 3.83 m with
    assimilation against 5.72 m without."""
    truth = _ensemble(8, 2, seed=5).engines[1]
    ens, free = _ensemble(8, 8), _ensemble(8, 8)
    p = ml.fibonacci_points(60)
    for k in range(10):
        for x in (ens, free):
            x.run(4)
        truth.step(4)
        ens.assimilate(p, ens.observe(truth, p, 10.0, seed=k), 10.0, localisation=3.0e6, inflation=1.05)
    h = truth.tiles_view()[0]
    rmse = [float(((x.states()[:, 0].mean(0) - h) ** 2).mean().sqrt()) for x in (ens, free)]
    print(f"height RMSE of the ensemble mean: {rmse[0]:.3f} m with assimilation, {rmse[1]:.3f} m without")
    assert rmse[0] < rmse[1]


P1 = random_points(3, 0)


@pytest.mark.parametrize("kw, name", [
    (dict(points=P1[:, :2]), "points"), (dict(values=[1.0, 2.0]), "values"), (dict(sigma=[1.0, 0.0, 1.0]), "sigma"),
    (dict(sigma=[1.0, 1.0]), "sigma"), (dict(inflation=0.9), "inflation"), (dict(fields=4), "fields"),
    (dict(fields=[0, 1]), "fields"), (dict(localisation=-1.0), "localisation"), (dict(members=1), "members"),
])
def test_refusals(kw, name):
    ens = _ensemble(4, kw.pop("members", 3), mode="streams")
    args = dict(points=P1, values=[1.0, 2.0, 3.0], sigma=1.0)
    args.update(kw)
    with pytest.raises(ValueError, match=name):
        ens.assimilate(**args)
