"""Three and more stacked layers on the CPU twin: the cases of
``initial_conditions.stacked_fields`` (the L x L Montgomery solve of ``tc2``,
``tc5``), their convergence, and the config plumbing."""
import functools

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine
from stsphere.models import initial_conditions as ic
from stsphere.models.geometry import DAY, CubedSphereGrid
from stsphere.models.swe import LayeredShallowWater
from stsphere.parallel.layout import TileLayout

DEPTHS3, WINDS3 = [4000.0, 4000.0, 4000.0], [0.5, 0.4, 0.3]


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _three(case="tc2", **kw):
    if case == "tc2":
        kw.setdefault("winds", WINDS3)
    return LayeredShallowWater(case, depths=DEPTHS3, density_ratio=0.9, limiter=2, **kw)


@pytest.mark.parametrize("case,depths", [("tc2", [4000.0, 4000.0]), ("tc5", [2000.0, 5960.0]), ("rest", [1000.0, 1000.0])])
def test_general_solve_for_two_layers_is_the_two_layer_state(case, depths):
    p = _grid(12).centers()
    kw = {"winds": [0.5, 0.4]} if case == "tc2" else {}
    two = ic.layered_fields(case, p, depths, 0.9, **kw)
    gen = ic.stacked_fields(case, p, depths, 0.9, **kw)
    for a, b in zip(two, gen):
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(a).max(), 1e-300)
    A = [3.0, 2.0]
    assert np.allclose(ic.montgomery_drops(A, 0.9)[0], (A[0] - A[1]) / (1 - 0.9), rtol=1e-13)


@pytest.mark.parametrize("case", ["tc2", "tc5"])
def test_three_layer_states_are_positive(case):
    ph = _three(case)
    h, wind, b = ph.global_fields(_grid(12))
    assert h.shape == (3, 6, 12, 12) and wind.shape == (3, 6, 12, 12, 3) and h.min() > 0
    if case == "tc2":
        assert np.array_equal(ph.exact(_grid(12), 3600.0), h)
    else:       # flat upper layers over the mountain
        assert np.all(h[:2] == 4000.0) and b.max() > 0


@functools.lru_cache(maxsize=None)
def _steady_day(N):
    """One day of the steady three-layer state: the layers' l2 depth errors."""
    e = Engine(_three("tc2"), TileLayout(N, 1, 1, ng=2), grid=_grid(N), dtype=torch.float64, device="cpu",
               backend="torch")
    A = e.tens["area"]
    v0 = e.tiles_view().clone()
    e.step(int(np.ceil(DAY / e.dt)))
    v = e.tiles_view()
    return [float(((((v[4 * k] - v0[4 * k]) ** 2) * A).sum() / ((v0[4 * k] ** 2) * A).sum()).sqrt()) for k in range(3)]


def test_three_layer_steady_state_converges():
    """Combined l2 error (root of the summed squares) falls by at least 4 from
    C16 to C32, the two-layer test's condition, and no layer by less than 2.5."""
    c, f = _steady_day(16), _steady_day(32)
    ratios = [c[k] / f[k] for k in range(3)]
    comb = float(np.sqrt(sum(x * x for x in c)) / np.sqrt(sum(x * x for x in f)))
    print(f"l2 depth error C16 {c}, C32 {f}: ratios {['%.2f' % r for r in ratios]}, combined {comb:.2f}")
    assert comb >= 4.0
    assert min(ratios) >= 2.5


def _cfg(depths, case="tc2", winds=None):
    layers = {"depths": depths, "density_ratio": 0.9}
    if winds is not None:
        layers["winds"] = winds
    return {"parallelization": {"tiles_per_edge": 1, "num_devices": 1, "device_type": "cpu"},
            "grid": {"N": 12}, "physics": {"model": "swe", "case": case, "limiter": "mc", "layers": layers},
            "time": {"nsteps": 2, "dt": 400.0}, "io": {"output_dir": "unused"}}


def test_config_plumbing():
    s = S.Solver(_cfg(DEPTHS3, winds=WINDS3), verbose=False)
    s.initialize()
    assert s.engines[0].physics.nl == 3 and s.engines[0].physics.F == 12 and s.layers() == 3
    s.close()
    for cfg, msg in ((_cfg([1000.0] * 9, "rest"), "2 to 8 layers"),
                     (_cfg(DEPTHS3, winds=[0.5, 0.4]), "one number per layer"),
                     (_cfg(DEPTHS3, "layered_jet"), "defined for two layers")):
        with pytest.raises(ValueError, match=msg):
            S.Solver(cfg, verbose=False).initialize()
