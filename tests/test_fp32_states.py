"""What the fp32 kernel tests of tests/test_fp32_kernels.py rely on, checked on
the CPU with the PyTorch backend alone (no kernel takes part):

* the bound ``max(4 x twin, 4 eps32)`` of ``fp32_twin_bound`` stays below the
  1e-4 of the fp32 state tests for every physics, limiter, state class and
  integrator the GPU tests run, so no new case is looser than the test it
  stands beside;
* that bound sees a relative error of 1e-4 in g in every field, one of 2e-5 in
  every momentum field and a wrong limiter (van Leer computed as MC) by more
  than 1000 x, all in the fp64 oracle, i.e. without any rounding to hide behind;
* the same 1e-4 error in g stays below 1e-4 on the carried state of three
  smooth tc5 steps, which is what the fp32 state tests measure;
* rounding ``plateau`` and ``zero_mom`` to fp32 keeps every exactly zero
  difference exact, so the fp32 kernels meet the same zero arms.

Every case prints what it measured."""
import pytest
import torch

import tracer_states
from rough_states import (FP32_CAP, branch_shares, engine_of, fp32_twin_bound, global_state, grid_of, increment_error,
                          install)
from stsphere.engine import Engine
from stsphere.models.swe import GRAVITY, ShallowWater
from stsphere.parallel.layout import TileLayout

MOMENTUM = (1, 2, 3)

# (kind, N, t, limiter, class, integrator, steps): the cases of tests/test_fp32_kernels.py at the
# shapes a CPU affords (the larger GPU shapes change the grid, not the arithmetic)
CASES = ([("tc5", 24, 2, lim, "rough", "ssprk3", 2) for lim in (0, 1, 2, 3, 4)]
         + [("tc5", 24, 2, lim, cls, "ssprk3", 2) for cls in ("plateau", "zero_mom") for lim in (1, 3, 4)]
         + [("tc5", 17, 1, 3, "rough", "ssprk3", 2)]
         + [("tc5", 16, 1, 2, "rough", integ, 1) for integ in ("euler", "rk4")]
         + [("adv", 24, 2, lim, "scalar", "ssprk3", 2) for lim in (1, 2, 3, 4)]
         + [("diff", 24, 2, 0, "scalar", "ssprk3", 2), ("topo", 24, 2, 3, "rough", "ssprk3", 2)])


def _fmt(xs):
    return " ".join(f"{x:.2e}" for x in xs)


@pytest.mark.parametrize("kind,N,t,lim,cls,integ,steps", CASES,
                         ids=[f"{k}-C{N}-t{t}-lim{lim}-{cls}-{integ}" for k, N, t, lim, cls, integ, _ in CASES])
def test_twin_bound_is_below_the_cap(kind, N, t, lim, cls, integ, steps):
    """Measured: 2.4e-6 to 3.6e-6 (h) and 6e-7 to 1.8e-6 (momentum) on ``rough``
    and ``plateau``, 8.2e-6 to 1.2e-5 on ``zero_mom`` (the largest, with PPM:
    its momentum increment is small), 2.7e-7 to 3.9e-7 for advection and
    diffusion."""
    r = fp32_twin_bound(kind, N, t, lim, cls, integ, steps, device="cpu")
    print(f"FP32 twin {kind} {cls} limiter {lim} C{N} t={t} {integ}: twin {_fmt(r.twin)} bound {_fmt(r.bound)}")
    assert all(0.0 < b <= FP32_CAP for b in r.bound), r.bound
    assert all(x > 0.0 for x in r.twin), r.twin          # the fp32 run is not the oracle over again


@pytest.mark.parametrize("nq,N,t,lim", [(nq, 16, 2, lim) for nq in (1, 2, 4) for lim in (0, 1, 2, 3)] + [(2, 17, 1, 2)])
def test_tracer_twin_bound_is_below_the_cap(nq, N, t, lim):
    r = tracer_states.fp32_twin_bound(nq, N, t, lim, "rough", "ssprk3", 1, device="cpu")
    print(f"FP32 twin tracers nq {nq} limiter {lim} C{N} t={t}: twin {_fmt(r.twin)} bound {_fmt(r.bound)}")
    assert len(r.bound) == 4 + nq and all(0.0 < b <= FP32_CAP for b in r.bound), r.bound
    assert all(x > 0.0 for x in r.twin), r.twin


# ---- what the bound sees ---------------------------------------------------------------------
def _oracle_with(lim, dt, g=GRAVITY, rough=True):
    """The fp64 oracle of C24 t=2 tc5 with another g, from the fp32-rounded
    ``rough`` state (``rough=False``: from the analytic start)."""
    e = Engine(ShallowWater("tc5", limiter=lim, g=g), TileLayout(24, 2, 1, ng=2), grid=grid_of(24), dt=dt)
    if rough:
        install(e, global_state("tc5", 24, "rough").float().double())
    return e


@pytest.mark.parametrize("lim", [1, 3])
def test_the_bound_sees_a_wrong_constant(lim):
    """g (1 + 1e-4): above the bound in every field (measured 3.9e-5, 2.6e-5,
    2.7e-5, 3.2e-5 against 1.1e-5 to 1.3e-5 and 2.7e-6 to 3.7e-6);
    g (1 + 2e-5): above it in every momentum field (5.2e-6 to 6.3e-6)."""
    r = fp32_twin_bound("tc5", 24, 2, lim, "rough", "ssprk3", 2, device="cpu")
    for rel, fields in ((1e-4, (0, 1, 2, 3)), (2e-5, MOMENTUM)):
        bad = _oracle_with(lim, r.ref.dt, g=GRAVITY * (1.0 + rel))
        bad.step(2)
        errs = increment_error(r.ref, bad, r.q0)
        print(f"FP32 mutation limiter {lim} g (1 + {rel:g}): {_fmt(errs)} bound {_fmt(r.bound)}")
        for f in fields:
            assert errs[f] > r.bound[f], (rel, f, errs, r.bound)


def test_the_bound_sees_a_wrong_limiter():
    """Van Leer computed as MC: more than 1000 x the bound in every field
    (measured 5.1e-2, 2.7e-2, 3.6e-2, 2.5e-2)."""
    r = fp32_twin_bound("tc5", 24, 2, 3, "rough", "ssprk3", 2, device="cpu")
    bad = _oracle_with(2, r.ref.dt)
    bad.step(2)
    errs = increment_error(r.ref, bad, r.q0)
    print(f"FP32 mutation van Leer computed as MC: {_fmt(errs)} bound {_fmt(r.bound)}")
    for f in range(4):
        assert errs[f] > 1000.0 * r.bound[f], (f, errs, r.bound)


def test_the_state_metric_on_smooth_tc5_does_not_see_a_wrong_constant():
    """The measurement of the fp32 state tests (analytic tc5, three steps,
    max |a - b| / max |a| per field on the carried state): g (1 + 1e-4) in the
    fp64 oracle stays below their 1e-4 in every field (measured 1.6e-5,
    1.2e-5, 6.8e-6, 9.96e-5), so they could not see it."""
    good = _oracle_with(3, None, rough=False)
    bad = _oracle_with(3, good.dt, g=GRAVITY * (1.0 + 1e-4), rough=False)
    good.step(3)
    bad.step(3)
    a, b = good.tiles_view().reshape(4, -1), bad.tiles_view().reshape(4, -1)
    errs = ((a - b).abs().amax(1) / a.abs().amax(1)).tolist()
    print(f"FP32 smooth tc5, state metric, g (1 + 1e-4): {_fmt(errs)}")
    assert 0.0 < min(errs) and max(errs) < FP32_CAP, errs


# ---- exact zeros survive the rounding ------------------------------------------------------------
@pytest.mark.parametrize("cls,fields", [("plateau", (0, 1, 2, 3)), ("zero_mom", (1, 2, 3))])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64-engine", "fp32-engine"])
def test_rounding_keeps_exact_zero_differences(cls, fields, dtype):
    """``branch_shares`` of the state as built and of the fp32-rounded state
    (held by an fp64 engine, and by an fp32 engine as the kernels get it): the
    zero share of the class's fields is 1 before and after, and no field gains
    or loses a zero difference."""
    exact, _ = engine_of("tc5", 24, 2, 2, cls, device="cpu")
    rounded, _ = engine_of("tc5", 24, 2, 2, cls, dtype=dtype, rounded=True, device="cpu")
    a, b = branch_shares(exact), branch_shares(rounded)
    for ax in ("x", "y"):
        for f in range(4):
            assert a[ax][f]["zero"] == b[ax][f]["zero"], (ax, f, a[ax][f], b[ax][f])
        for f in fields:
            assert b[ax][f]["zero"] == 1.0, (ax, f, b[ax][f])
