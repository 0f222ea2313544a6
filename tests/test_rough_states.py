"""The rough test states (tests/rough_states.py) do what the GPU tests of
tests/test_rough_kernels.py rely on, checked on the CPU with the fp64 oracle:
they reach every limiter arm, the oracle stays valid on them for the steps
the GPU tests take, two fp64 renderings of one step agree on them at the
rounding floor of the increment metric, and a wrong limiter arm in the oracle
shows in that metric on them (and not on the analytic case)."""
import functools

import pytest
import torch

import stsphere.models.base as base
from rough_states import (SWE_CLASSES, _primitive_window, branch_shares, grid_of, increment_error, install,
                          make_state)
from stsphere.engine import Engine
from stsphere.models.advection import Advection
from stsphere.models.diffusion import Diffusion
from stsphere.models.swe import ShallowWater
from stsphere.ops.fused import FusedPlan, FusedTorch
from stsphere.parallel.layout import TileLayout


def _engine(phys, N, t, dt=None):
    return Engine(phys, TileLayout(N, t, 1, ng=phys.halo), grid=grid_of(N), dt=dt)


@functools.lru_cache(maxsize=None)
def _swe_global(N, case, cls):
    """The global state of a class (it does not depend on the limiter or the
    layout), built once."""
    return make_state(_engine(ShallowWater(case), N, 1), cls)


def _swe(N, t, case, lim, cls, dt=None):
    e = _engine(ShallowWater(case, limiter=lim), N, t, dt)
    q0 = install(e, _swe_global(N, case, cls))
    return e, q0


@pytest.mark.parametrize("lim", [2, 4])
def test_rough_reaches_every_slope_arm_and_both_rusanov_sides(lim):
    """C24 t=2 tc5: every primitive field, in x and in y, has at least 10 % of
    its cells with opposite signs, 10 % with the steep bound active and 10 %
    on the central slope (measured 39-66 %, 16-19 %, 17-44 %); sL > sR and
    sR > sL each hold on at least 25 % of the edges.  With the PPM window
    (ng = 3) every arm of the monotonicity limiter is reached as well."""
    e, _ = _swe(24, 2, "tc5", lim, "rough")
    sh = branch_shares(e, lim)
    print(sh)
    for ax in ("x", "y"):
        for f in range(4):
            for k in ("opposite", "steep", "central"):
                assert sh[ax][f][k] >= 0.10, (ax, f, k, sh[ax][f])
            if lim == 4:
                for k in ("ppm_flat", "ppm_over_l", "ppm_over_r", "ppm_keep"):
                    assert sh[ax][f][k] > 0.0, (ax, f, k, sh[ax][f])
    for k, v in sh["speed"].items():
        assert v >= 0.25, (k, v)


@pytest.mark.parametrize("cls,fields", [("plateau", (0, 1, 2, 3)), ("zero_mom", (1, 2, 3))])
def test_exact_zero_differences(cls, fields):
    """plateau: every cell of every field has an exactly zero difference on a
    side, in x and in y; zero_mom: every velocity difference is an exact zero
    (while the depth is the rough one)."""
    e, _ = _swe(24, 2, "tc5", 2, cls)
    sh = branch_shares(e)
    for ax in ("x", "y"):
        for f in fields:
            assert sh[ax][f]["zero"] == 1.0, (ax, f, sh[ax][f])
    if cls == "zero_mom":
        assert sh["x"][0]["opposite"] >= 0.10 and sh["y"][0]["opposite"] >= 0.10


@pytest.mark.parametrize("lim", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("cls", SWE_CLASSES)
def test_oracle_stays_valid_on_the_states(cls, lim):
    """After the two steps the GPU tests take the oracle state is finite and
    min h >= 0.9 min h0 (measured 0.93-1.03)."""
    e, q0 = _swe(24, 2, "tc5", lim, cls)
    e.step(2)
    q = e.tiles_view()
    assert torch.isfinite(q).all()
    ratio = float(q[0].min() / q0[0].min())
    print(f"{cls} limiter {lim}: min h / min h0 = {ratio:.4f}")
    assert ratio >= 0.9


@pytest.mark.parametrize("phys", [lambda: Advection(limiter=1), lambda: Advection(limiter=2),
                                  lambda: Advection(limiter=3), lambda: Advection(limiter=4), lambda: Diffusion()],
                         ids=["adv1", "adv2", "adv3", "adv4", "diff"])
def test_scalar_class_stays_finite(phys):
    e = _engine(phys(), 24, 2)
    G = make_state(e, "scalar")
    q0 = install(e, G)
    assert 0.25 <= float((q0 == 0).double().mean()) <= 0.35 and float(q0.min()) == 0.0
    e.step(2)
    assert torch.isfinite(e.tiles_view()).all()
    assert not torch.equal(e.tiles_view(), q0)


@pytest.mark.parametrize("N,t,B,case,lim", [(24, 2, 4, "tc5", 2), (12, 1, 4, "tc2", 1)])
def test_floor_of_the_increment_metric(N, t, B, case, lim):
    """Engine.step against FusedTorch (two fp64 renderings of the same
    algorithm) for one step on ``rough``: below 1e-13 of the increment
    (measured <= 6.6e-15), three orders under the 1e-11 the kernels get."""
    ref, q0 = _swe(N, t, case, lim, "rough")
    fe, _ = _swe(N, t, case, lim, "rough", dt=ref.dt)
    ft = FusedTorch(fe, FusedPlan(fe.layout, 0, fe.grid, B=B, ns=3))
    ref.step(1)
    ft.step()
    errs = increment_error(ref, fe, q0)
    inc = [(ref.tiles_view()[f] - q0[f]).abs().max().item() / q0[f].abs().max().item() for f in range(4)]
    print(f"C{N} t={t} {case} limiter {lim}: increment errors {errs}; increment / state {inc}")
    assert max(errs) < 1e-13


# ---- a wrong limiter arm shows on a rough state, not on the analytic one ----------
_intact = base.limited_slope


def _mc_without_steep_bound(dl, dr, lim):
    if lim != 2:
        return _intact(dl, dr, lim)
    return torch.where(dl * dr > 0, 0.5 * (dl + dr), torch.zeros_like(dl))


def _minmod_magnitude_for_opposite_signs(dl, dr, lim):
    if lim == 0:
        return _intact(dl, dr, lim)
    return torch.where(dl * dr < 0, torch.sign(dl) * torch.minimum(dl.abs(), dr.abs()), _intact(dl, dr, lim))


@pytest.mark.parametrize("broken", [_mc_without_steep_bound, _minmod_magnitude_for_opposite_signs])
def test_a_wrong_limiter_arm_is_seen(monkeypatch, broken):
    """Mutation check of the metric: the oracle with one limiter arm broken
    (MC without its 2 min bound; the minmod magnitude instead of 0 for
    opposite signs) against the intact oracle, one MC step at C24 t=2.  On
    ``rough`` the increment error is above 1e-3 in every field (measured
    0.09-0.19 and 0.20-0.84); on the initial tc5 velocities the MC edit changes
    under 2 % of the slopes (measured 0.5 % in x, 1.5 % in y, raw panel-edge
    ghosts included), against 15-20 % on ``rough``."""
    good, q0 = _swe(24, 2, "tc5", 2, "rough")
    bad, _ = _swe(24, 2, "tc5", 2, "rough", dt=good.dt)
    good.step(1)
    monkeypatch.setattr(base, "limited_slope", broken)
    bad.step(1)
    errs = increment_error(good, bad, q0)
    print(f"{broken.__name__}: rough increment errors {errs}")
    assert min(errs) > 1e-3, errs
    if broken is _mc_without_steep_bound:
        smooth = _engine(ShallowWater("tc5"), 24, 2)
        g, n = 2, smooth.plan.n
        w = _primitive_window(smooth)[1:]
        changed = []
        for rows in (w[:, :, g:g + n, :], w.transpose(-1, -2)[:, :, g:g + n, :]):
            c = rows[..., g:g + n]
            dl, dr = c - rows[..., g - 1:g + n - 1], rows[..., g + 1:g + n + 1] - c
            changed.append(float((broken(dl, dr, 2) != _intact(dl, dr, 2)).double().mean()))
        print(f"initial tc5 velocities: share of slopes the edit changes, x and y: {changed}")
        assert max(changed) < 0.02
