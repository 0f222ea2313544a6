"""The topography of tests/rough_states.py (``TopographySWE``) does what the
GPU tests of tests/test_topography_kernels.py rely on, checked on the CPU with
the fp64 oracle: grad b is non-zero in every cell (the tc5 cone: under 5 % of
them, on one cube edge), the term -g h grad b is a visible part of the momentum
increment, the oracle stays valid over it, two fp64 renderings of a step agree
at the rounding floor, one reversed ghost strip of b on any panel-edge tile
side shows in the increment metric five orders above the kernels' bound, and
the host tables that carry grad b to the fused step (the cached global cell
records, the remote records of several ranks) follow the topography."""
import functools

import numpy as np
import pytest
import torch

from rough_states import (SWE_CLASSES, TopographySWE, global_of, gradb_with_reversed_ghost_strip, grid_of,
                          increment_error, install, make_state, topography)
from stsphere.engine import Engine, VirtualCluster, assemble_global
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.ops.fused import FusedExchangePlan, FusedPlan, FusedTorch, global_cell_records
from stsphere.parallel.layout import TileLayout
from stsphere.parallel.topology import LINKS

OTHER = (("g", 11.0), ("omega", 5e-5))         # the second set of constants of the GPU tests


def _engine(phys, N, t, dt=None, grid=None):
    return Engine(phys, TileLayout(N, t, 1, ng=phys.halo), grid=grid or grid_of(N), dt=dt)


@functools.lru_cache(maxsize=None)
def _global(N, cls, kw=()):
    """The global state of a class over the topography (it does not depend on
    the limiter or the layout), built once per set of constants."""
    return make_state(_engine(TopographySWE("tc5", **dict(kw)), N, 1), cls)


def _topo(N, t, lim, cls, dt=None, kw=(), grid=None):
    e = _engine(TopographySWE("tc5", limiter=lim, **dict(kw)), N, t, dt, grid)
    return e, install(e, _global(N, cls, kw))


def _gradb_global(e) -> np.ndarray:
    """[6, N, N] |grad b| of a one-rank engine."""
    mag = e.tens["gradb"].double().norm(dim=0).numpy()
    return assemble_global(e.layout, {0: mag})


def _edges_touched(mask: np.ndarray) -> int:
    """Number of the 12 cube edges with a marked cell in the row along them,
    on either side."""
    line = {"W": lambda m: m[:, 0], "E": lambda m: m[:, -1], "S": lambda m: m[0, :], "N": lambda m: m[-1, :]}
    touched = set()
    for (f, ed), lk in LINKS.items():
        if line[ed](mask[f]).any():
            touched.add(frozenset({(f, ed), (lk.nbr_face, lk.nbr_edge)}))
    return len(touched)


# ---- footprint -----------------------------------------------------------------
def test_topography_range():
    b = topography(grid_of(24))
    print(f"C24 b: {b.min():.1f} .. {b.max():.1f} m")
    assert 50.0 <= b.min() and b.max() <= 800.0


@pytest.mark.parametrize("N,t", [(24, 2), (48, 1)])
def test_gradient_in_every_cell(N, t):
    """grad b != 0 in 100 % of the cells, b != 0 on every tile, all 12 cube
    edges touched; for tc5 under 5 % of the cells (measured 3.1-3.5 %), 2 of 6
    panels and exactly one cube edge: why the class exists."""
    e = _engine(TopographySWE("tc5"), N, t)
    mag = _gradb_global(e)
    assert (mag > 0).all() and (e.tens["b"] != 0).all()
    assert _edges_touched(mag > 0) == 12
    # not a token gradient: the smallest is a visible share of the largest
    print(f"C{N} t={t}: min |grad b| / max |grad b| = {mag.min() / mag.max():.3e}")
    cone = _engine(ShallowWater("tc5"), N, t)
    mc = _gradb_global(cone)
    share = float((mc > 0).mean())
    panels = int((mc.reshape(6, -1) > 0).any(1).sum())
    print(f"C{N} t={t} tc5: grad b != 0 in {100 * share:.2f} % of the cells, {panels} panels, "
          f"{_edges_touched(mc > 0)} cube edge")
    assert 0 < share < 0.05 and panels == 2 and _edges_touched(mc > 0) == 1


def test_size_of_the_term():
    """On ``rough`` max(dt g h |grad b|) is at least 1 % of the largest
    momentum increment of a step (measured 12 %): an error in the term is
    far above the kernels' 1e-11."""
    e, q0 = _topo(24, 2, 2, "rough")
    term = e.dt * e.physics.g * q0[0] * e.tens["gradb"].double().norm(dim=0)
    e.step(1)
    inc = float((e.tiles_view()[1:4] - q0[1:4]).abs().max())
    print(f"max dt g h |grad b| = {float(term.max()):.3e} (median {float(term.median()):.3e}), "
          f"max momentum increment {inc:.3e}, ratio {float(term.max()) / inc:.3f}")
    assert float(term.max()) >= 0.01 * inc


# ---- the oracle stays valid ----------------------------------------------------
@pytest.mark.parametrize("lim", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("cls", SWE_CLASSES)
def test_oracle_stays_valid_over_the_topography(cls, lim):
    """After the two steps the GPU tests take the oracle state is finite and
    min h >= 0.9 min h0 (measured 1.01-1.02 for limiters 2 and 4 on rough)."""
    e, q0 = _topo(24, 2, lim, cls)
    e.step(2)
    q = e.tiles_view()
    assert torch.isfinite(q).all()
    ratio = float(q[0].min() / q0[0].min())
    print(f"{cls} limiter {lim}: min h / min h0 = {ratio:.4f}")
    assert ratio >= 0.9


@pytest.mark.parametrize("lim", [2, 4])
def test_oracle_stays_valid_with_other_constants(lim):
    """g = 11, omega = 5e-5 (measured 1.02).  (g = 3.7, omega = 2e-4 makes the
    tc5 depth negative and is not used.)"""
    e, q0 = _topo(24, 2, lim, "rough", kw=OTHER)
    assert e.physics.g == 11.0 and e.physics.omega == 5e-5 and float(q0[0].min()) > 0
    e.step(2)
    q = e.tiles_view()
    assert torch.isfinite(q).all()
    ratio = float(q[0].min() / q0[0].min())
    print(f"g = 11, omega = 5e-5, limiter {lim}: min h / min h0 = {ratio:.4f}")
    assert ratio >= 0.9


def test_oracle_stays_valid_for_the_four_step_launch():
    """C32 t=2, limiter 2, the four steps of the fused multi-step cases."""
    e, q0 = _topo(32, 2, 2, "rough")
    e.step(4)
    q = e.tiles_view()
    assert torch.isfinite(q).all()
    ratio = float(q[0].min() / q0[0].min())
    print(f"C32 t=2 four steps: min h / min h0 = {ratio:.4f}")
    assert ratio >= 0.9


def test_oracle_stays_valid_on_tc2_with_a_rotated_axis():
    """tc2 with alpha = pi / 4 over the topography, two steps."""
    mk = lambda: TopographySWE("tc2", alpha=np.pi / 4)
    e = _engine(mk(), 24, 2)
    q0 = install(e, make_state(_engine(mk(), 24, 1), "rough"))
    e.step(2)
    q = e.tiles_view()
    assert torch.isfinite(q).all()
    ratio = float(q[0].min() / q0[0].min())
    print(f"tc2 alpha = pi / 4: min h / min h0 = {ratio:.4f}")
    assert ratio >= 0.9


# ---- metric floor ----------------------------------------------------------------
def test_floor_of_the_increment_metric_over_the_topography():
    """Engine.step against FusedTorch for one step on ``rough``, C24 t=2 B=4:
    below 1e-13 of the increment (measured 6.6e-15)."""
    ref, q0 = _topo(24, 2, 2, "rough")
    fe, _ = _topo(24, 2, 2, "rough", dt=ref.dt)
    ft = FusedTorch(fe, FusedPlan(fe.layout, 0, fe.grid, B=4, ns=3))
    ref.step(1)
    ft.step()
    errs = increment_error(ref, fe, q0)
    print(f"C24 t=2 topography rough: increment errors {errs}")
    assert max(errs) < 1e-13


# ---- one reversed ghost strip of b shows ------------------------------------------
def test_a_reversed_ghost_strip_of_b_is_seen():
    """Mutation check: for each of the 48 panel-edge tile sides of C24 t=2 the
    layer-0 ghost strip of b read in reversed order changes grad b by at least
    1e-2 of max |grad b| (measured >= 0.24), and one MC step from ``rough``
    with that grad b has an increment error against the intact oracle above
    1e-6, five orders above the kernels' bound (measured >= 1.8e-2).  On the
    tc5 cone the same edit changes grad b on 4 of the 48 sides."""
    good, q0 = _topo(24, 2, 2, "rough")
    bad, _ = _topo(24, 2, 2, "rough", dt=good.dt)
    good.step(1)
    G = _global(24, "rough")
    b = topography(good.grid)
    intact = bad.tens["gradb"].clone()
    gmax = float(intact.norm(dim=0).max())
    cone = _engine(ShallowWater("tc5"), 24, 2)
    bc = cone.physics.global_fields(cone.grid)[2]
    sides = [(t, s) for t in range(bad.plan.T) for s in range(4) if (int(bad.geo.pedge[t]) >> s) & 1]
    assert len(sides) == 48
    seen_cone, dmin, emin = 0, np.inf, np.inf
    for t, s in sides:
        gb = torch.as_tensor(np.ascontiguousarray(gradb_with_reversed_ghost_strip(bad.geo, b, t, s)))
        d = float((gb - intact).norm(dim=0).max()) / gmax
        bad.tens["gradb"] = gb
        install(bad, G)
        bad.step(1)
        errs = increment_error(good, bad, q0)
        e = max(errs[1:4])
        changed = gradb_with_reversed_ghost_strip(cone.geo, bc, t, s) != cone.tens["gradb"].numpy()
        seen_cone += bool(changed.any())
        print(f"tile {t} side {'WESN'[s]}: grad b changes by {d:.3f} of the maximum, "
              f"momentum increment error {e:.2e}; tc5 cone {'changes' if changed.any() else 'unchanged'}")
        dmin, emin = min(dmin, d), min(emin, e)
        assert d >= 1e-2 and e > 1e-6, (t, s, d, errs)
    bad.tens["gradb"] = intact
    assert torch.equal(torch.as_tensor(np.ascontiguousarray(np.moveaxis(bad.geo.fv_gradient(b), -1, 0))), intact)
    print(f"48 of 48 sides seen: smallest grad b change {dmin:.3f}, smallest increment error {emin:.2e}; "
          f"tc5 cone: {seen_cone} of 48 sides")
    assert seen_cone < 48 // 4


# ---- the cached cell records follow the topography -------------------------------
def test_cell_records_are_cached_per_topography():
    """On one shared grid the records of ShallowWater("tc5") and then of
    TopographySWE("tc5") differ, the second with grad b != 0 in every cell
    (they once shared a cache entry keyed by the case name); the same
    topography still shares its entry."""
    grid = CubedSphereGrid(24)
    cone = global_cell_records(_engine(ShallowWater("tc5"), 24, 2, grid=grid))
    e = _engine(TopographySWE("tc5"), 24, 2, grid=grid)
    rec = global_cell_records(e)
    assert rec is not cone and not np.array_equal(rec[:, 4:7], cone[:, 4:7])
    assert (np.abs(rec[:, 4:7]).max(1) > 0).all()
    assert float((np.abs(cone[:, 4:7]).max(1) > 0).mean()) < 0.05
    assert np.array_equal(rec[:, :4], cone[:, :4]) and np.array_equal(rec[:, 7:], cone[:, 7:])
    # the records are the oracle's grad b, cell for cell
    gb = np.stack([assemble_global(e.layout, {0: e.tens["gradb"][k].numpy()}) for k in range(3)], -1)
    assert np.array_equal(rec[:, 4:7], gb.reshape(-1, 3))
    assert global_cell_records(_engine(TopographySWE("tc5", limiter=1), 24, 1, grid=grid)) is rec
    assert global_cell_records(_engine(ShallowWater("tc5"), 24, 1, grid=grid)) is cone


# ---- several ranks ------------------------------------------------------------------
@pytest.mark.parametrize("N,t,R", [(32, 2, 2), (32, 2, 3), (32, 2, 8), (48, 1, 6)])
def test_fused_exchange_ranks_equal_one_rank_over_the_topography(N, t, R):
    """The body of tests/test_fused.py::test_fused_exchange_ranks_equal_one_rank
    from ``rough`` over the topography, on the shared grid: the grad b rows of
    the remote cells come from the global records in ring-slot order, and the
    assembled state equals the one-rank fused step bit for bit."""
    grid = grid_of(N)
    G = _global(N, "rough")
    mk = lambda: TopographySWE("tc5")
    # what the bug needed: plain tc5 records already cached on this grid
    global_cell_records(_engine(ShallowWater("tc5"), N, t))
    L1 = TileLayout(N, t, 1, ng=2)
    one = Engine(mk(), L1, grid=grid)
    install(one, G)
    f1 = FusedTorch(one, FusedPlan(L1, 0, grid, B=16))
    L = TileLayout(N, t, R, ng=2)
    X = FusedExchangePlan(L, grid, 16)
    engs = [Engine(mk(), L, r, grid=grid, dt=one.dt) for r in range(R)]
    for e in engs:
        install(e, G)
    fts = [FusedTorch(engs[r], X.plans[r], remote_cells=X.need_remote[r]) for r in range(R)]
    assert sum(len(X.need_remote[r]) for r in range(R)) > 0
    for _ in range(2):
        f1.step()
        states = [e.pool[0] for e in engs]
        recvs = []
        for r in range(R):
            g = X.need_remote[r]
            tid, _, _ = L.locate(g)
            own = np.asarray(L.owner)[tid]
            off = L.local_flat(g)
            recvs.append(torch.stack([states[int(o)][:, int(k)] for o, k in zip(own, off)]) if len(g) else None)
        for r in range(R):
            fts[r].step(recvs[r])
    a, b = global_of(one), global_of(engs)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("ranks", [2, 8])
def test_virtual_ranks_equal_one_rank_over_the_topography(ranks):
    """VirtualCluster with 2 and 8 ranks of C24 t=2 on the oracle (grad b from
    each rank's own RankGeometry.fv_gradient) equals one rank bit for bit."""
    N, t = 24, 2
    one, _ = _topo(N, t, 2, "rough")
    vc = VirtualCluster(lambda: TopographySWE("tc5"), TileLayout(N, t, ranks, ng=2), grid=grid_of(N), dt=one.dt)
    for e in vc.engines:
        install(e, _global(N, "rough"))
    one.step(2)
    vc.step(2)
    a, b = global_of(one), global_of(vc.engines)
    assert torch.isfinite(a).all() and torch.equal(a, b)
