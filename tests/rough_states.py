"""Rough test states for the finite-volume kernels, and the metric that goes
with them (a plain helper module: ``from rough_states import ...``).

The analytic cases (tc2, tc5, tc6, cosine bell) are so smooth that the slope
limiters almost always return the central slope, so a kernel whose limiter
arms were wrong would still match the oracle on them.  The states here put
every primitive field into every arm:

``rough``     h (1 + 0.02 u), u ~ U(-1, 1) per cell; v + 20 m/s U(-1, 1) per
              component, projected onto the tangent plane; momentum h v.
``plateau``   piecewise constant on 2 x 3-cell patches: h = mean(h) (1 + 0.01 k),
              k in {-1, 0, 1}; v = 15 m/s k' per component.  Every cell has an
              exactly zero difference on at least one side.
``zero_mom``  the ``rough`` depth with momentum exactly 0.
``scalar``    (advection, diffusion) max|q0| U(0, 1) with 30 % of the cells
              exactly 0.

``TopographySWE`` puts a topography with a non-zero gradient under every cell
(the tc5 cone covers 3 % of them), for the tests of the term -g h grad b.

Every state is a function of the global grid alone (seeded
``torch.Generator``), so engines of any layout, rank count and precision get
the same field: build it once with ``global_state`` and ``install`` it.

``fp32_twin_bound`` is the reference of every fp32 kernel test: the fp64
oracle from the fp32-rounded state, and the increment error the PyTorch
backend makes against it when it runs in fp32 from that same state.
"""
import collections
import functools

import numpy as np
import torch

from stsphere.engine import Engine, assemble_global
from stsphere.models.base import PPM, cells_x, cells_y, extend
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

SWE_CLASSES = ("rough", "plateau", "zero_mom")
PATCH = (2, 3)            # plateau patch: 2 cells along x, 3 along y
SHARE_KEYS = ("opposite", "zero", "steep", "central")


def _uniform(gen, shape, lo, hi):
    return lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)


def global_of(engines) -> torch.Tensor:
    """[F, 6, N, N] fp64 global field of the engines of one layout (one engine,
    or all ranks of a ``VirtualCluster``)."""
    engines = list(engines) if isinstance(engines, (list, tuple)) else [engines]
    lay, F = engines[0].layout, engines[0].physics.F
    return torch.as_tensor(np.stack([
        assemble_global(lay, {e.rank: e.tiles_view()[f].detach().double().cpu().numpy() for e in engines})
        for f in range(F)]))


def local_of(engine, G: torch.Tensor) -> torch.Tensor:
    """Global [F, 6, N, N] -> this rank's [F, T, n, n] (fp64, CPU)."""
    g = G.numpy()
    return torch.as_tensor(np.stack([engine.geo.gather_global(g[f]) for f in range(g.shape[0])]))


def install(engine, G: torch.Tensor) -> torch.Tensor:
    """Install the global state on one engine (``Engine.set_state`` refreshes
    the halos); returns the fp64 local state q0 that was installed, as the
    engine holds it (rounded to the engine's precision)."""
    q = local_of(engine, G).to(engine.dtype)
    engine.set_state(q)
    return q.double()


def swe_state(G0: torch.Tensor, centers, cls: str, seed: int = 0) -> torch.Tensor:
    """Shallow-water state of class ``cls`` from the global initial state
    G0 [4, 6, N, N] and the cell centres [6, N, N, 3]."""
    gen = torch.Generator().manual_seed(1000 + seed)
    h0, M0 = G0[0], G0[1:4]
    shp = h0.shape
    if cls in ("rough", "zero_mom"):
        h = h0 * (1.0 + 0.02 * _uniform(gen, shp, -1.0, 1.0))
        if cls == "zero_mom":
            return torch.cat([h[None], torch.zeros_like(M0)])
        r = torch.as_tensor(np.moveaxis(np.asarray(centers), -1, 0))
        v = M0 / h0 + 20.0 * _uniform(gen, (3,) + shp, -1.0, 1.0)
        v = v - (v * r).sum(0) * r
        return torch.cat([h[None], h * v])
    if cls == "plateau":
        N = shp[-1]
        px, py = -(-N // PATCH[0]), -(-N // PATCH[1])
        k = torch.randint(-1, 2, (4, 6, py, px), generator=gen).double()
        k = k.repeat_interleave(PATCH[1], dim=2).repeat_interleave(PATCH[0], dim=3)[:, :, :N, :N]
        h = h0.mean() * (1.0 + 0.01 * k[0])
        return torch.cat([h[None], h * (15.0 * k[1:4])])
    raise ValueError(f"unknown shallow-water state class {cls!r}")


def scalar_state(G0: torch.Tensor, seed: int = 0) -> torch.Tensor:
    """max|q0| U(0, 1) with 30 % of the cells exactly 0 ([1, 6, N, N])."""
    gen = torch.Generator().manual_seed(2000 + seed)
    q = G0.abs().max() * _uniform(gen, G0.shape, 0.0, 1.0)
    zero = torch.rand(G0.shape, generator=gen, dtype=torch.float64) < 0.3
    return torch.where(zero, torch.zeros_like(q), q)


def make_state(engines, cls: str, seed: int = 0) -> torch.Tensor:
    """Global state of class ``cls`` ("rough", "plateau", "zero_mom" for
    shallow water, "scalar" for advection and diffusion) from the engines'
    current (initial) state."""
    engines = list(engines) if isinstance(engines, (list, tuple)) else [engines]
    G0 = global_of(engines)
    if cls == "scalar":
        return scalar_state(G0, seed)
    return swe_state(G0, engines[0].grid.centers(), cls, seed)


@functools.lru_cache(maxsize=None)
def grid_of(N: int) -> CubedSphereGrid:
    return CubedSphereGrid(N)


# ---------------------------------------------------------------------------
# topography in every cell
# ---------------------------------------------------------------------------

def topography(grid: CubedSphereGrid) -> np.ndarray:
    """b [6, N, N] in metres, non-zero with a non-zero gradient in every cell:
    300 (1.5 + x y + 0.7 z x - 0.5 y z + 0.4 x) + 100 u with (x, y, z) the cell
    centre and u ~ U(-1, 1) per cell (56 m <= b <= 785 m at C24).  The smooth
    part has no symmetry of the cube; the noise makes every one-cell shift or
    reversal of a ghost strip visible."""
    p = np.asarray(grid.centers(), dtype=np.float64)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    gen = torch.Generator().manual_seed(3000)
    u = _uniform(gen, p.shape[:-1], -1.0, 1.0).numpy()
    return 300.0 * (1.5 + x * y + 0.7 * z * x - 0.5 * y * z + 0.4 * x) + 100.0 * u


class TopographySWE(ShallowWater):
    """A shallow-water case (depth and wind of the base case) over
    ``topography``: the tc5 cone covers 3 % of the cells, two panels and one
    cube edge, so every rendering of -g h grad b is otherwise untested
    almost everywhere.  Only ``global_fields`` differs: setup, the streaming
    stage's b table and the fused step's records read b through it."""

    def global_fields(self, grid: CubedSphereGrid):
        h, wind, _ = super().global_fields(grid)
        return h, wind, topography(grid)


SIDE_STRIP = {0: (slice(1, -1), 0), 1: (slice(1, -1), -1), 2: (0, slice(1, -1)), 3: (-1, slice(1, -1))}   # W E S N


def gradb_with_reversed_ghost_strip(geo, b: np.ndarray, tile: int, side: int) -> np.ndarray:
    """grad b [3, T, n, n] (the layout of ``Engine.tens["gradb"]``) of the rank
    geometry ``geo`` with the layer-0 ghost strip of b on ``side`` (0 W, 1 E,
    2 S, 3 N) of local tile ``tile`` read in reversed order: the mistake a
    wrong orientation on a reversed cube edge makes.  ``geo`` is left as it
    was."""
    keep = geo.ext1
    try:
        geo.ext1 = keep.copy()
        strip = geo.ext1[tile][SIDE_STRIP[side]]
        geo.ext1[tile][SIDE_STRIP[side]] = strip[::-1].copy()
        gb = geo.fv_gradient(b)
    finally:
        geo.ext1 = keep
    return np.moveaxis(gb, -1, 0)


# ---------------------------------------------------------------------------
# which limiter arms a state reaches
# ---------------------------------------------------------------------------

def _primitive_window(engine) -> torch.Tensor:
    """[F, T, n+2g, n+2g] primitive window of a one-rank engine's state, as
    ``Physics.rhs`` builds it (raw index-space ghosts)."""
    e = engine
    assert e.layout.num_ranks == 1, "branch_shares reads no receive buffer"
    g = e.physics.halo
    qe = extend(e.pool[0], None, e.gmap, e.plan.T, e.plan.n, g, cmap=e.cmap).double()
    if e.physics.name != "swe":
        return qe
    h = qe[0]
    safe = torch.where(h != 0, h, torch.ones_like(h))
    return torch.stack([h, qe[1] / safe, qe[2] / safe, qe[3] / safe])


def _line_shares(rows: torch.Tensor, g: int, n: int, lim: int) -> dict:
    """rows [..., n, n+2g]: the oracle's limiter conditions at the interior
    cells of every line."""
    c = rows[..., g:g + n]
    dl = c - rows[..., g - 1:g + n - 1]
    dr = rows[..., g + 1:g + n + 1] - c
    p = dl * dr
    cen = 0.5 * (dl + dr)
    steep = (p > 0) & (2.0 * torch.minimum(dl.abs(), dr.abs()) < cen.abs())
    out = {"opposite": (p < 0), "zero": (dl == 0) | (dr == 0), "steep": steep,
           "central": (p > 0) & ~steep}
    if lim == PPM:
        def cell(c0, c1):
            return rows[..., c0 + g:c1 + g]
        a = (7.0 / 12.0) * (cell(-1, n) + cell(0, n + 1)) - (1.0 / 12.0) * (cell(-2, n - 1) + cell(1, n + 2))
        aL, aR = a[..., :-1], a[..., 1:]
        qc = cell(0, n)
        flat = (aR - qc) * (qc - aL) <= 0
        d = aR - aL
        m6 = 6.0 * (qc - 0.5 * (aL + aR))
        over_l = ~flat & (d * m6 > d * d)
        over_r = ~flat & ~over_l & (-(d * d) > d * m6)
        out.update(ppm_flat=flat, ppm_over_l=over_l, ppm_over_r=over_r, ppm_keep=~flat & ~over_l & ~over_r)
    return {k: float(v.double().mean()) for k, v in out.items()}


def branch_shares(engine, lim: int = 2) -> dict:
    """Shares of the oracle's limiter conditions on the primitive window of a
    one-rank engine's current state: ``{"x": [per field {opposite, zero,
    steep, central}], "y": [...], "speed": {...}}``.

    opposite: dl dr < 0 (slope 0); zero: dl == 0 or dr == 0; steep: same sign
    and 2 min(|dl|, |dr|) < |dl + dr| / 2 (the MC bound is active); central:
    same sign, bound inactive.  ``lim = 4`` adds the shares of the PPM
    limiter's arms (ppm_flat, ppm_over_l, ppm_over_r, ppm_keep).  ``speed``
    (shallow water): the shares of the interior edges, per direction, where
    the Rusanov speed of the left cell exceeds the right one's and vice
    versa."""
    e = engine
    g, n = e.physics.halo, e.plan.n
    w = _primitive_window(e)
    F = w.shape[0]
    rows_x = w[:, :, g:g + n, :]
    rows_y = w.transpose(-1, -2)[:, :, g:g + n, :]
    out = {"x": [_line_shares(rows_x[f], g, n, lim) for f in range(F)],
           "y": [_line_shares(rows_y[f], g, n, lim) for f in range(F)]}
    if e.physics.name == "swe":
        grav = e.physics.g
        t = {k: v.double() for k, v in e.tens.items() if k in ("mx", "my")}
        sp = {}
        for ax, (cL, cR), m in (("x", cells_x(w, g, n), t["mx"].permute(1, 0, 2)[:, :, None, :]),
                                ("y", cells_y(w, g, n), t["my"].permute(1, 0, 2)[:, :, :, None])):
            sL = ((cL[1:] * m).sum(0)).abs() + torch.sqrt(grav * cL[0])
            sR = ((cR[1:] * m).sum(0)).abs() + torch.sqrt(grav * cR[0])
            sp[f"{ax}:sL>sR"] = float((sL > sR).double().mean())
            sp[f"{ax}:sR>sL"] = float((sR > sL).double().mean())
        out["speed"] = sp
    return out


# ---------------------------------------------------------------------------
# the metric
# ---------------------------------------------------------------------------

def _where(engine, f, t, j, i, block=None) -> str:
    """Where a cell sits: distances to the tile sides, which of them are panel
    edges, and its position in the kernel's block."""
    n = engine.plan.n
    pe = int(engine.geo.pedge[t])
    dist = {"W": i, "E": n - 1 - i, "S": j, "N": n - 1 - j}
    sides = ", ".join(f"{s} {d}{' (panel edge)' if (pe >> k) & 1 else ''}"
                      for k, (s, d) in enumerate(dist.items()))
    name = engine.physics.fields[f]
    msg = f"field {name} tile {t} j {j} i {i}; cells to the tile sides: {sides}"
    if block is not None:
        bx, by = block
        if bx == 64:                                # streaming stage: 60-column strips, `by` rows per segment
            msg += f"; march strip {i // 60} column {i % 60}, segment {j // by} row {j % by}"
        else:
            last = (n - 1) // bx == i // bx and n % bx, (n - 1) // by == j // by and n % by
            msg += (f"; block ({i // bx}, {j // by}) of {-(-n // bx)} x {-(-n // by)}, local ({i % bx}, {j % by})"
                    f"{', partial in x' if last[0] else ''}{', partial in y' if last[1] else ''}")
    return msg


def increment_error(ref, hip, q0: torch.Tensor, bound=None, block=None, what: str = ""):
    """Per field  max|(hip - q0) - (ref - q0)| / max|ref - q0|  over the
    interior cells, in fp64: the error of what the kernels computed, not of
    the state they carry.  ``q0`` is the [F, T, n, n] state both engines
    started from.  A NaN in either state raises with its location; with
    ``bound`` (a number, or one per field) a field above it raises with the
    worst cell's field, tile, row and column, its distance to each tile side,
    which sides are panel edges, and its position in ``block`` (the kernel's
    block shape; (64, R) for the streaming stage).  Returns the list of
    per-field errors."""
    a = ref.tiles_view().detach().double().cpu()
    b = hip.tiles_view().detach().double().cpu()
    q0 = q0.double().cpu().reshape(a.shape)
    for nm, x in (("reference", a), ("hip", b)):
        bad = ~torch.isfinite(x)
        if bool(bad.any()):
            f, t, j, i = torch.nonzero(bad)[0].tolist()
            raise AssertionError(f"{what}: {int(bad.sum())} non-finite values in the {nm} state, first at "
                                 + _where(ref, f, t, j, i, block))
    F = a.shape[0]
    da, db = a - q0, b - q0
    scale = da.reshape(F, -1).abs().amax(1)
    diff = (db - da).abs()
    errs = [float(diff[f].max() / scale[f]) if float(scale[f]) > 0 else float(diff[f].max()) for f in range(F)]
    if bound is not None:
        bounds = [float(bound)] * F if np.isscalar(bound) else [float(x) for x in bound]
        over = [f for f in range(F) if not errs[f] <= bounds[f]]
        if over:
            f = max(over, key=lambda k: errs[k] / max(bounds[k], 1e-300))
            t, j, i = np.unravel_index(int(diff[f].argmax()), diff[f].shape)
            raise AssertionError(
                f"{what}: increment error {errs[f]:.3e} > {bounds[f]:.3e} (all fields {['%.2e' % x for x in errs]}); "
                f"worst cell: {_where(ref, f, int(t), int(j), int(i), block)}; increment reference "
                f"{float(da[f, t, j, i]):.6e} kernel {float(db[f, t, j, i]):.6e}, max |increment| {float(scale[f]):.3e}")
    return errs


# ---------------------------------------------------------------------------
# the fp32 reference: oracle and PyTorch twin from the rounded state
# ---------------------------------------------------------------------------

EPS32 = float(torch.finfo(torch.float32).eps)
FP32_CAP = 1e-4           # the bound of the fp32 state tests the increment tests stand beside: none may be looser
Fp32Reference = collections.namedtuple("Fp32Reference", "ref q0 twin bound")


def physics_of(kind: str, lim: int):
    """``kind``: "adv", "diff", "topo" (tc5 over ``topography``) or a shallow-water case."""
    from stsphere.models.advection import Advection
    from stsphere.models.diffusion import Diffusion
    if kind == "adv":
        return Advection(limiter=lim)
    if kind == "diff":
        return Diffusion()
    if kind == "topo":
        return TopographySWE("tc5", limiter=lim)
    return ShallowWater(kind, limiter=lim)


@functools.lru_cache(maxsize=None)
def global_state(kind: str, N: int, cls: str) -> torch.Tensor:
    """The global start state of a class: a function of the case and the grid
    alone (not of the limiter, the layout, the precision or the device)."""
    phys = physics_of(kind, 2)
    return make_state(Engine(phys, TileLayout(N, 1, 1, ng=phys.halo), grid=grid_of(N)), cls)


def engine_of(kind, N, t, lim, cls, backend="torch", dtype=torch.float64, integ="ssprk3", block=None, dt=None,
              rounded=False, device="cuda"):
    """(one-rank engine with the class's state installed, q0).  ``rounded``:
    the state rounded to fp32 first (the start of the fp32 comparisons)."""
    phys = physics_of(kind, lim)
    e = Engine(phys, TileLayout(N, t, 1, ng=phys.halo), grid=grid_of(N), dtype=dtype, device=device,
               backend=backend, integrator=integ, block=block, dt=dt)
    G = global_state(kind, N, cls)
    return e, install(e, G.float().double() if rounded else G)


def twin_bound(twin_errs):
    """max(4 x twin, 4 eps32) per field: the margin the project gives an fp32
    kernel over the PyTorch twin (tests/test_derived_gpu.py), room for another
    order of operations and nothing else; 4 eps32 where the twin happens to be
    exact.  No bound may exceed ``FP32_CAP``."""
    bound = [max(4.0 * x, 4.0 * EPS32) for x in twin_errs]
    assert max(bound) <= FP32_CAP, f"fp32 twin bound {bound} above the cap {FP32_CAP}: the twin itself is off"
    return bound


def fp32_reference(make, steps: int) -> Fp32Reference:
    """``make(dtype, dt)`` -> (engine started from the fp32-rounded state, q0).
    Steps the fp64 oracle and, with the oracle's dt, the same backend in fp32;
    the code under test takes no part.  Neither engine is stepped again."""
    ref, q0 = make(torch.float64, None)
    ref.step(steps)
    twin, _ = make(torch.float32, ref.dt)
    twin.step(steps)
    if ref.device.type == "cuda":
        torch.cuda.synchronize()
    errs = increment_error(ref, twin, q0, what="fp32 twin")
    return Fp32Reference(ref, q0, errs, twin_bound(errs))


@functools.lru_cache(maxsize=None)
def fp32_twin_bound(kind, N, t, lim=2, cls="rough", integ="ssprk3", steps=2, device="cuda") -> Fp32Reference:
    """(ref, q0, twin, bound) of one case, computed once and shared by every
    kernel shape that runs it: the fp64 oracle after ``steps`` steps from the
    fp32-rounded state of class ``cls``, that state as installed, the per-field
    increment error of the PyTorch backend run in fp32 from it (with the
    oracle's dt), and ``twin_bound`` of that error."""
    return fp32_reference(lambda dtype, dt: engine_of(kind, N, t, lim, cls, dtype=dtype, integ=integ, dt=dt,
                                                      rounded=True, device=device), steps)
