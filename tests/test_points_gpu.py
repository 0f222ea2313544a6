"""The gfx950 points kernel (ops/csrc/points_kernel.hip) against its twin
(models/points.py), and its plumbing through the solver."""
import functools

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine
from stsphere.models import points as mp
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

from points_sets import MARGIN, SHAPES, check_coverage, point_set, random_points

pytestmark = pytest.mark.gpu

CASES = ["tc5", "tc6"]
# the project's fp64 bound, relative to max |field| (a vector counts as one
# field).  Kernel and twin evaluate the same fp64 expressions; they differ by the
# last bits of atan, sqrt and the divisions, which move a weight by ~N eps
BOUND = 1e-12


@functools.lru_cache(maxsize=None)
def _state(N, t, case):
    """CPU fp64 engine two steps into the case (the shared reference state)."""
    e = Engine(ShallowWater(case), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N))
    e.step(2)
    return e


class _Stub:
    """What ``PointSampler`` reads of an engine, for a layout no engine can step:
    (9, 3) has tiles of 3 cells, fewer than the 2 ng = 4 the shallow-water halo
    needs, so its padded storage is built here with one ghost layer (NaN in the
    ghosts) from the one-tile engine's state."""

    def __init__(self, N, t, case, dtype, device, backend):
        from stsphere.engine import assemble_global
        from stsphere.models.base import interior
        from stsphere.ops.points import PointSampler
        ref = _state(N, 1, case)
        self.layout, self.rank, self.grid = TileLayout(N, t, 1, ng=1), 0, ref.grid
        self.plan = self.layout.plan(0)
        self.device, self.dtype, self.backend, self.dt = torch.device(device), dtype, backend, ref.dt
        glob = np.stack([assemble_global(ref.layout, {0: v}) for v in ref.tiles_view().numpy()]).reshape(4, -1)
        pad, _ = mp.rank_maps(self.layout, 0)
        q = torch.full((4, self.plan.S), float("nan"), dtype=torch.float64)
        q[:, torch.as_tensor(pad, dtype=torch.long)] = torch.as_tensor(glob)
        self.state = q.to(dtype).to(self.device)
        self._interior = lambda: interior(self.state, self.plan.T, self.plan.n, self.plan.ng)
        self._sampler = PointSampler(self)

    def points(self):
        return self._sampler

    def tiles_view(self):
        return self._interior()


def _engine(N, t, case, dtype=torch.float64, device="cuda:0", backend="hip"):
    if N // t < 4:
        return _Stub(N, t, case, dtype, device, backend)
    ref = _state(N, t, case)
    e = Engine(ShallowWater(case), ref.layout, grid=ref.grid, dtype=dtype, device=device, backend=backend, dt=ref.dt)
    e.set_state(ref.tiles_view().to(dtype))
    return e


def _twin(e, p):
    """(fields [F, K], tiles [F, K], velocity [3, K], elem [K]) of the twin on
    the engine's own state (whatever its type), on the CPU."""
    sm = e.points()
    q = e.state.detach().cpu()
    pad = mp.locate(sm.N, p, sm.pad_np, sm.tab.mesh)
    unp = mp.locate(sm.N, p, sm.unp_np, sm.tab.mesh)
    return (mp.sample(q, pad), mp.sample(e.tiles_view().detach().cpu().reshape(q.shape[0], -1), unp),
            mp.velocity(q, pad), pad.elem)


def _close(got, ref, vector=False):
    got, ref = got.detach().cpu(), ref.detach().cpu()
    scale = ref.abs().max() if vector else ref.abs().amax(1, keepdim=True)
    err = ((got - ref).abs() / scale).max().item()
    print(f"  max |kernel - twin| / max |field| = {err:.3e}")
    assert torch.isfinite(got).all() and err <= BOUND, err


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,t", SHAPES)
def test_kernel_against_twin(N, t, case, dtype):
    """All three sampling modes and the element ids on the constructed point
    set; fp32: the twin on the same fp32 state (the arithmetic is fp64 in both)."""
    e = _engine(N, t, case, dtype)
    p = point_set(N)
    sm = e.points()
    assert sm.hip
    f, el = sm.fields(p, elem=True)
    tl = sm.tiles(p, e.tiles_view().contiguous())
    v = sm.velocity(p)
    torch.cuda.synchronize()
    rf, rt, rv, rel = _twin(e, p)
    check_coverage(N, rel)
    assert np.array_equal(el.cpu().numpy(), rel)
    assert f.dtype == torch.float64 and f.shape == (4, len(p))
    _close(f, rf)
    _close(tl, rt)
    _close(v, rv, vector=True)


@pytest.mark.parametrize("K", [1, 257])
def test_small_sets(K):
    e = _engine(9, 3, "tc5")
    p = point_set(9)[-K:]
    f, el = e.points().fields(p, elem=True)
    rf, _, _, rel = _twin(e, p)
    assert np.array_equal(el.cpu().numpy(), rel)
    _close(f, rf)


def _particles(e, K=300, interval=4, seed=3):
    lat, lon = mp.points_lonlat(random_points(seed, K))
    return e.particles(lat, lon, interval=interval)


def test_determinism_and_routes():
    """Repeatable bit for bit; the terms fold to the direct result; the fused
    advance equals sample then advance, with and without terms."""
    e = _engine(12, 2, "tc6")
    sm, p = e.points(), point_set(12)
    for fn in (sm.fields, sm.velocity):
        a, b, t = fn(p), fn(p), fn(p, terms=True)
        assert torch.equal(a, b) and torch.equal(mp.fold_terms(t), a)
    a, b, c = (_particles(e) for _ in range(3))
    for P in (a, b, c):
        P.start()
    for _ in range(5):
        a.advance()
        b.advance_sequenced()
        c.advance_sequenced(terms=True)
    torch.cuda.synchronize()
    assert torch.isfinite(a.st.x).all()
    for other in (b, c):
        for u, v in zip((a.st.x, a.st.xs, a.st.v0), (other.st.x, other.st.xs, other.st.v0)):
            assert torch.equal(u, v)


def test_ghost_poison():
    """NaN in the whole ghost ring: the same results bit for bit."""
    e = _engine(24, 2, "tc6")
    sm, p = e.points(), point_set(24)
    P = _particles(e)
    P.start()
    before = [sm.fields(p), sm.velocity(p)]
    x0 = [t.clone() for t in (P.st.x, P.st.xs, P.st.v0)]
    P.advance()
    x1 = P.st.x.clone()
    keep = e.tiles_view().clone()
    e.state.fill_(float("nan"))
    e.tiles_view().copy_(keep)
    assert int(torch.isnan(e.state).sum()) == 4 * (e.plan.S - e.plan.T * e.plan.n ** 2)
    after = [sm.fields(p), sm.velocity(p)]
    for dst, src in zip((P.st.x, P.st.xs, P.st.v0), x0):
        dst.copy_(src)
    P.advance()
    torch.cuda.synchronize()
    for a, b in zip(before, after):
        assert torch.isfinite(b).all() and torch.equal(a, b)
    assert torch.equal(P.st.x, x1)


def _gpu_cfg(out, nd=1, t=2, **io):
    return {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "gpu"},
            "grid": {"N": 24}, "physics": {"model": "swe", "case": "tc5"}, "time": {"nsteps": 12},
            "runtime": {"fused": "on" if nd == 1 else "auto"}, "io": dict({"output_dir": str(out)}, **io)}


def _twin_engine(state, dt):
    N = state.shape[-1]
    e = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), dt=dt)
    e.set_state(torch.as_tensor(state))
    return e


def test_after_fused_stepping(tmp_path):
    """The ghost slots are not current after a fused multi-step launch: the
    sampling reads none."""
    s = S.Solver(_gpu_cfg(tmp_path), verbose=False)
    s.initialize()
    s.step(6)
    assert s.fused is not None
    p = point_set(24)
    lat, lon = mp.points_lonlat(p)
    names = ("h", "mx", "my", "mz")
    got = s.sample(names, lat, lon)
    e = _twin_engine(s.gather_global(), s.dt)
    ref = e.points().fields(mp.lonlat_points(lat, lon))
    _close(torch.as_tensor(got), ref)


def test_nan_patch():
    """A state with a NaN patch of cells (what the watchdog would meet):
    particles whose stencil touches it are lost after one advance and stay so;
    all others equal the twin.  No address depends on the state's values: the
    kernel's indices come from the point and the clamped tables only."""
    e = _engine(24, 2, "tc5")
    tv = e.tiles_view()
    tv[:, 1, 3:8, 2:9] = float("nan")
    cpu = Engine(ShallowWater("tc5"), e.layout, grid=e.grid, dt=e.dt)
    cpu.set_state(tv.detach().cpu())
    a, b = _particles(e, K=2000, seed=5), _particles(cpu, K=2000, seed=5)
    for P in (a, b):
        P.start()
        P.advance()
    torch.cuda.synchronize()
    lost = torch.isnan(b.st.x).any(1)
    assert 0 < int(lost.sum()) < 2000
    for P in (a, b):
        P.advance()
    torch.cuda.synchronize()
    ga, gb = a.st.x.cpu(), b.st.x
    assert torch.equal(torch.isnan(ga).any(1), torch.isnan(gb).any(1))
    assert bool((torch.isnan(gb).any(1) | ~lost).all())          # lost stays lost
    ok = ~torch.isnan(gb).any(1)
    assert float((ga[ok] - gb[ok]).norm(dim=1).max()) <= BOUND


@pytest.mark.parametrize("nd", [2, 6])
def test_virtual_ranks_equal_one_rank(tmp_path, nd):
    """Six advances on one state (the one-rank run's, given to every rank): the
    ranks' terms add to the one-rank positions and samples bit for bit."""
    lat, lon = mp.points_lonlat(random_points(11, 200))
    out, state = [], None
    for k in (1, nd):
        s = S.Solver(_gpu_cfg(tmp_path / str(k), nd=k, t=1), verbose=False)
        s.initialize()
        if state is None:
            s.step(2)
            state = s.gather_global()
        assert len(s.engines) == k
        for e in s.engines:
            e.set_state(torch.as_tensor(np.stack([e.geo.gather_global(v) for v in state])))
        s.add_particles(lat, lon, interval=2)
        for _ in range(6):
            s._particles_advance()
        out.append((np.stack(s.particle_positions()), s.sample(("h", "mx", "u", "v"), lat, lon)))
    assert np.isfinite(out[0][0]).all()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_particles_follow_the_twin(tmp_path):
    """C24, 12 steps, interval 4: after every advance the positions equal the
    twin advanced on the same states within 1e-12 (chord on the unit sphere);
    every predictor and corrector point keeps its margin."""
    s = S.Solver(_gpu_cfg(tmp_path), verbose=False)
    s.initialize()
    seeds = random_points(13, 500)
    lat, lon = mp.points_lonlat(seeds)
    s.add_particles(lat, lon, interval=4)
    tw = mp.TwinParticles(24, mp.lonlat_points(lat, lon), 4 * s.dt, s.grid.radius)
    tw.start(torch.as_tensor(s.gather_global()))
    for _ in range(3):
        s.step(4)
        tw.advance(torch.as_tensor(s.gather_global()))
        x = s._particles[0].st.x.cpu()
        assert float((x - tw.st.x).norm(dim=1).max()) <= 1e-12
    assert s.fused is not None
    assert min(float(m.min()) for m in tw.margins) >= MARGIN
    la, lo = s.particle_positions()
    assert np.array_equal(np.stack([la, lo]), np.stack(mp.points_lonlat(s._particles[0].st.x.cpu().numpy())))


def test_particles_in_a_run(tmp_path):
    """C24, 12 steps, interval 4, history every 4: every frame's positions equal
    the twin advanced on that run's own history frames within 1e-12 (chord on the
    unit sphere); the last frame equals ``particle_positions()`` bit for bit."""
    from stsphere.utils import zarr_lite
    seeds = random_points(13, 500)
    lat, lon = mp.points_lonlat(seeds)
    s = S.Solver(_gpu_cfg(tmp_path, history_interval=4,
                          particles={"lat": lat.tolist(), "lon": lon.tolist(), "interval": 4, "fields": ["h"]}),
                 verbose=False)
    s.initialize()
    s.run()
    assert s.fused is not None
    hist, hp = str(tmp_path / "history.zarr"), str(tmp_path / "history_particles.zarr")
    frames = np.stack([zarr_lite.read_array(hist, f) for f in ("h", "mx", "my", "mz")], 1)      # [4, 4, 6, N, N]
    pl, po = zarr_lite.read_array(hp, "lat"), zarr_lite.read_array(hp, "lon")
    assert frames.shape[0] == 4 and pl.shape == (4, 500) and list(zarr_lite.read_array(hp, "step")) == [0, 4, 8, 12]
    tw = mp.TwinParticles(24, mp.lonlat_points(lat, lon), 4 * s.dt, s.grid.radius)
    tw.start(torch.as_tensor(frames[0]))
    for k in range(4):
        if k:
            tw.advance(torch.as_tensor(frames[k]))
        chord = np.linalg.norm(mp.lonlat_points(pl[k], po[k]) - tw.st.x.numpy(), axis=1).max()
        print(f"  frame {k}: max chord {chord:.3e}")
        assert chord <= 1e-12, (k, chord)
    assert min(float(m.min()) for m in tw.margins) >= MARGIN
    la, lo = s.particle_positions()
    assert np.array_equal(pl[-1], la) and np.array_equal(po[-1], lo)
    s.close()
