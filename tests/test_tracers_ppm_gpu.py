"""Monotone PPM for the shallow-water tracers on the GPU: the PPM variant of
``ops/csrc/swe_tracer_stage.hip`` (three-layer window, tracer faces formed in
the flux phase, two interpolated ghost layers at the panel edges) against its
fp64 PyTorch twin (``ShallowWaterTracers(..., tracer_limiter="ppm")``), with
the project's bounds: relative error below 1e-11 for fp64 and below 1e-4 for
fp32.  Blocks are those the LDS rule admits for the case; every test asserts
which block ran."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from stsphere.engine import Engine, VirtualCluster
from stsphere.models.base import extend
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater, ShallowWaterTracers
from stsphere.ops import native
from stsphere.ops.hip_compute import TRACER_LDS_MAX, tracer_lds_bytes
from stsphere.parallel.layout import TileLayout

from tracer_states import TRACER_SETS, increment_error, install, make_state

pytestmark = pytest.mark.gpu

BLOCKS = [(16, 16), (16, 8)]
FP64_BOUND, FP32_BOUND = 1e-11, 1e-4


def _blocks(nq, dtype=torch.float64):
    """The blocks whose launch fits in LDS (fp64 with four tracers: 16 x 8 only)."""
    es = 8 if dtype == torch.float64 else 4
    return [b for b in BLOCKS if tracer_lds_bytes(b[0], b[1], nq, es, 4) <= TRACER_LDS_MAX]


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _phys(nq, lim, case="tc5", tracers=None, tracer_limiter="ppm"):
    return ShallowWaterTracers(case, tracers=tracers or TRACER_SETS[nq], limiter=lim, tracer_limiter=tracer_limiter)


def _lay(N, t, ranks=1, ng=3):
    return TileLayout(N, t, ranks, ng=ng)


@functools.lru_cache(maxsize=None)
def _reference(N, t, nq, lim, integ, steps):
    """The twin's state after ``steps`` steps (fp64, once per case, shared by
    the block shapes and precisions; never stepped again), and its dt."""
    ref = Engine(_phys(nq, lim), _lay(N, t), grid=_grid(N), dtype=torch.float64, device="cuda", backend="torch",
                 integrator=integ)
    ref.step(steps)
    torch.cuda.synchronize()
    return ref.tiles_view().detach().clone(), ref.dt


def _hip(N, t, nq, lim, block, dtype=torch.float64, integ="ssprk3", dt=None, **kw):
    e = Engine(_phys(nq, lim, **kw), _lay(N, t), grid=_grid(N), dtype=dtype, device="cuda", backend="hip",
               integrator=integ, block=block, dt=dt)
    assert e.compute.phys_id == 3 and (e.compute.bx, e.compute.by) == tuple(block) and e.compute._tlim == 4
    return e


def _relerr(a, hip):
    F = a.shape[0]
    b = hip.tiles_view().double()
    assert bool(torch.isfinite(b).all()), f"{int((~torch.isfinite(b)).sum())} non-finite values in the hip state"
    a, b = a.reshape(F, -1), b.reshape(F, -1)
    return ((a - b).abs().amax(dim=1) / a.abs().amax(dim=1).clamp_min(1e-30)).max().item()


def _check(N, t, nq, lim, block, dtype=torch.float64, integ="ssprk3", steps=4):
    a, dt = _reference(N, t, nq, lim, integ, steps)
    hip = _hip(N, t, nq, lim, block, dtype, integ, dt)
    hip.step(steps)
    torch.cuda.synchronize()
    err = _relerr(a, hip)
    print(f"C{N} t={t} nq={nq} lim={lim} PPM tracers block={block} {dtype} {integ}: rel err {err:.3e}")
    assert err < (FP64_BOUND if dtype == torch.float64 else FP32_BOUND)


# NQ = 2 with every dynamics limiter, NQ = 1 and 4 with MC; 16 x 16 with four
# fp64 tracers does not fit in LDS and is no case (test_launcher_contract)
CASES = [(t, nq, lim, block) for t in (1, 2) for nq, lim in ((2, 0), (2, 1), (2, 2), (2, 3), (1, 2), (4, 2))
         for block in _blocks(nq)]


@pytest.mark.parametrize("t,nq,lim,block", CASES)
def test_kernel_matches_twin(t, nq, lim, block):
    _check(24, t, nq, lim, block)


@pytest.mark.parametrize("integ", ["euler", "rk4"])
def test_integrators(integ):
    _check(24, 2, 2, 2, (16, 16), integ=integ)


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("N,t", [(17, 1), (18, 1), (34, 2), (20, 1)])
def test_partial_blocks(N, t, block):
    """n = 17: the last block is one cell wide; n = 18: two cells wide, so with
    three ghost layers the last-but-one block's window reaches the ghost strip
    too (block_sides); n = 20: a partial block."""
    _check(N, t, 2, 2, block)


def _arm_shares(e):
    """Shares of the parabola limiter's arms and of the active clamp over the
    interior (cell, direction) pairs of the tracer rows, on the twin's window
    (raw ghosts) of a one-rank engine."""
    g, n, T = 3, e.plan.n, e.plan.T
    qe = extend(e.pool[0], None, e.gmap, T, n, g, cmap=e.cmap).double()
    w = qe[4:] / qe[0]
    out = {k: 0.0 for k in ("flat", "over_l", "over_r", "untouched", "clamp")}
    for rows in (w[:, :, g:g + n, :], w.transpose(-1, -2)[:, :, g:g + n, :]):
        def cell(c0, c1):
            return rows[..., c0 + g:c1 + g]
        a0 = (7.0 / 12.0) * (cell(-1, n) + cell(0, n + 1)) - (1.0 / 12.0) * (cell(-2, n - 1) + cell(1, n + 2))
        lo, hi = torch.minimum(cell(-1, n), cell(0, n + 1)), torch.maximum(cell(-1, n), cell(0, n + 1))
        a = torch.minimum(torch.maximum(a0, lo), hi)
        aL, aR, c = a[..., :-1], a[..., 1:], cell(0, n)
        flat = (aR - c) * (c - aL) <= 0
        d = aR - aL
        m6 = 6.0 * (c - 0.5 * (aL + aR))
        ol = ~flat & (d * m6 > d * d)
        orr = ~flat & ~ol & (-(d * d) > d * m6)
        for k, v in (("flat", flat), ("over_l", ol), ("over_r", orr), ("untouched", ~flat & ~ol & ~orr),
                     ("clamp", (a0 != a)[..., :-1])):
            out[k] += 0.5 * float(v.double().mean())
    return out


@pytest.mark.parametrize("t", [1, 2])
@pytest.mark.parametrize("cls", ["rough", "plateau"])
def test_rough_start(cls, t):
    """Rough SWE state and rough tracers: every arm of the parabola limiter and
    the clamp are taken by at least 5 % of the interior (cell, direction)
    pairs; measured on the increment of one step."""
    N = 16
    L = _lay(N, t)
    for lim in (0, 2):
        ref = Engine(_phys(2, lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="torch")
        G = make_state(ref, cls)
        if t == 1:
            probe = Engine(_phys(2, lim), L, grid=_grid(N), dtype=torch.float64, device="cpu", backend="torch")
            install(probe, G)
            shares = _arm_shares(probe)
            print(f"{cls}: arms {({k: round(v, 3) for k, v in shares.items()})}")
            assert min(shares.values()) >= 0.05, shares
        for block in BLOCKS:
            r = Engine(_phys(2, lim), L, grid=_grid(N), dtype=torch.float64, device="cuda", backend="torch", dt=ref.dt)
            hip = _hip(N, t, 2, lim, block, dt=ref.dt)
            q0 = install(r, G)
            install(hip, G)
            r.step(1)
            hip.step(1)
            torch.cuda.synchronize()
            errs = increment_error(r, hip, q0, bound=FP64_BOUND, block=block, what=f"{cls} lim {lim} block {block}")
            print(f"{cls} t={t} lim={lim} block={block}: increment errors {['%.2e' % e for e in errs]}")


@pytest.mark.parametrize("ranks", [2, 8])
def test_remote_ghosts_virtual_ranks(ranks):
    """Several virtual ranks on one GPU against one rank: three-layer receive
    rows of 4 + NQ values and the interior / boundary block lists."""
    N = 24
    mk = lambda: _phys(2, 2)   # noqa: E731
    single = Engine(mk(), _lay(N, 2), grid=_grid(N), device="cuda", backend="hip")
    vc = VirtualCluster(mk, _lay(N, 2, ranks), grid=_grid(N), device="cuda", backend="hip", dt=single.dt)
    for e in [single] + list(vc.engines):
        assert e.compute.phys_id == 3 and e.compute._tlim == 4 and (e.compute.bx, e.compute.by) in BLOCKS
    print(f"blocks: one rank {(single.compute.bx, single.compute.by)}, "
          f"{ranks} ranks {(vc.engines[0].compute.bx, vc.engines[0].compute.by)}")
    single.step(5)
    vc.step(5)
    torch.cuda.synchronize()
    for f in range(6):
        a, b = single.global_field(f), vc.global_field(f)
        assert abs(a - b).max() <= 1e-12 * max(1.0, abs(a).max()), f


@pytest.mark.parametrize("block", BLOCKS)
def test_properties_on_the_device(block):
    """q = 0.75 stays constant, a 0/1 cap stays in [0, 1] and the tracer masses
    drift by rounding only: C24, 20 steps."""
    N = 24
    e = _hip(N, 2, 2, 2, block, tracers=[0.75, "cap"])
    A = e.tens["area"]
    m0 = [(e.tiles_view()[4 + k] * A).sum().item() for k in range(2)]
    e.step(20)
    torch.cuda.synchronize()
    v = e.tiles_view()
    q = v[4:] / v[0]
    dev = (q[0] - 0.75).abs().max().item()
    lo, hi = q[1].min().item(), q[1].max().item()
    drift = [abs((v[4 + k] * A).sum().item() - m0[k]) / abs(m0[k]) for k in range(2)]
    print(f"block {block}: constancy {dev:.2e}; cap min {lo:.3e} max - 1 {hi - 1:.3e}; mass drift {drift}")
    assert dev < 1e-13
    assert -1e-12 <= lo and hi <= 1.0 + 1e-12
    assert max(drift) < 1e-13


def test_swe_rows_match_the_plain_stage_kernel():
    """h and M of a PPM-tracer run (ng = 3) against the plain SWE run on
    stage_kernel.hip (ng = 2), same block."""
    N = 24
    worst = 0.0
    for block in BLOCKS:
        a = Engine(ShallowWater("tc5", limiter=2), _lay(N, 2, ng=2), grid=_grid(N), device="cuda", backend="hip",
                   block=block)
        b = _hip(N, 2, 2, 2, block, dt=a.dt)
        c = Engine(_phys(2, 2, tracer_limiter=None), _lay(N, 2, ng=2), grid=_grid(N), device="cuda", backend="hip",
                   block=block, dt=a.dt)
        assert (a.compute.bx, a.compute.by) == (c.compute.bx, c.compute.by) == block and c.compute._tlim == 0
        for e in (a, b, c):
            e.step(8)
        torch.cuda.synchronize()
        x, y = a.tiles_view().reshape(4, -1), b.tiles_view()[:4].reshape(4, -1)
        err = ((x - y).abs().amax(1) / x.abs().amax(1)).max().item()
        same = torch.equal(b.tiles_view()[:4], c.tiles_view()[:4])
        print(f"SWE rows, PPM-tracer kernel vs stage kernel, block {block}: rel diff {err:.3e}; "
              f"bitwise equal to the PLR-tracer run: {same}")
        worst = max(worst, err)
    assert worst < FP64_BOUND


@pytest.mark.parametrize("block", BLOCKS)
def test_fp32(block):
    _check(24, 2, 2, 2, block, dtype=torch.float32)


def test_launcher_contract():
    """Two ghost layers with PPM tracers: the launcher's own error code, before
    anything is launched; a block whose launch does not fit in LDS: a
    ValueError from HipCompute that names the bytes."""
    N = 24
    e = _hip(N, 2, 2, 2, (16, 8))
    hc = e.compute
    d = hc.desc(e.integ.stages[0], e.dt, None, hc.nblocks)
    assert d.mg == 3 and d.tracer_limiter == 4
    d.mg, d.pw = 2, d.n + 4
    lib = native.require_native()
    rc = lib.stsp_stage_launch(3, hc.dcode, 16, 8, d, native.current_stream_handle())
    assert rc == -15
    with pytest.raises(RuntimeError, match="-15"):
        native.check(rc, "tracer stage kernel")
    lib.stsp_swe_tracer_lds_tl.argtypes = [ctypes.c_int] * 5
    lib.stsp_swe_tracer_lds_tl.restype = ctypes.c_int
    lib.stsp_swe_tracer_lds.argtypes = [ctypes.c_int] * 4
    lib.stsp_swe_tracer_lds.restype = ctypes.c_int
    for bx, by in BLOCKS:
        for nq in (1, 2, 3, 4):
            for dc, es in ((1, 8), (0, 4)):
                assert lib.stsp_swe_tracer_lds_tl(dc, bx, by, nq, 4) == tracer_lds_bytes(bx, by, nq, es, 4)
                assert lib.stsp_swe_tracer_lds_tl(dc, bx, by, nq, 0) == lib.stsp_swe_tracer_lds(dc, bx, by, nq) \
                    == tracer_lds_bytes(bx, by, nq, es, 0)
    assert lib.stsp_swe_tracer_lds_tl(1, 16, 16, 4, 4) == 70016
    with pytest.raises(ValueError, match="70016 bytes"):
        Engine(_phys(4, 2), _lay(N, 2), grid=_grid(N), device="cuda", backend="hip", block=(16, 16))
    # the rule never picks it
    auto = Engine(_phys(4, 2), _lay(48, 1), grid=_grid(48), device="cuda", backend="hip")
    assert (auto.compute.bx, auto.compute.by) == (16, 8)


def test_solver_on_the_shipped_config(tmp_path):
    """configs/c48_tracers_ppm_1gpu.yaml shortened to 8 steps at C24, fused off:
    the stage path runs physics 3 on three ghost layers; the products exist."""
    import os

    import yaml

    import stsphere as S
    with open(os.path.join(S.__path__[0], "configs", "c48_tracers_ppm_1gpu.yaml")) as f:
        c = yaml.safe_load(f)
    c["grid"]["N"] = 24
    c["time"] = {"integrator": "ssprk3", "nsteps": 8}
    c["io"] = {"output_dir": str(tmp_path)}
    c["runtime"] = {"fused": "off"}
    s = S.Solver(c, verbose=False)
    s.initialize()
    s.step(8)
    hc = s.engines[0].compute
    assert s.fused is None and hc.phys_id == 3 and hc._tlim == 4 and s.layout.ng == 3
    assert (hc.bx, hc.by) in BLOCKS
    g = s.gather_global()
    assert np.array_equal(s.tracer(0), g[4] / g[0])
    ll = s.latlon_field("q0", 8, 16)
    assert ll.shape == (8, 16) and np.isfinite(ll).all()
    tn = s.tracer_error_norms()
    print(f"block {(hc.bx, hc.by)}; cosine bell after 8 steps: {tn}")
    assert set(tn) == {"l1", "l2", "linf"} and all(np.isfinite(v) and 0 <= v < 1 for v in tn.values())
    assert s.tracer_error_norms(1) is None
    s.close()
