"""The topography term -g h grad b in every stencil kernel (GPU), with
topography in every cell (tests/rough_states.py::TopographySWE; the tc5 cone
reaches 3 % of the cells, two panels and one cube edge): the block stage
kernel and march3 (grad b from the per-rank cell records), the streaming stage
on both geometry paths (cell records; compact: grad b formed in the kernel from
the padded b table and its ghost ring), the fused step (the gbt rows, indexed
by the window source code) and the remote renderings of both tables (loopback
layouts, virtual ranks), against the fp64 PyTorch oracle.

Unless stated otherwise a case starts from ``rough`` over the topography with
limiter 2, runs two SSP-RK3 steps with the oracle's dt and asserts
``increment_error`` per field below 1e-11; tests/test_topography_states.py
checks on the CPU that the term is 12 % of the largest momentum increment and
that one reversed ghost strip of b costs 1.8e-2 in this metric.  Further: g
and omega other than the defaults, tc2 with a rotated axis, the lake at rest
(the exact cancellation the curvature balance exists for) and fp32.  Every
case prints its measured errors; profiles/topography/README.md records them."""
import functools
import math

import pytest
import torch

from rough_states import (TopographySWE, fp32_twin_bound, global_of, grid_of, increment_error, install,
                          make_state)
from stsphere.engine import Engine, VirtualCluster
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

BOUND = 1e-11
STEPS = 2
TC5 = ("tc5", ())
OTHER = ("tc5", (("g", 11.0), ("omega", 5e-5)))
TC2_TILTED = ("tc2", (("alpha", math.pi / 4),))


def _physics(spec, lim):
    case, kw = spec
    return TopographySWE(case, limiter=lim, **dict(kw))


@functools.lru_cache(maxsize=None)
def _global(spec, N, cls):
    """The global start state of a class: a function of the case, its
    constants and the grid alone."""
    phys = _physics(spec, 2)
    return make_state(Engine(phys, TileLayout(N, 1, 1, ng=phys.halo), grid=grid_of(N)), cls)


def _engine(spec, N, t, lim=2, cls="rough", backend="torch", dtype=torch.float64, block=None, dt=None, rounded=False,
            loopback=None):
    """(engine on the GPU with the class's state installed, q0).  ``rounded``:
    the state rounded to fp32 first; ``loopback``: a layout with every ghost
    through the rank's own ring, "stage" with the receive buffers of the
    stage kernels' direct exchange, "fused" without (the caller attaches the
    exchange)."""
    phys = _physics(spec, lim)
    L = TileLayout(N, t, 1, ng=phys.halo, loopback=loopback is not None)
    kw = {}
    if loopback == "stage":
        from stsphere.parallel.comm import NativeBuffers
        kw["transport"] = NativeBuffers(L.plan(0), 4, dtype, torch.device("cuda"))
    e = Engine(phys, L, grid=grid_of(N), dtype=dtype, device="cuda", backend=backend, block=block, dt=dt, **kw)
    G = _global(spec, N, cls)
    return e, install(e, G.float().double() if rounded else G)


@functools.lru_cache(maxsize=None)
def _reference(spec, N, t, lim=2, cls="rough", steps=STEPS, rounded=False):
    """(oracle engine after ``steps`` steps, q0): computed once per case and
    shared by every kernel that runs it; never stepped again."""
    ref, q0 = _engine(spec, N, t, lim, cls, rounded=rounded)
    ref.step(steps)
    torch.cuda.synchronize()
    return ref, q0


def _check(ref, hip, q0, block, what, bound=BOUND):
    torch.cuda.synchronize()
    errs = increment_error(ref, hip, q0, block=block, what=what)      # raises on a NaN
    print(f"TOPO {what}: " + " ".join(f"{x:.2e}" for x in errs))
    increment_error(ref, hip, q0, bound=bound, block=block, what=what)
    return errs


def _name(spec):
    return spec[0] + "".join(f" {k}={v:g}" for k, v in spec[1])


# ---- block stage kernel -------------------------------------------------------------------
def _block_case(spec, N, t, lim, cls, block):
    ref, q0 = _reference(spec, N, t, lim, cls)
    hip, _ = _engine(spec, N, t, lim, cls, backend="hip", block=block, dt=ref.dt)
    assert bool((hip.tens["cgeo"][..., 4:7] != 0).any(-1).all())      # grad b in every cell record
    hip.step(STEPS)
    _check(ref, hip, q0, block, f"block {_name(spec)} {cls} limiter {lim} C{N} t={t} block {block[0]}x{block[1]}")


@pytest.mark.parametrize("N,t,block,lim", [
    (48, 1, (16, 16), 2), (48, 1, (16, 16), 4),    # full ten-wave blocks, cube corners
    (20, 1, (16, 16), 2),                          # partial blocks, block-wide fix-up
    (24, 2, (16, 8), 2), (24, 2, (16, 8), 4),      # tile corners with carried ghosts
    (24, 2, (8, 8), 2),
    (25, 1, (8, 8), 2), (33, 1, (16, 16), 2),      # a block ending one cell short of a panel edge
])
def test_block_kernel(N, t, block, lim):
    _block_case(TC5, N, t, lim, "rough", block)


# ---- streaming stage (64, R), both geometry paths -------------------------------------------
def _march_engine(monkeypatch, compact, spec, N, t, R, dt=None, dtype=torch.float64, rounded=False, lim=2,
                  loopback=None):
    """A streaming-stage engine on the chosen geometry path, asserted to be the
    path its launches take."""
    if compact is not None:
        monkeypatch.setenv("STSP_MARCH_COMPACT", "1" if compact else "0")
    else:
        monkeypatch.delenv("STSP_MARCH_COMPACT", raising=False)
        compact = dtype == torch.float64
    hip, q0 = _engine(spec, N, t, lim, "rough", backend="hip", dtype=dtype, block=(64, R), dt=dt, rounded=rounded,
                      loopback=loopback)
    hc = hip.compute
    assert hc.march and hc.march_geometry == ("compact" if compact else "records")
    if compact:
        bp = hc.mt["bpad"]
        assert bp is not None and bp.numel() == hip.plan.S and bp.dtype == dtype
        # the ghost ring of b is filled: no edge ghost of a tile is left at 0
        P, ng, n = hip.plan.P, hip.plan.ng, hip.plan.n
        ring = bp.view(hip.plan.T, P, P)
        assert bool((ring[:, ng:ng + n, ng:ng + n] != 0).all())
        assert bool((ring[:, :ng, ng:ng + n] != 0).all()) and bool((ring[:, ng + n:, ng:ng + n] != 0).all())
        assert bool((ring[:, ng:ng + n, :ng] != 0).all()) and bool((ring[:, ng:ng + n, ng + n:] != 0).all())
    else:
        assert hc.mt is None
    return hip, q0


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "records"])
@pytest.mark.parametrize("N,t,R", [(24, 1, 8), (72, 1, 16), (25, 1, 8), (50, 2, 4)])
def test_march(monkeypatch, N, t, R, compact):
    """One wave with both halo lanes panel-edge ghosts; two strips with a
    partial last strip; an odd tile; four rows per wave with tile edges inside
    the panels."""
    ref, q0 = _reference(TC5, N, t)
    hip, _ = _march_engine(monkeypatch, compact, TC5, N, t, R, dt=ref.dt)
    hip.step(STEPS)
    _check(ref, hip, q0, (64, R), f"march {'compact' if compact else 'records'} rough limiter 2 C{N} t={t} rows {R}")


def test_march_compact_agrees_with_records(monkeypatch):
    """grad b formed in the kernel from b against the oracle's grad b in the
    cell records: within 1e-12 of the increment."""
    a, q0 = _march_engine(monkeypatch, False, TC5, 48, 1, 16)
    b, _ = _march_engine(monkeypatch, True, TC5, 48, 1, 16, dt=a.dt)
    a.step(STEPS)
    b.step(STEPS)
    _check(a, b, q0, (64, 16), "march compact against records, rough limiter 2 C48 t=1 rows 16", bound=1e-12)


# ---- pipelined streaming step ----------------------------------------------------------------
def _march3_case(spec, N, R):
    from stsphere.ops.march3 import March3Step
    ref, q0 = _reference(spec, N, 1)
    hip, _ = _engine(spec, N, 1, backend="hip", dt=ref.dt)
    March3Step(hip, rows=R).step(STEPS)
    _check(ref, hip, q0, (64, R), f"march3 {_name(spec)} rough limiter 2 C{N} t=1 rows {R}")


@pytest.mark.parametrize("N,R", [(48, 16), (50, 32)])
def test_march3(N, R):
    _march3_case(TC5, N, R)


# ---- fused step --------------------------------------------------------------------------------
FUSED_SHAPES = [(12, 1, 6), (36, 2, 6), (32, 2, 8), (48, 4, 12), (48, 1, 16), (54, 1, 18), (60, 3, 20)]


def _fused_case(spec, N, t, B, lim, cls):
    from stsphere.ops.fused import FusedKernel
    ref, q0 = _reference(spec, N, t, lim, cls)
    hip, _ = _engine(spec, N, t, lim, cls, backend="hip", dt=ref.dt)
    fk = FusedKernel(hip, B=B)
    assert fk.plan.B == B and fk.tens["gbt"] is not None and bool((fk.tens["gbt"][:, :3] != 0).any())
    for _ in range(STEPS):
        fk.step(1)
    torch.cuda.synchronize()
    fk.check()
    _check(ref, hip, q0, (B, B), f"fused {_name(spec)} {cls} limiter {lim} C{N} t={t} B={B}")


@pytest.mark.parametrize("N,t,B", FUSED_SHAPES)
def test_fused(N, t, B):
    """One launch per step, one shape per block size."""
    _fused_case(TC5, N, t, B, 2, "rough")


@pytest.mark.parametrize("lim", [1, 3])
def test_fused_other_limiters(lim):
    _fused_case(TC5, 32, 2, 8, lim, "rough")


@pytest.mark.parametrize("cls", ["plateau", "zero_mom"])
def test_fused_exact_zero_differences(cls):
    _fused_case(TC5, 32, 2, 8, 2, cls)


@pytest.mark.parametrize("handoff", ["tag", "epoch"])
def test_fused_four_step_launch(monkeypatch, handoff):
    """Four steps in one launch equal four single-step launches bit for bit
    (both in-launch hand-off forms), and the oracle on the increment."""
    from stsphere.ops.fused import FusedKernel
    monkeypatch.setenv("STSP_FUSED_HANDOFF", handoff)
    ref, q0 = _reference(TC5, 32, 2, steps=4)
    a, _ = _engine(TC5, 32, 2, backend="hip", dt=ref.dt)
    b, _ = _engine(TC5, 32, 2, backend="hip", dt=ref.dt)
    FusedKernel(a).step(4)
    fk = FusedKernel(b)
    assert fk.handoff == handoff and fk.tens["gbt"] is not None
    fk.launch(0, nsteps=4)
    torch.cuda.synchronize()
    fk.check()
    assert torch.equal(a.pool[0], b.pool[0])
    _check(ref, b, q0, (fk.plan.B,) * 2, f"fused four-step launch ({handoff}) rough limiter 2 C32 t=2")


# ---- remote cells and ghosts of b ------------------------------------------------------------
def _loopback_stage_pair(a, b, what, q0, ref, block):
    """One-rank engine ``a`` against the loopback engine ``b`` stepped through
    the direct exchange: bitwise equal, ``a`` within the bound of the oracle."""
    from stsphere.ops.native_runtime import NativeStepper
    from stsphere.ops.xgmi import XgmiHalo
    xg = XgmiHalo(b, timeout_s=1.0)
    ns = NativeStepper(b, use_graph=True, steps_per_graph=4, xgmi=xg)
    try:
        a.step(STEPS)
        ns.run(STEPS)
        torch.cuda.synchronize()
        ns.check()
        assert torch.equal(a.tiles_view(), b.tiles_view())
        assert int(xg.epoch.min()) == int(xg.epoch.max()) >= STEPS * len(b.integ.stages)
    finally:
        ns.close()
        xg.close()
    _check(ref, a, q0, block, what)


def test_loopback_block_kernel():
    """Every ghost of the block kernel through the rank's own ring (the layout
    of tests/test_xgmi.py::test_xgmi_loopback_matches_single)."""
    ref, q0 = _reference(TC5, 24, 2)
    a, _ = _engine(TC5, 24, 2, backend="hip", dt=ref.dt)
    b, _ = _engine(TC5, 24, 2, backend="hip", dt=ref.dt, loopback="stage")
    block = (a.compute.bx, a.compute.by)
    assert not a.compute.march and (b.compute.bx, b.compute.by) == block
    _loopback_stage_pair(a, b, f"loopback block {block[0]}x{block[1]} rough limiter 2 C24 t=2 (one rank)", q0, ref, block)


@pytest.mark.parametrize("N,t", [(24, 2), (48, 1)])
def test_loopback_march(monkeypatch, N, t):
    """The streaming stage 64 x 4 on a loopback layout: every ghost of the
    state comes from the ring and every ghost of the b table from
    ``ghost_sources`` (the layout of
    tests/test_xgmi.py::test_xgmi_loopback_march_matches_single)."""
    ref, q0 = _reference(TC5, N, t)
    a, _ = _march_engine(monkeypatch, None, TC5, N, t, 4, dt=ref.dt)
    b, _ = _march_engine(monkeypatch, None, TC5, N, t, 4, dt=ref.dt, loopback="stage")
    assert torch.equal(a.compute.mt["bpad"], b.compute.mt["bpad"])
    _loopback_stage_pair(a, b, f"loopback march compact 64x4 rough limiter 2 C{N} t={t} (one rank)", q0, ref, (64, 4))


@pytest.mark.parametrize("handoff", ["tag", "epoch"])
def test_loopback_fused(monkeypatch, handoff):
    """The fused kernel on a loopback layout (the layout of
    tests/test_fused.py::test_fused_loopback_kernel_equals_one_rank): every
    ring cell's gbt row sits on the remote-slot index.  Two single steps and a
    two-step launch, bitwise equal to the one-rank kernel, which is within the
    bound of the oracle after the four steps."""
    from stsphere.ops.fused import FusedKernel
    monkeypatch.setenv("STSP_FUSED_HANDOFF", handoff)
    ref, q0 = _reference(TC5, 32, 2, steps=4)
    a, _ = _engine(TC5, 32, 2, backend="hip", dt=ref.dt)
    b, _ = _engine(TC5, 32, 2, backend="hip", dt=ref.dt, loopback="fused")
    fa = FusedKernel(a)
    fb = FusedKernel(b, B=fa.plan.B, timeout_s=1.0)
    try:
        assert fb.mem is not None and bool((fb.plan.src <= -2).any())
        S = b.plan.S
        assert fa.tens["gbt"].shape[0] == S and fb.tens["gbt"].shape[0] > S      # remote rows appended
        fa.step(2)
        fb.step(2)
        fa.launch(0, nsteps=2)
        fb.launch(0, nsteps=2)
        torch.cuda.synchronize()
        fb.check()
        assert torch.equal(a.tiles_view(), b.tiles_view())
    finally:
        fb.close()
    _check(ref, a, q0, (fa.plan.B,) * 2, f"loopback fused ({handoff}) rough limiter 2 C32 t=2 (one rank, four steps)")


@pytest.mark.parametrize("ranks", [2, 8])
def test_virtual_ranks_block_kernel(ranks):
    """Virtual ranks (grad b from each rank's own geometry, receive-buffer
    gather, interior / boundary block split) against the one-rank HIP engine,
    within 1e-12 of the field maximum (tests/test_rough_kernels.py::
    test_remote_ghost_path_on_rough); the one-rank engine against the oracle."""
    N, t = 24, 2
    ref, q0 = _reference(TC5, N, t)
    single, _ = _engine(TC5, N, t, backend="hip", dt=ref.dt)
    vc = VirtualCluster(lambda: TopographySWE("tc5"), TileLayout(N, t, ranks, ng=2), grid=grid_of(N), device="cuda",
                        backend="hip", dt=single.dt)
    for e in vc.engines:
        install(e, _global(TC5, N, "rough"))
    single.step(STEPS)
    vc.step(STEPS)
    torch.cuda.synchronize()
    a, b = global_of(single), global_of(vc.engines)
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    for f in range(4):
        d = float((a[f] - b[f]).abs().max())
        print(f"TOPO remote ghosts {ranks} ranks field {f}: {d / float(a[f].abs().max()):.2e} of the field maximum")
        assert d <= 1e-12 * max(1.0, float(a[f].abs().max())), f
    _check(ref, single, q0, (single.compute.bx, single.compute.by), f"virtual ranks {ranks}: one-rank block kernel C24 t=2")


# ---- derived fields ------------------------------------------------------------------------------
def test_derived_fields_over_the_topography():
    """DerivedFields against its PyTorch twin on C24 t=2 with the tolerances of
    tests/test_derived_gpu.py; the energy differs from the b = 0 energy of the
    same state by far more than its tolerance, so a dropped b would show."""
    from stsphere.models import derived as md
    N, t = 24, 2
    G = _global(TC5, N, "rough")
    L = TileLayout(N, t, 1, ng=2)
    cpu = Engine(TopographySWE("tc5"), L, grid=grid_of(N))
    install(cpu, G)
    fr, ir = (x.clone() for x in cpu.derived())
    flat = Engine(TopographySWE("tc5"), L, grid=grid_of(N))
    install(flat, G)
    flat.tens["b"] = torch.zeros_like(flat.tens["b"])
    e_flat = float(flat.derived()[1][md.INVARIANTS.index("energy")])
    hip = Engine(TopographySWE("tc5"), L, grid=grid_of(N), device="cuda", backend="hip", dt=cpu.dt)
    install(hip, G)
    f, inv = hip.derived()
    torch.cuda.synchronize()
    f, inv = f.double().cpu(), inv.cpu()
    fd = [float((f[k] - fr[k]).abs().max() / fr[k].abs().max()) for k in range(3)]
    a, b = dict(zip(md.INVARIANTS, inv.tolist())), dict(zip(md.INVARIANTS, ir.tolist()))
    idf = {k: abs(a[k] - b[k]) / abs(b[k]) for k in md.INVARIANTS if k != "circulation"}
    idf["circulation"] = abs(a["circulation"] - b["circulation"]) / b["abs_circulation"]
    share = abs(b["energy"] - e_flat) / abs(b["energy"])
    print(f"TOPO derived C24 t=2: fields {fd} inv {idf}; g h b share of the energy {share:.3e}")
    assert torch.isfinite(f).all()
    for k in range(3):
        assert fd[k] <= 1e-12, (md.FIELDS[k], fd[k])
    for k in ("mass", "energy", "potential_enstrophy", "abs_circulation", "circulation"):
        assert idf[k] <= 1e-12, (k, idf[k])
    assert idf["max_courant"] <= 1e-14
    assert share > 1e-3 and abs(a["energy"] - e_flat) / abs(b["energy"]) > 1e-3


# ---- other constants -----------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["block", "march", "march3", "fused"])
def test_other_constants(monkeypatch, family):
    """g = 11, omega = 5e-5 (every other test runs the defaults; the kernels
    take both as launch parameters)."""
    if family == "block":
        _block_case(OTHER, 24, 2, 2, "rough", (16, 16))
    elif family == "march":
        ref, q0 = _reference(OTHER, 24, 1)
        hip, _ = _march_engine(monkeypatch, None, OTHER, 24, 1, 8, dt=ref.dt)
        assert hip.compute._g == 11.0 and hip.compute._omega2 == 2 * 5e-5
        hip.step(STEPS)
        _check(ref, hip, q0, (64, 8), f"march compact {_name(OTHER)} rough limiter 2 C24 t=1 rows 8")
    elif family == "march3":
        _march3_case(OTHER, 48, 16)
    else:
        _fused_case(OTHER, 32, 2, 8, 2, "rough")


@pytest.mark.parametrize("family", ["block", "fused"])
def test_tc2_with_a_rotated_axis(family):
    """tc2 with alpha = pi / 4 (the flow crosses every panel edge obliquely)."""
    if family == "block":
        _block_case(TC2_TILTED, 24, 2, 2, "rough", (16, 16))
    else:
        _fused_case(TC2_TILTED, 32, 2, 8, 2, "rough")


# ---- rest stays at rest ----------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,t", [("block", 24, 2), ("march", 24, 1), ("march3", 48, 1), ("fused", 32, 2)])
def test_rest_stays_at_rest(family, N, t):
    """The lake at rest (h0 = 1000 m, no wind, no topography) for two steps:
    the pressure flux and the curvature balance cancel.  max |M| <= 1e-11 dt g
    h0^2 / 2 max(L / A), the project's fp64 bound on the largest single term
    that has to cancel (the oracle: 3.6e-16 of that scale); max |h - h0| <=
    1e-11 dt h0 sqrt(g h0) max(L / A) (the oracle: exactly 0)."""
    block = {"block": (16, 16), "march": (64, 8)}.get(family)
    hip = Engine(ShallowWater("rest"), TileLayout(N, t, 1, ng=2), grid=grid_of(N), device="cuda", backend="hip",
                 block=block)
    h0, g, dt = 1000.0, hip.physics.g, hip.dt
    assert bool((hip.tiles_view()[0] == h0).all()) and bool((hip.tiles_view()[1:] == 0).all())
    tn = hip.tens
    invA = tn["invA"].double()
    loa = max(float((tn["ex"].double()[..., :-1] * invA).max()), float((tn["ex"].double()[..., 1:] * invA).max()),
              float((tn["ey"].double()[:, :-1] * invA).max()), float((tn["ey"].double()[:, 1:] * invA).max()))
    if family == "march3":
        from stsphere.ops.march3 import March3Step
        March3Step(hip, rows=16).step(STEPS)
    elif family == "fused":
        from stsphere.ops.fused import FusedKernel
        fk = FusedKernel(hip, B=8)
        fk.step(STEPS)
        torch.cuda.synchronize()
        fk.check()
    else:
        hip.step(STEPS)
    torch.cuda.synchronize()
    q = hip.tiles_view().double()
    assert torch.isfinite(q).all()
    m_scale, h_scale = dt * g * h0 * h0 / 2 * loa, dt * h0 * math.sqrt(g * h0) * loa
    m, dh = float(q[1:4].abs().max()), float((q[0] - h0).abs().max())
    print(f"TOPO rest {family} C{N} t={t}: max |M| {m:.3e} = {m / m_scale:.2e} of dt g h0^2 / 2 max(L / A); "
          f"max |h - h0| {dh:.3e} = {dh / h_scale:.2e} of dt h0 sqrt(g h0) max(L / A)")
    assert m <= 1e-11 * m_scale and dh <= 1e-11 * h_scale


# ---- fp32 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,N,t", [("block", 24, 2), ("march", 24, 1), ("march-compact", 24, 1), ("march3", 48, 1),
                                        ("fused", 32, 2)])
def test_fp32(monkeypatch, family, N, t):
    """``march`` runs the per-tile records (the fp32 default), ``march-compact``
    the compact geometry."""
    ref, q0, twin, _ = fp32_twin_bound("topo", N, t, 2, "rough", "ssprk3", STEPS)
    if family.startswith("march") and family != "march3":
        hip, _ = _march_engine(monkeypatch, True if family == "march-compact" else None, TC5, N, t, 8, dt=ref.dt,
                               dtype=torch.float32, rounded=True)
        hip.step(STEPS)
        block = (64, 8)
    else:
        block = (16, 16) if family == "block" else None
        hip, _ = _engine(TC5, N, t, backend="hip", dtype=torch.float32, block=block, dt=ref.dt, rounded=True)
        if family == "march3":
            from stsphere.ops.march3 import March3Step
            March3Step(hip, rows=16).step(STEPS)
            block = (64, 16)
        elif family == "fused":
            from stsphere.ops.fused import FusedKernel
            fk = FusedKernel(hip)
            assert fk.tens["gbt"] is not None and fk.tens["gbt"].dtype == torch.float32
            fk.step(STEPS)
            torch.cuda.synchronize()
            fk.check()
            block = (fk.plan.B,) * 2
        else:
            hip.step(STEPS)
    print(f"TOPO fp32 twin C{N} t={t}: " + " ".join(f"{x:.2e}" for x in twin))
    _check(ref, hip, q0, block, f"fp32 {family} rough limiter 2 C{N} t={t}", bound=[4.0 * x for x in twin])
