"""Face task tables of the fused step's table-driven builds (ops/fused.py::
face_table / face_tables, read by ops/csrc/fused_step.hip): a shared face takes
the limited slope of its upper cell from the next lane of its wave, so the
tables must put the right task into that lane, keep faces next to a panel-edge
line out of shared passes, and cover every stage's face set exactly once."""
import numpy as np
import pytest

from stsphere.models.geometry import CubedSphereGrid
from stsphere.ops.fused import (FT_FULL, FT_IDLE, FT_MIN_RUN, FT_SHARED, FT_SLOPE, FusedPlan, block_class,
                                class_edge_lines, face_table, face_tables, ft_unpack, fused_threads,
                                stage_face_coords, table_pass_cap)
from stsphere.parallel.layout import TileLayout

PLANS = [(24, 1, 6), (24, 1, 8), (48, 1, 16)]
_plans = {}


def _plan(N, t, B):
    if (N, t, B) not in _plans:
        P = FusedPlan(TileLayout(N, t, 1, ng=2), 0, CubedSphereGrid(N), B=B, ns=3)
        flags = np.array([sum(1 << int(r) for r in np.unique(P.reg[b]) if r >= 0) for b in range(P.nb)])
        _plans[(N, t, B)] = (P, flags)
    return _plans[(N, t, B)]


def _near(B, cls, ax, k):
    lines = class_edge_lines(B, cls)
    return any(abs(int(k) - e) <= 1 for e in lines[int(ax)])


@pytest.mark.parametrize("N,t,B", PLANS)
def test_class_edge_lines_are_the_blocks_edge_lines(N, t, B):
    """The class of a block fixes where its panel-edge lines lie in the window
    (the kernel's kx0 / kx1 / ky0 / ky1)."""
    P, flags = _plan(N, t, B)
    assert len(set(block_class(f) for f in flags)) == 9
    for b in range(P.nb):
        X0, Y0 = int(P.org[b, 0]), int(P.org[b, 1])
        kx = [k for f_, k in ((2, -X0), (4, N - X0)) if flags[b] & f_]
        ky = [k for f_, k in ((8, -Y0), (16, N - Y0)) if flags[b] & f_]
        assert (kx, ky) == tuple(class_edge_lines(B, block_class(flags[b])))


@pytest.mark.parametrize("N,t,B", PLANS)
def test_shared_tables(N, t, B):
    P, flags = _plan(N, t, B)
    coords = stage_face_coords(B)
    nshared = 0
    for cls in sorted(set(block_class(f) for f in flags)):
        tabs = face_table(B, cls, share=True)
        assert sum(len(e) // 64 for e, _, _ in tabs) <= table_pass_cap(B)
        for s_, (ent, nm, sm) in enumerate(tabs):
            ax, k, p, kind = ft_unpack(ent)
            npass = len(ent) // 64
            assert len(ent) % 64 == 0 and npass <= 32
            # the flux tasks are the stage's face set, each face once
            flux = (kind == FT_SHARED) | (kind == FT_FULL)
            got = sorted(zip(ax[flux].tolist(), k[flux].tolist(), p[flux].tolist()))
            want = sorted(zip(*(x.tolist() for x in coords[s_])))
            assert got == want, (cls, s_)
            run = 0
            for t_ in range(len(ent)):
                q = t_ // 64
                sh = (sm >> q) & 1
                if kind[t_] == FT_SHARED:
                    nshared += 1
                    # the next lane of the same pass holds the upper cell's slope
                    assert t_ % 64 != 63 and sh
                    assert kind[t_ + 1] in (FT_SHARED, FT_SLOPE)
                    assert (ax[t_ + 1], k[t_ + 1], p[t_ + 1]) == (ax[t_], k[t_] + 1, p[t_])
                    assert not _near(B, cls, ax[t_], k[t_])
                    run += 1
                else:
                    if kind[t_] == FT_SLOPE:
                        assert sh and run >= FT_MIN_RUN       # closes a run of at least three faces
                    else:
                        assert run == 0                       # a run ends in its slope-only lane
                    run = 0
                if kind[t_] == FT_FULL:
                    assert not sh
                    if _near(B, cls, ax[t_], k[t_]):
                        assert (nm >> q) & 1
            assert run == 0
            assert nm >> npass == 0 and sm >> npass == 0 and nm & sm == 0
            # idle and slope-only lanes too read window cells only: k - 2 .. k of row p
            assert k.min() >= 2 and k.max() <= P.d.W - 1 and p.min() >= 0 and p.max() <= P.d.W - 1
    assert nshared > 0


@pytest.mark.parametrize("N,t,B", PLANS)
@pytest.mark.parametrize("share", [True, False])
def test_schedule_runs_every_pass_on_one_wave(N, t, B, share):
    P, flags = _plan(N, t, B)
    edge = flags != 1
    G = P.gtab.shape[1]
    ftab, sched, classes = face_tables(B, flags, np.asarray(P.ccnt), edge, G, share=share)
    nw = fused_threads(B) // 64
    assert ftab.shape == (len(classes), 64 * table_pass_cap(B)) and sched.shape == (P.nb, 3, 20)
    for b in range(P.nb):
        cls = block_class(flags[b])
        assert classes[int(sched[b, 0, 19])] == cls
        tabs = face_table(B, cls, share=share)
        for s_, (ent, nm, sm) in enumerate(tabs):
            npass = len(ent) // 64
            assert npass <= 32
            waves = sched[b, s_, :16]
            assert not waves[nw:].any()
            assert int(np.bitwise_or.reduce(waves)) == (1 << npass) - 1
            assert sum(bin(int(x)).count("1") for x in waves) == npass      # no pass twice
            assert (int(sched[b, s_, 16]), int(sched[b, s_, 17])) == (nm, sm)
            o = 64 * int(sched[b, s_, 18])
            assert (ftab[int(sched[b, s_, 19]), o:o + len(ent)] == ent).all()


@pytest.mark.parametrize("N,t,B", PLANS)
def test_share_off_is_the_arithmetic_order(monkeypatch, N, t, B):
    """STSP_FUSED_SHARE=0: slot t of stage s is the full face that
    stage_face_coords gives for task t, no pass is shared, and the near passes
    are those of near_pass_masks."""
    from stsphere.ops.fused import near_pass_masks
    monkeypatch.setenv("STSP_FUSED_SHARE", "0")
    P, flags = _plan(N, t, B)
    coords = stage_face_coords(B)
    nm_legacy = near_pass_masks(B, P.org, flags, N)
    for b in range(P.nb):
        tabs = face_table(B, block_class(flags[b]))
        for s_, (ent, nm, sm) in enumerate(tabs):
            ax, k, p, kind = ft_unpack(ent)
            n = len(coords[s_][0])
            assert len(ent) == 64 * -(-n // 64) and sm == 0
            assert (kind[:n] == FT_FULL).all() and (kind[n:] == FT_IDLE).all()
            assert (ax[:n] == coords[s_][0]).all() and (k[:n] == coords[s_][1]).all() and (p[:n] == coords[s_][2]).all()
            assert nm == int(nm_legacy[b, s_])
