"""Host-side index math of the direct xGMI halo (ops/xgmi.py), on CPU.

The data flow of one stage is simulated with numpy: every rank's cells carry
their global id.  Each rank applies its remote push entries into the
receivers' rings.  Then every remote ghost slot of every rank must hold
exactly the cell the geometry says (``ghost_sources``).  The counters' producer
counts and the per-block wait/feed masks are checked against the same
simulation.
"""
import numpy as np
import pytest

from stsphere.ops.xgmi import SLOT_BITS, XgmiPlan, _side_cell
from stsphere.parallel.layout import TileLayout, corner_xy

CASES = [(16, 2, 2, False), (24, 2, 4, False), (16, 2, 8, False), (12, 1, 6, False), (20, 1, 3, False),
         (16, 2, 1, True), (40, 2, 8, False), (36, 3, 6, False)]


def _id(c):
    return "-".join(map(str, c))


# every case with two ghost layers (bare ids) and with the three of PPM: a third
# strip layer and 3 x 3 carried corners in the push tables, the ring and the masks
CASES_NG = [pytest.param(*c, 2, id=_id(c)) for c in CASES] + [pytest.param(*c, 3, id=_id(c) + "-ng3") for c in CASES]
# tiles of 18 and 34 cells: a 16-wide block reaches the far ghost strip only with window layer 3
LAYER3 = [(36, 2, 8, False), (34, 1, 2, False)]
# one or two tiles per rank: the diagonal tile behind a carried corner belongs to a rank
# that feeds neither strip of the block, so only the corner ghosts put that peer into the mask
CORNER_PEER = [(24, 2, 12, False), (24, 2, 24, False)]
PPM_BLOCKS = [(16, 16), (16, 8), (8, 16), (32, 8)]
# (N, t, R, loop, halo, ng, bx, by): halo 1 and 2 on 16 x 16, halo 3 on every block shape PPM can run
WINDOW_CASES = [pytest.param(*c, h, 2, 16, 16, id=f"{h}-{_id(c)}") for h in (1, 2) for c in CASES] + \
               [pytest.param(*c, 2, 2, 16, 16, id=f"2-{_id(c)}") for c in CORNER_PEER] + \
               [pytest.param(*c, 3, 3, bx, by, id=f"3-{_id(c)}-{bx}x{by}")
                for c in CASES + LAYER3 + CORNER_PEER for bx, by in PPM_BLOCKS]


def _plans(N, t, R, loop, bx=16, by=16, halo=2, ng=2):
    L = TileLayout(N, t, R, ng=ng, loopback=loop)
    return L, {r: XgmiPlan(L, r, bx, by, halo) for r in range(R)}


@pytest.mark.parametrize("N,t,R,loop,ng", CASES_NG)
def test_every_remote_ghost_delivered(N, t, R, loop, ng):
    L, xp = _plans(N, t, R, loop, halo=ng, ng=ng)
    assert all(x.push.shape[2] == ng and x.cpush.shape[2:] == (ng, ng) for x in xp.values())
    n = L.n
    ring_slots = xp[0].ring_slots
    assert all(x.ring_slots == ring_slots for x in xp.values())
    rings = {r: np.full(ring_slots, -1, dtype=np.int64) for r in range(R)}
    for r, x in xp.items():
        rem = x.push < -1
        code = (-2 - x.push[rem]).astype(np.int64)
        peer, slot = code >> SLOT_BITS, code & ((1 << SLOT_BITS) - 1)
        li, s2, kk, pp = np.nonzero(rem)
        i, j = _side_cell(s2, kk, pp, n)
        tiles = np.asarray(x.plan.tiles)[li]
        gid = np.empty(len(li), dtype=np.int64)
        for k, tid in enumerate(tiles):
            f, I0, J0 = L.tile_origin(int(tid))
            gid[k] = L.global_flat(f, I0 + i[k], J0 + j[k])
        for p, s, gval in zip(peer, slot, gid):
            assert rings[p][s] in (-1, gval), "two different cells pushed into one ring slot"
            rings[p][s] = gval
        want = set(zip(L.local_flat(gid).tolist(), code.tolist()))
        # carried corner ghosts (panel-edge strip ends): their own push table
        crem = x.cpush < -1
        ccode = (-2 - x.cpush[crem]).astype(np.int64)
        cpeer, cslot = ccode >> SLOT_BITS, ccode & ((1 << SLOT_BITS) - 1)
        cli, cq, ca, cb = np.nonzero(crem)
        ci = np.where(cq & 1, n - 1 - cb, cb)
        cj = np.where(cq & 2, n - 1 - ca, ca)
        for k in range(len(cli)):
            f, I0, J0 = L.tile_origin(int(x.plan.tiles[cli[k]]))
            gval = L.global_flat(f, I0 + ci[k], J0 + cj[k])
            assert rings[cpeer[k]][cslot[k]] in (-1, gval), "two different cells pushed into one ring slot"
            rings[cpeer[k]][cslot[k]] = gval
            want.add((int(L.local_flat(np.array([gval]))[0]), int(ccode[k])))
        # prime entries = the distinct (source cell, destination) pairs of both push tables
        assert len(x.prime_src) == len(np.unique(np.stack([x.prime_src, x.prime_code], 1), axis=0))
        pairs = set(zip(x.prime_src.tolist(), x.prime_code.tolist()))
        assert pairs == want
    ncorner = 0
    for p in range(R):
        pl = L.plan(p)
        gm = pl.ghost_map
        gs = L.ghost_sources(p)
        m = gm < 0
        assert (rings[p][-1 - gm[m]] == gs[m]).all()
        rc = pl.remote_corners()
        ncorner += int(rc.sum())
        assert (rings[p][-1 - pl.corner_map[rc]] == L.corner_sources(p)[rc]).all()
    if t > 1 and R > 1 and not loop:
        assert ncorner > 0 or R <= 2


@pytest.mark.parametrize("N,t,R,loop,ng", CASES_NG)
def test_producer_counts_match_feed_masks(N, t, R, loop, ng):
    L, xp = _plans(N, t, R, loop, halo=ng, ng=ng)
    for r in range(R):
        for p in range(R):
            feeds = int(((xp[p].bmask[:, 1].astype(np.int64) >> r) & 1).sum())
            assert xp[r].nprod[p] == feeds, (r, p)


def _window_needs(x, n, halo):
    """Per block: the peers whose ring slots the kernel's window loop (REMOTE
    branch) reads: remote strip cells, and the carried remote corner ghosts
    among the cells outside in both x and y.  Returns (all of them, those of
    the strip cells alone), one mask per block each."""
    bx, by = x.bx, x.by
    plan = x.plan
    gm = plan.ghost_map
    slot_peer = np.full(max(plan.num_recv, 1), -1)
    for p, off, cnt in zip(plan.recv_peers, plan.recv_offsets, plan.recv_counts):
        slot_peer[off:off + cnt] = p
    rc = plan.remote_corners()
    corner_slot = []            # per tile: (x, y) of a carried remote corner ghost -> its receive slot
    for t in range(plan.T):
        q, a, b = np.nonzero(rc[t])
        cx, cy = corner_xy(q, a, b, n)
        corner_slot.append({(int(u), int(v)): -1 - int(m) for u, v, m in zip(cx, cy, plan.corner_map[t, q, a, b])})
    needs, strips = [], []
    for bid in range(x.nblocks):
        tile, rem = divmod(bid, x.nbx * x.nby)
        yb, xb = divmod(rem, x.nbx)
        x0, y0 = xb * bx, yb * by
        need = strip = 0
        for ly in range(by + 2 * halo):
            for lx in range(bx + 2 * halo):
                X, Y = x0 + lx - halo, y0 + ly - halo
                if not (X < n + halo and Y < n + halo):
                    continue
                ox, oy = (X < 0) or (X >= n), (Y < 0) or (Y >= n)
                if ox and oy:
                    slot = corner_slot[tile].get((X, Y))
                    if slot is not None:
                        need |= 1 << int(slot_peer[slot])
                    continue
                if ox == oy:
                    continue
                if X < 0:
                    s, k, pos = 0, -1 - X, Y
                elif X >= n:
                    s, k, pos = 1, X - n, Y
                elif Y < 0:
                    s, k, pos = 2, -1 - Y, X
                else:
                    s, k, pos = 3, Y - n, X
                m = gm[tile, s, k, pos]
                if m < 0:
                    strip |= 1 << int(slot_peer[-1 - m])
        needs.append(need | strip)
        strips.append(strip)
    return needs, strips


@pytest.mark.parametrize("N,t,R,loop,halo,ng,bx,by", WINDOW_CASES)
def test_wait_masks_cover_every_window_read(N, t, R, loop, halo, ng, bx, by):
    """Replays the kernel's window loop (REMOTE branch) for every block."""
    L, xp = _plans(N, t, R, loop, bx, by, halo, ng)
    ncorner = corner_only = 0
    for r, x in xp.items():
        for bid, (need, strip) in enumerate(zip(*_window_needs(x, L.n, halo))):
            assert (int(x.bmask[bid, 0]) & need) == need, (r, bid)
            corner_only += need != strip
        ncorner += int(x.plan.remote_corners().sum())
    if t > 1 and R > 2 and not loop:
        assert ncorner > 0          # the corner branch of the replay ran
    if (N, t, R, loop) in CORNER_PEER:
        assert corner_only > 0      # ... and some block waits for a peer because of a corner ghost alone


def test_single_rank_needs_nothing():
    L, xp = _plans(24, 2, 1, False)
    x = xp[0]
    assert (x.bmask == 0).all() and (x.push >= -1).all() and x.prime_src.size == 0
