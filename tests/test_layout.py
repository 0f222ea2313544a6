"""Halo maps checked geometrically, independently of the map construction
(every ghost must hold the geometrically adjacent cell)."""
import numpy as np
import pytest

from stsphere.models.geometry import CubedSphereGrid
from stsphere.parallel.layout import TileLayout, corner_xy, ghost_xy


def _cell_vertex_sets(N):
    g = CubedSphereGrid(N, radius=1.0)
    v = g.vertices()
    key = {}
    ids = np.empty(v.shape[:3], dtype=np.int64)
    for idx in np.ndindex(*v.shape[:3]):
        k = tuple(np.round(v[idx], 9))
        ids[idx] = key.setdefault(k, len(key))
    assert len(key) == 6 * N * N + 2          # Euler: V = 6N^2 + 2
    cells = {}
    for f in range(6):
        for j in range(N):
            for i in range(N):
                cells[(f * N + j) * N + i] = frozenset((ids[f, j, i], ids[f, j, i + 1], ids[f, j + 1, i], ids[f, j + 1, i + 1]))
    return cells


def _adjacent(cells, a, b):
    return len(cells[a] & cells[b]) == 2


@pytest.mark.parametrize("N,t,ng", [(6, 1, 2), (8, 2, 3), (9, 3, 2), (4, 1, 3)])
def test_ghost_sources_are_geometric_neighbours(N, t, ng):
    L = TileLayout(N, t, 1, ng=ng)
    cells = _cell_vertex_sets(N)
    src = L.ghost_sources(0)   # [T,4,ng,n]
    n = L.n
    for li, tid in enumerate(L.rank_tiles[0]):
        f, I0, J0 = L.tile_origin(tid)
        for s in range(4):
            for p in range(n):
                # tile boundary cell adjacent to this side at position p
                x, y = ghost_xy(s, 0, np.array([p]), n)
                bx = min(max(int(x[0]), 0), n - 1)
                by = min(max(int(y[0]), 0), n - 1)
                inner = L.global_flat(f, I0 + bx, J0 + by)
                prev, prev2 = inner, None
                for k in range(ng):
                    c = int(src[li, s, k, p])
                    assert _adjacent(cells, c, prev), (tid, s, k, p)
                    assert c != prev2
                    if k >= 1:
                        assert not _adjacent(cells, c, inner)
                    if p + 1 < n:
                        assert _adjacent(cells, c, int(src[li, s, k, p + 1]))
                    prev2, prev = prev, c


@pytest.mark.parametrize("N,t,R", [(8, 2, 8), (12, 2, 4), (12, 1, 3), (8, 2, 2)])
def test_send_recv_lists_consistent(N, t, R):
    L = TileLayout(N, t, R, ng=2)
    for r in range(R):
        p = L.plan(r)
        for peer, off, cnt in zip(p.recv_peers, p.recv_offsets, p.recv_counts):
            q = L.plan(peer)
            k = q.send_peers.index(r)
            assert q.send_counts[k] == cnt
            # sender's cells (padded offsets -> global) are exactly what r needs, in order
            need = L.needs(r, peer)
            sent = q.send_idx[q.send_offsets[k]:q.send_offsets[k] + cnt]
            assert (L.local_flat(need) == sent).all()
        # every remote ghost references a valid slot
        gm = p.ghost_map
        assert ((-1 - gm[gm < 0]) < p.num_recv).all()


@pytest.mark.parametrize("N,t,R", [(8, 1, 1), (8, 2, 1), (12, 2, 8)])
def test_push_map_is_bijection_onto_local_ghosts(N, t, R):
    L = TileLayout(N, t, R, ng=2)
    for r in range(R):
        p = L.plan(r)
        pushed = p.push_map[p.push_map >= 0]
        assert len(np.unique(pushed)) == len(pushed) == (p.ghost_map >= 0).sum()
        # carried corner ghosts: pushed by their own table, once each
        cp = p.corner_push[p.corner_push >= 0]
        assert len(np.unique(cp)) == len(cp) == (p.corner_carried & (p.corner_map >= 0)).sum()
        allp = np.concatenate([pushed, cp])
        assert len(np.unique(allp)) == len(allp)
        assert set(allp.tolist()) == set(p.halo_dst.tolist())


@pytest.mark.parametrize("N,t,R,ng", [(12, 2, 1, 2), (24, 4, 1, 3), (24, 2, 6, 2), (24, 4, 8, 3)])
def test_corner_ghosts_carry_the_diagonal_strip_cells(N, t, R, ng):
    """Carried corner ghosts: exactly the quadrants with one panel-edge side,
    each slot's source is the true neighbour-panel cell at that extended
    position (tile_extended_index), and every remote one has a receive slot
    whose sender packs that cell."""
    L = TileLayout(N, t, R, ng=ng)
    n = L.n
    for r in range(R):
        p = L.plan(r)
        cs = L.corner_sources(r)
        for li, tid in enumerate(p.tiles):
            f, I0, J0 = L.tile_origin(tid)
            ext = L.tile_extended_index(tid, ng)
            for q in range(4):
                xe = (I0 + n == N) if q & 1 else (I0 == 0)
                ye = (J0 + n == N) if q & 2 else (J0 == 0)
                assert p.corner_carried[li, q].all() == (xe != ye)
                assert p.corner_carried[li, q].any() == (xe != ye)
                for a in range(ng):
                    for b in range(ng):
                        x = n + b if q & 1 else -1 - b
                        y = n + a if q & 2 else -1 - a
                        if xe != ye:
                            assert cs[li, q, a, b] == ext[y + ng, x + ng] >= 0
        rc = p.remote_corners()
        if rc.any():
            slots = -1 - p.corner_map[rc]
            assert (slots < p.num_recv).all()
            for s, c in zip(slots, cs[rc]):
                k = int(np.searchsorted(np.asarray(p.recv_offsets), s, side="right")) - 1
                peer = p.recv_peers[k]
                assert L.needs(r, peer)[s - p.recv_offsets[k]] == c


def test_block_classes_partition_all_blocks():
    L = TileLayout(64, 2, 8, ng=2)
    p = L.plan(0)
    inter, bnd = p.block_classes(16, 16)
    allb = np.sort(np.concatenate([inter, bnd]))
    assert (allb == np.arange(p.T * 2 * 2)).all() and len(bnd) > 0 and len(inter) > 0


PPM_BLOCKS = [(16, 16), (16, 8), (8, 16), (32, 8)]
WINDOW_LAYOUTS = [(24, 2, 4, False), (34, 1, 2, False), (36, 2, 8, False), (48, 1, 6, False), (36, 3, 6, False),
                  (24, 2, 1, True)]
# interior blocks over all ranks, 16 x 16 blocks, counted by hand from the geometry:
# (34,1,2): blocks at 0, 16, 32; the window of block 1 spans 13 .. 34 with three layers
# (reaches the far strip) and 14 .. 33 with two (does not)
INTERIOR_16x16 = {(34, 1, 2, 3): 12, (48, 1, 6, 3): 6, (24, 2, 4, 3): 0, (24, 2, 4, 2): 0, (48, 1, 6, 2): 6}


def _window_reads_remote(plan, t, x0, y0, bx, by, ng, corners):
    """The stage kernel's window of one block, cell by cell, bounded as its
    loader bounds it (x < n + ng and y < n + ng): does any cell come out of
    the receive buffer?"""
    n = plan.n
    for Y in range(y0 - ng, min(y0 + by + ng, n + ng)):
        for X in range(x0 - ng, min(x0 + bx + ng, n + ng)):
            ox, oy = X < 0 or X >= n, Y < 0 or Y >= n
            if ox and oy:
                if (X, Y) in corners:
                    return True
            elif ox:
                if plan.ghost_map[t, 0 if X < 0 else 1, -1 - X if X < 0 else X - n, Y] < 0:
                    return True
            elif oy:
                if plan.ghost_map[t, 2 if Y < 0 else 3, -1 - Y if Y < 0 else Y - n, X] < 0:
                    return True
    return False


@pytest.mark.parametrize("bx,by", PPM_BLOCKS)
@pytest.mark.parametrize("N,t,R,loop", WINDOW_LAYOUTS)
@pytest.mark.parametrize("ng", [2, 3])
def test_block_classes_match_the_window_replay(ng, N, t, R, loop, bx, by):
    """Every block whose (bx + 2 ng) x (by + 2 ng) window touches a remote strip
    cell or a remote carried corner waits for the exchange (boundary class);
    a block that touches neither is not held back (interior class)."""
    L = TileLayout(N, t, R, ng=ng, loopback=loop)
    n = L.n
    nbx, nby = -(-n // bx), -(-n // by)
    ninterior = 0
    for r in range(R):
        plan = L.plan(r)
        inter, bnd = plan.block_classes(bx, by)
        assert (np.sort(np.concatenate([inter, bnd])) == np.arange(plan.T * nbx * nby)).all()
        bnd = set(bnd.tolist())
        rc = plan.remote_corners()
        free = 0
        for tl in range(plan.T):
            q, a, b = np.nonzero(rc[tl])
            corners = set(zip(*(v.tolist() for v in corner_xy(q, a, b, n))))
            for yb in range(nby):
                for xb in range(nbx):
                    bid = (tl * nby + yb) * nbx + xb
                    if _window_reads_remote(plan, tl, xb * bx, yb * by, bx, by, ng, corners):
                        assert bid in bnd, (r, tl, yb, xb)
                    else:
                        free += 1
        assert (len(inter) > 0) == (free > 0) and len(inter) <= free, (r, len(inter), free)
        ninterior += len(inter)
    if (bx, by) == (16, 16) and (N, t, R, ng) in INTERIOR_16x16:
        assert ninterior == INTERIOR_16x16[(N, t, R, ng)]
