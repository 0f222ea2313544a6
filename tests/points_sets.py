"""Point sets shared by tests/test_points.py and tests/test_points_gpu.py."""
import functools
import math

import numpy as np

from stsphere.models import latlon as ml
from stsphere.models.geometry import CubedSphereGrid
from stsphere.parallel.layout import TileLayout

# (N, tiles per edge): N - 1 = 7 is a short eid row; odd N puts the panel's centre
# lines through cell centres; 2 and 3 tiles per edge exercise the padded index map
SHAPES = [(8, 1), (12, 2), (9, 3), (24, 2)]
MARGIN = 1e-9
SEED = 7          # random points of every shape keep margin >= MARGIN (asserted)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def random_points(N, K=1000, seed=SEED):
    g = np.random.default_rng(seed + N).standard_normal((K, 3))
    return _unit(g)


@functools.lru_cache(maxsize=None)
def constructed(N):
    """Every cell centre, the midpoints of every pair of neighbouring centres
    (on dual grid lines), the 12 cube-edge lines at N + 1 points each, the 8
    cube corners, the 6 panel centres, both poles."""
    c = CubedSphereGrid(N).centers()
    flat = c.reshape(-1, 3)
    pts = [flat, _unit(c[:, :, :-1] + c[:, :, 1:]).reshape(-1, 3), _unit(c[:, :-1] + c[:, 1:]).reshape(-1, 3)]
    # neighbours across cube edges: a border cell and its layer-0 ghost source
    lay = TileLayout(N, 1, 1, ng=1)
    gs = lay.ghost_sources(0)[:, :, 0, :]
    pos = np.arange(N)
    for f in range(6):
        own = [lay.global_flat(f, 0, pos), lay.global_flat(f, N - 1, pos), lay.global_flat(f, pos, 0),
               lay.global_flat(f, pos, N - 1)]
        for s in range(4):
            pts.append(_unit(flat[own[s]] + flat[gs[f, s]]))
    th = np.tan(-0.25 * math.pi + np.arange(N + 1) * (0.5 * math.pi / N))
    for ax in range(3):
        a, b = (ax + 1) % 3, (ax + 2) % 3
        for sa in (-1.0, 1.0):
            for sb in (-1.0, 1.0):
                v = np.zeros((N + 1, 3))
                v[:, a], v[:, b], v[:, ax] = sa, sb, th
                pts.append(_unit(v))
    corners = np.array([[x, y, z] for x in (-1.0, 1.0) for y in (-1.0, 1.0) for z in (-1.0, 1.0)])
    pts += [_unit(corners), np.concatenate([np.eye(3), -np.eye(3)]), np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0]])]
    return np.ascontiguousarray(np.concatenate(pts))


@functools.lru_cache(maxsize=None)
def point_set(N):
    """Constructed points, then 1000 random ones; K is no multiple of 256."""
    p = np.concatenate([constructed(N), random_points(N)])
    if len(p) % 256 == 0:
        p = np.concatenate([p, random_points(N, 1, SEED + 1)])
    return np.ascontiguousarray(p)


def check_coverage(N, elem):
    """Interior quads of all six panels, edge quads of all twelve cube edges
    and all eight triangles are hit."""
    mesh = ml.DualMesh(N)
    nint, nq = mesh.nint, len(mesh.equad)
    inter = elem[elem < nint]
    assert set(np.unique(inter // (N - 1) ** 2)) == set(range(6))
    quads = np.unique(elem[(elem >= nint) & (elem < nint + nq)] - nint)
    face = mesh.equad[quads] // (N * N)
    edges = {tuple(sorted((int(a), int(b)))) for a, b in zip(face[:, 0], face[:, 2])}
    assert len(edges) == 12, edges
    assert set(np.unique(elem[elem >= nint + nq] - nint - nq)) == set(range(8))
