"""Point sampling and Lagrangian particles of an engine (models/points.py).

``PointSampler(engine)`` owns the mesh tables of the engine's grid and the
rank's two cell maps (padded state [F, T P P]; unpadded [C, T, n, n] as
``DerivedFields.compute`` returns) and fills the kernel descriptor of each
launch.  ``Particles(engine, p, interval)`` holds the particle state (x, xs, v0,
[K, 3] float64 on the engine's device) and advances it.  With ``backend='hip'``
on a GPU every step is an ordinary launch of ``ops/csrc/points_kernel.hip`` on
the caller's stream; with ``backend='torch'``, or on a CPU device, they run the
twin.  No ghost slot is ever read, so both work right after a fused launch.

One rank:   ``fields(p)``, ``tiles(p, x)``, ``velocity(p)`` -> [C, K] float64;
            ``Particles.start()``, ``advance()`` (one fused launch).
Several:    every rank's ``...(terms=True)`` [C, 4, K] (0 where the rank does
            not own the source), the arrays added (one rank owns each term:
            exact), then ``Particles.apply(stage, sum)`` on every rank, which
            folds the terms in the one-rank association.

All shape, alignment and range contracts the kernel relies on are checked
here, on the host, before anything is launched.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from ..models import points as mp
from .common import MAX_K, assert_interior, use_hip

CORRECTOR, PREDICTOR = 0, 1

_TABLES: Dict[int, mp.PointTables] = {}


def tables_for(N: int) -> mp.PointTables:
    if N not in _TABLES:
        if len(_TABLES) >= 8:
            _TABLES.pop(next(iter(_TABLES)))
        _TABLES[N] = mp.PointTables(N)
    return _TABLES[N]


class PointSampler:
    def __init__(self, engine):
        e = self.e = engine
        plan = e.plan
        N = self.N = e.layout.N
        if N < 2:
            raise ValueError("point sampling needs N >= 2")
        tab = self.tab = tables_for(N)
        pad, unp = mp.rank_maps(e.layout, e.rank)
        self.S = plan.S
        self.cells = plan.T * plan.n * plan.n
        self.pad_np, self.unp_np = pad, unp
        self.hip = use_hip(e)
        # ---- host-side contract checks ------------------------------------------
        nb = 12 * (N - 1) + 8
        assert tab.eid.shape == (6, 4, N - 1) and tab.eid.min() >= 0 and tab.eid.max() < tab.nq == nb - 8
        assert tab.bcell.shape == (nb, 4) and tab.bcell.max() < tab.ncell and tab.bcell[:, :3].min() >= 0
        assert (tab.bcell[:tab.nq, 3] >= 0).all() and (tab.bcell[tab.nq:, 3] == -1).all()
        assert tab.ctri.shape == (6, 4) and tab.ctri.min() >= 0 and tab.ctri.max() < 8
        assert tab.bctr.shape == (nb, 4, 3) and tab.bctr.dtype == np.float64 and np.isfinite(tab.bctr).all()
        for m, lim in ((pad, self.S), (unp, self.cells)):
            assert m.dtype == np.int32 and m.shape == (tab.ncell,) and m.min() >= -1 and m.max() < lim
        # the padded map addresses interior cells only (a ghost slot is never a source)
        assert_interior(plan, pad)
        if self.hip:
            from . import native
            self.lib = native.require_native()
            self.dcode = native.dtype_code(e.dtype)
            t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=e.device)
            self.d_eid, self.d_bcell, self.d_ctri, self.d_bctr = t(tab.eid), t(tab.bcell), t(tab.ctri), t(tab.bctr)
            self.d_pad, self.d_unp = t(pad), t(unp)
            for a in (self.d_eid, self.d_bcell, self.d_ctri, self.d_pad, self.d_unp):
                assert a.dtype == torch.int32 and a.is_contiguous() and a.data_ptr() % 4 == 0
            assert self.d_bctr.dtype == torch.float64 and self.d_bctr.is_contiguous() and self.d_bctr.data_ptr() % 8 == 0

    # ---- points ----------------------------------------------------------------------
    def points(self, p) -> torch.Tensor:
        """p [K, 3] (array or tensor) as a contiguous float64 tensor on the device."""
        p = torch.as_tensor(p, dtype=torch.float64).to(self.e.device).contiguous()
        if p.dim() != 2 or p.shape[1] != 3 or p.shape[0] < 1:
            raise ValueError(f"points [K, 3] with K >= 1 expected, not {tuple(p.shape)}")
        if p.shape[0] > MAX_K:
            raise ValueError(f"{p.shape[0]} points exceed the launch limit {MAX_K}")
        return p

    # ---- kernel ----------------------------------------------------------------------
    def _desc(self, Q: torch.Tensor, padded: bool, K: int):
        from . import native
        lim = self.S if padded else self.cells
        e = self.e
        assert Q.dim() == 2 and Q.shape[1] == lim and Q.is_contiguous() and Q.dtype == e.dtype and Q.is_cuda
        assert 1 <= K <= MAX_K
        d = native.PointsDesc()
        d.Q, d.cmap = native.ptr(Q), native.ptr(self.d_pad if padded else self.d_unp)
        d.eid, d.bcell, d.ctri, d.bctr = (native.ptr(self.d_eid), native.ptr(self.d_bcell), native.ptr(self.d_ctri),
                                          native.ptr(self.d_bctr))
        d.cs = d.lim = lim
        d.da = 0.5 * math.pi / self.N
        d.K, d.N = K, self.N
        return d

    def _run(self, d, what: str) -> None:
        from . import native
        native.check(self.lib.stsp_points_launch(self.dcode, d, native.current_stream_handle(self.e.device)), what)

    def _sample(self, p: torch.Tensor, Q: torch.Tensor, padded: bool, velocity: bool, terms: bool, elem: bool):
        from . import native
        p = self.points(p)
        K = p.shape[0]
        if velocity and Q.shape[0] < 4:
            raise ValueError("the velocity needs the shallow-water state (h, M)")
        if velocity:
            Q = Q[:4]      # (h, M): a contiguous view (tracer fields follow them)
        C = 3 if velocity else Q.shape[0]
        if self.hip:
            out = torch.empty((C, 4, K) if terms else (C, K), dtype=torch.float64, device=self.e.device)
            el = torch.empty(K, dtype=torch.int32, device=self.e.device) if elem else None
            d = self._desc(Q, padded, K)
            d.p, d.out, d.elem = native.ptr(p), native.ptr(out), native.ptr(el)
            d.C, d.velocity, d.terms, d.mode = C, int(velocity), int(terms), 0
            self._run(d, "points sample kernel")
            return (out, el) if elem else out
        loc = mp.locate(self.N, p, self.pad_np if padded else self.unp_np, self.tab.mesh, self.e.device)
        t = mp.velocity_terms(Q, loc) if velocity else mp.sample_terms(Q, loc)
        out = t if terms else mp.fold_terms(t)
        return (out, torch.as_tensor(loc.elem.astype(np.int32), device=self.e.device)) if elem else out

    # ---- this rank's samples: [C, K], or the terms [C, 4, K] ------------------------------
    def fields(self, p, q: Optional[torch.Tensor] = None, terms: bool = False, elem: bool = False):
        """Every channel of the padded state ``q`` [F, S] (default: the engine's)."""
        q = self.e.state if q is None else q
        return self._sample(p, q, True, False, terms, elem)

    def tiles(self, p, x: torch.Tensor, terms: bool = False, elem: bool = False):
        """The channels of an unpadded array ``x`` [C, T, n, n]."""
        return self._sample(p, x.reshape(x.shape[0], -1).contiguous(), False, False, terms, elem)

    def velocity(self, p, q: Optional[torch.Tensor] = None, terms: bool = False, elem: bool = False):
        """The Cartesian velocity [3, K] of the padded shallow-water state."""
        q = self.e.state if q is None else q
        return self._sample(p, q, True, True, terms, elem)


class Particles:
    """K particles carried by the engine's shallow-water flow (Heun's scheme,
    models/points.py), step ``interval * engine.dt``."""

    def __init__(self, engine, p, interval: int = 1):
        if int(interval) != interval or interval < 1:
            raise ValueError(f"particles: interval must be a positive integer, not {interval!r}")
        if engine.physics.name != "swe":
            raise ValueError(f"particles are carried by the shallow-water model, not {engine.physics.name!r}")
        self.e = engine
        self.interval = int(interval)
        self.sampler: PointSampler = engine.points()
        x = self.sampler.points(mp.check_seeds(p))
        self.K = x.shape[0]
        self.st = mp.ParticleState(x, x.clone(), torch.zeros_like(x))
        self.radius = float(engine.grid.radius)

    @property
    def dtp(self) -> float:
        return self.interval * self.e.dt

    @property
    def x(self) -> torch.Tensor:
        return self.st.x

    def set_positions(self, p) -> None:
        """Replace the positions (restore); ``start()`` must follow."""
        x = self.sampler.points(p)
        if x.shape[0] != self.K:
            raise ValueError(f"particles: {x.shape[0]} positions for {self.K} particles")
        self.st.x.copy_(x)

    # ---- pieces (several ranks) -------------------------------------------------------------
    def sample(self, stage: int, terms: bool = False, q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Velocity at xs (corrector) or x (predictor) from this rank's cells."""
        return self.sampler.velocity(self.st.xs if stage == CORRECTOR else self.st.x, q, terms=terms)

    def apply(self, stage: int, vel: torch.Tensor) -> None:
        """The corrector / predictor move from the summed velocity [3, K] or terms [3, 4, K]."""
        terms = vel.dim() == 3
        assert vel.shape == ((3, 4, self.K) if terms else (3, self.K)) and vel.dtype == torch.float64
        s = self.sampler
        if s.hip and vel.is_cuda:
            from . import native
            vel = vel.contiguous()
            d = native.PointsDesc()
            d.vel, d.x, d.xs, d.v0 = native.ptr(vel), native.ptr(self.st.x), native.ptr(self.st.xs), native.ptr(self.st.v0)
            d.K, d.N, d.terms, d.mode, d.stage = self.K, s.N, int(terms), 1, int(stage)
            d.radius, d.dtp = self.radius, self.dtp
            s._run(d, "points advance kernel")
        elif stage == CORRECTOR:
            mp.corrector(self.st, vel.to(self.st.x.device), self.dtp, self.radius)
        else:
            mp.predictor(self.st, vel.to(self.st.x.device), self.dtp, self.radius)

    # ---- one rank ---------------------------------------------------------------------------
    def start(self, q: Optional[torch.Tensor] = None) -> None:
        self.apply(PREDICTOR, self.sample(PREDICTOR, q=q))

    def advance_sequenced(self, q: Optional[torch.Tensor] = None, terms: bool = False) -> None:
        self.apply(CORRECTOR, self.sample(CORRECTOR, terms, q))
        self.apply(PREDICTOR, self.sample(PREDICTOR, terms, q))

    def advance(self, q: Optional[torch.Tensor] = None) -> None:
        """One advance of a rank that owns every cell: one fused launch."""
        s = self.sampler
        if self.e.layout.num_ranks != 1:
            raise ValueError("the fused advance needs one rank; several ranks sample, add and apply")
        if not s.hip:
            return self.advance_sequenced(q)
        from . import native
        q = self.e.state if q is None else q
        if q.shape[0] < 4:
            raise ValueError("the velocity needs the shallow-water state (h, M)")
        d = s._desc(q[:4], True, self.K)
        d.x, d.xs, d.v0 = native.ptr(self.st.x), native.ptr(self.st.xs), native.ptr(self.st.v0)
        d.C, d.velocity, d.mode = 3, 1, 2
        d.radius, d.dtp = self.radius, self.dtp
        s._run(d, "points fused advance kernel")

    def lonlat(self):
        """(lat, lon) [K] numpy, radians."""
        return mp.points_lonlat(self.st.x.detach().cpu().numpy())
