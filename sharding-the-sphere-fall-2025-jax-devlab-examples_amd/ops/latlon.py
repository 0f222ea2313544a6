"""Longitude-latitude regridding of an engine's fields (models/latlon.py).

``LatLon(engine, lat, lon)`` owns the rank's index tables (one for the padded
state [F, T P P], one for the unpadded [C, T, n, n] that
``DerivedFields.compute`` returns), the weights and the east / north vectors,
and fills the kernel descriptor of each launch (outputs are fresh tensors, so a
result stays valid across later calls).  With ``backend='hip'`` on a GPU the gather and the
finish step are ordinary launches of ``ops/csrc/latlon_kernel.hip`` on the
caller's stream; with ``backend='torch'``, or on a CPU device, they run the
PyTorch twin.  No ghost slot is ever read.

One rank:   ``fields(q)``, ``tiles(x)``, ``winds(q)`` -> (arrays, zonal means).
Several:    every rank's ``partial_*(terms=True)``: dense, the four terms of
            every sum kept apart ([C, 4, K]), 0 where the rank does not own the
            source; the ranks' arrays added in ascending rank order
            (``ops.common.add_partials``: exact, one rank owns each term), then ``finish`` on
            the sum, which folds the terms in the one-rank association.

All shape contracts the kernel relies on are checked here, on the host, before
anything is launched.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ..models import latlon as ml
from .common import MAX_K, assert_interior, use_hip


class LatLon:
    def __init__(self, engine, lat: np.ndarray, lon: np.ndarray):
        e = self.e = engine
        plan = e.plan
        self.tab = ml.tables_for(e.layout.N, lat, lon)
        self.nlat, self.nlon, self.K = self.tab.nlat, self.tab.nlon, self.tab.K
        pad, unp = self.tab.rank_index(e.layout, e.rank)
        self.pad = ml.regrid_tables(self.tab, pad, e.device)
        self.unp = ml.RegridTables(torch.as_tensor(unp, device=e.device), self.pad.w, self.pad.east, self.pad.north,
                                   self.nlat, self.nlon)
        self.S = plan.S
        self.cells = plan.T * plan.n * plan.n
        self.hip = use_hip(e)
        self._cpu = None          # tables on the CPU, for a finish step on gathered partials (SPMD rank 0)
        # ---- host-side shape contract checks ------------------------------------
        if self.K > MAX_K:
            raise ValueError(f"lat-lon grid of {self.K} points exceeds the launch limit {MAX_K}")
        for tb, lim in ((self.pad, self.S), (self.unp, self.cells)):
            assert tb.idx.dtype == torch.int32 and tb.idx.shape == (self.K, 4) and tb.idx.is_contiguous()
            assert tb.w.dtype == torch.float64 and tb.w.shape == (self.K, 4) and tb.w.is_contiguous()
            if self.K:
                assert int(tb.idx.min()) >= -1 and int(tb.idx.max()) < lim
            for v in (tb.east, tb.north):
                assert v.dtype == torch.float64 and v.shape == (self.K, 3) and v.is_contiguous()
        # the padded table addresses interior cells only (a ghost slot is never a source)
        assert_interior(plan, pad)
        if self.hip:
            from . import native
            self.lib = native.require_native()
            self.dcode = native.dtype_code(e.dtype)
            for tb in (self.pad, self.unp):
                assert tb.idx.data_ptr() % 16 == 0 and tb.w.data_ptr() % 32 == 0

    # ---- kernel ----------------------------------------------------------------------
    def _launch(self, **kw) -> None:
        from . import native
        d = native.LatLonDesc()
        d.K, d.nlat, d.nlon = self.K, self.nlat, self.nlon
        for k, v in kw.items():
            setattr(d, k, native.ptr(v) if isinstance(v, torch.Tensor) else v)
        native.check(self.lib.stsp_latlon_launch(self.dcode, d, native.current_stream_handle(self.e.device)),
                     "lat-lon kernel")

    def _gather(self, x: torch.Tensor, tb: ml.RegridTables, lim: int, velocity: bool, terms: bool) -> torch.Tensor:
        e = self.e
        assert x.dim() == 2 and x.shape[1] == lim and x.is_contiguous() and x.dtype == e.dtype and x.is_cuda
        assert not velocity or x.shape[0] == 4
        C = 3 if velocity else x.shape[0]
        out = torch.empty((C, 4, self.K) if terms else (C, self.K), dtype=e.dtype, device=e.device)
        self._launch(Q=x, idx=tb.idx, w=tb.w, partial=out, cs=lim, C=C, velocity=int(velocity), phases=1,
                     terms=int(terms))
        return out

    # ---- this rank's partials: [C, K], or the terms [C, 4, K] ---------------------------
    def partial_fields(self, q: Optional[torch.Tensor] = None, terms: bool = False) -> torch.Tensor:
        """Every channel of the padded state ``q`` [F, S] (default: the engine's)."""
        q = self.e.state if q is None else q
        if self.hip:
            return self._gather(q, self.pad, self.S, False, terms)
        t = ml.regrid_terms(q, self.pad)
        return t if terms else ml.fold_terms(t)

    def partial_tiles(self, x: torch.Tensor, terms: bool = False) -> torch.Tensor:
        """The channels of an unpadded array ``x`` [C, T, n, n]."""
        x = x.reshape(x.shape[0], -1)
        if self.hip:
            return self._gather(x.contiguous(), self.unp, self.cells, False, terms)
        t = ml.regrid_terms(x, self.unp)
        return t if terms else ml.fold_terms(t)

    def partial_velocity(self, q: Optional[torch.Tensor] = None, terms: bool = False) -> torch.Tensor:
        """The Cartesian velocity [3, K] of the padded shallow-water state."""
        q = self.e.state if q is None else q
        if q.shape[0] < 4:
            raise ValueError("winds need the shallow-water state (h, M)")
        q = q[:4]      # (h, M): a contiguous view (tracer fields follow them)
        if self.hip:
            return self._gather(q, self.pad, self.S, True, terms)
        t = ml.velocity_terms(q[0], q[1:4], self.pad)
        return t if terms else ml.fold_terms(t)

    # ---- finish ---------------------------------------------------------------------------
    def finish(self, partial: torch.Tensor, project: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
        """(arrays [C, nlat, nlon], zonal means [C, nlat] float64) of the summed
        partial [C, K] (or terms [C, 4, K]); ``project``: the Cartesian triple
        becomes (u, v)."""
        C, terms = partial.shape[0], partial.dim() == 3
        assert partial.shape == ((C, 4, self.K) if terms else (C, self.K)) and (not project or C == 3)
        if not (self.hip and partial.is_cuda):
            tb = self.pad
            if partial.device != tb.w.device:
                if self._cpu is None or self._cpu.w.device != partial.device:
                    self._cpu = ml.regrid_tables(self.tab, None, partial.device)
                tb = self._cpu
            partial = ml.fold_terms(partial) if terms else partial
            arr = ml.project(partial, tb) if project else partial.reshape(C, self.nlat, self.nlon)
            return arr, ml.zonal_mean(arr)
        assert partial.is_contiguous() and partial.dtype == self.e.dtype
        Co = 2 if project else C
        zm = torch.empty((Co, self.nlat), dtype=torch.float64, device=partial.device)
        if project or terms:
            out = torch.empty((Co, self.K), dtype=partial.dtype, device=partial.device)
            self._launch(partial=partial, east=self.pad.east, north=self.pad.north, out=out, zm=zm, cs=1, C=C,
                         project=int(project), phases=2, terms=int(terms))
            return out.reshape(Co, self.nlat, self.nlon), zm
        self._launch(partial=partial, zm=zm, cs=1, C=C, phases=2)
        return partial.reshape(C, self.nlat, self.nlon), zm

    # ---- one rank ---------------------------------------------------------------------------
    def fields(self, q: Optional[torch.Tensor] = None):
        return self.finish(self.partial_fields(q))

    def tiles(self, x: torch.Tensor):
        return self.finish(self.partial_tiles(x))

    def winds(self, q: Optional[torch.Tensor] = None):
        return self.finish(self.partial_velocity(q), project=True)
