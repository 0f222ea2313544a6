"""Lat-lon input of an engine's state (models/latlon_in.py: the definitions and
the numpy twin).

``LatLonIn(engine, lat, lon)`` owns the checked source grid, the rank's tile
origins and the float64 work copy, and fills the descriptor of
``ops/csrc/latlon_in_kernel.hip``.  ``ingest(arrays, order, quadrature, state)``
overwrites the named fields of the padded ``state`` [F, S] (default: the
engine's) in place: with ``backend='hip'`` on a GPU the preparation and the ingest
launch on the caller's stream; with ``backend='torch'``, or on a CPU device, the
twin runs on the host and its values are copied into the interior.  Either way the
same-rank ghost slots are then refreshed as ``Engine.set_state`` does.

All shape, range and alignment contracts the kernel relies on are checked here,
on the host, before anything is launched.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from ..models import latlon_in as ml
from .common import use_hip

MAX_NODES = 1 << 28               # nlat nlon of the source (the launcher's limit)


class LatLonIn:
    def __init__(self, engine, lat, lon):
        e = self.e = engine
        self.grid = ml.source_grid(lat, lon)
        g, plan = self.grid, e.plan
        if g.nlat * g.nlon > MAX_NODES:
            raise ValueError(f"lat-lon input: a source of {g.nlat} x {g.nlon} nodes exceeds the launch limit {MAX_NODES}")
        self.hip = use_hip(e)
        self._work: Dict[int, torch.Tensor] = {}
        if not self.hip:
            return
        from . import native
        self.lib = native.require_native()
        self.dcode = native.dtype_code(e.dtype)
        lay = e.layout
        org = np.array([lay.tile_origin(t) for t in plan.tiles], dtype=np.int32).reshape(-1, 3)
        # ---- host-side shape contract checks ----------------------------------
        assert plan.S == plan.T * plan.P * plan.P and plan.P == plan.n + 2 * plan.ng and len(org) == plan.T
        assert org[:, 0].min() >= 0 and org[:, 0].max() < 6 and org[:, 1:].min() >= 0
        assert (org[:, 1:] + plan.n).max() <= lay.N
        self.tiles = torch.as_tensor(org, device=e.device).contiguous()
        d = self.desc = native.LatLonInDesc()
        d.tiles, d.S, d.F = native.ptr(self.tiles), plan.S, int(e.physics.F)
        d.lat0, d.dlat, d.lon0, d.dlon = g.lat0, g.dlat, g.lon0, g.dlon
        d.nlat, d.nlon, d.poles = g.nlat, g.nlon, int(g.poles)
        d.ntile, d.n, d.N, d.mg, d.pw = plan.T, plan.n, lay.N, plan.ng, plan.P

    def _source(self, plan: ml.ChannelPlan, arrays) -> torch.Tensor:
        """The input channels [Cin, nlat, nlon] on the device: float32 when every
        array is, else float64."""
        g, dev = self.grid, self.e.device
        ts = [a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)) for a in (arrays[k] for k in plan.inputs)]
        for k, t in zip(plan.inputs, ts):
            if tuple(t.shape) != (g.nlat, g.nlon):
                raise ValueError(f"lat-lon input: {k} has shape {tuple(t.shape)}, the grid is {(g.nlat, g.nlon)}")
        dt = torch.float32 if all(t.dtype == torch.float32 for t in ts) else torch.float64
        return torch.stack([t.to(device=dev, dtype=dt) for t in ts]).contiguous()

    def ingest(self, arrays, order: int = 3, quadrature: int = 1, state: Optional[torch.Tensor] = None,
               phases: int = 3) -> None:
        """``phases``: bit 0 the preparation, bit 1 the ingest launch (a probe times
        them apart; the work copy of the last preparation is kept)."""
        e, g = self.e, self.grid
        plan = ml.channel_plan(e.physics, list(arrays))
        if order not in ml.ORDERS or quadrature not in ml.QUADRATURES:
            raise ValueError(f"lat-lon input: order in {ml.ORDERS} and quadrature in {ml.QUADRATURES} expected, not "
                             f"{order!r}, {quadrature!r}")
        q = e.state if state is None else state
        assert q.shape == (e.physics.F, e.plan.S) and q.dtype == e.dtype and q.device.type == e.device.type
        if not self.hip:
            host = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))
                    for k, v in arrays.items()}
            qi = e.interior(q)
            h_now = None if plan.has_h else qi[0].detach().cpu().double().numpy()
            out = ml.ingest_tiles(g, plan, ml.prepare(g, plan, host), e.layout, e.rank, order, quadrature, h_now)
            for f, v in out.items():
                qi[f].copy_(torch.as_tensor(v).to(e.dtype))
            e.refresh_halos(q)
            return
        from . import native
        src = self._source(plan, arrays)
        C = plan.C
        assert 1 <= C <= ml.MAX_CHANNELS and q.is_contiguous() and src.shape[0] == C - int(plan.has_wind)
        if C not in self._work:
            self._work[C] = torch.empty((C, g.nlat, g.nlon), dtype=torch.float64, device=e.device)
        work = self._work[C]
        assert src.data_ptr() % 8 == 0 and work.data_ptr() % 8 == 0 and q.data_ptr() % 8 == 0
        d = self.desc
        d.src, d.work, d.Q = native.ptr(src), native.ptr(work), native.ptr(q)
        d.src_dtype = native.dtype_code(src.dtype)
        d.C, d.has_h, d.has_wind, d.nq = C, int(plan.has_h), int(plan.has_wind), len(plan.qfields)
        for k in range(4):
            d.qfield[k] = plan.qfields[k] if k < len(plan.qfields) else 0
        d.order, d.quad, d.phases = int(order), int(quadrature), int(phases)
        native.check(self.lib.stsp_latlon_in_launch(self.dcode, d, native.current_stream_handle(e.device)),
                     "lat-lon input kernel")
        e.refresh_halos(q)
