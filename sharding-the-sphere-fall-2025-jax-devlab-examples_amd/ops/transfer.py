"""Grid transfer into a rank's state (models/transfer.py: the definitions and the
PyTorch twin).

``Transfer(physics, layout, rank, grid, dtype, device, hip)`` owns the target side:
the padded cell map of the rank, the target grid's centres and areas, the channel
kinds; the source side's tables (neighbour table, gradient weights, centres,
areas) are built per source resolution on first use.  ``apply(src, q, limiter)``
overwrites the interior of the padded buffer ``q`` [F, S] in place from the global
unpadded state ``src`` [F, 6, Ns, Ns]: with ``hip`` one launch of
``ops/csrc/transfer_kernel.hip`` on the caller's stream, else the twin on the host.
Ghost slots are the caller's to refresh (``Engine.set_from_cubed`` does).

All shape and range contracts the kernel relies on are checked here, on the host,
before anything is launched.
"""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from ..models import transfer as mt
from ..models.base import interior
from ..models.geometry import CubedSphereGrid
from .common import use_hip


class Transfer:
    def __init__(self, physics, layout, rank: int, grid: CubedSphereGrid, dtype, device, hip: bool):
        self.physics, self.layout, self.rank, self.grid = physics, layout, rank, grid
        self.dtype, self.device, self.hip = dtype, torch.device(device), hip
        self.plan = layout.plan(rank)
        self.kind, self.depth = mt.channel_kinds(physics)
        self.F = int(physics.F)
        if self.F > mt.MAX_FIELDS:
            raise ValueError(f"grid transfer: {self.F} rows exceed the limit {mt.MAX_FIELDS}")
        self._twins: Dict[int, mt.RefineTwin] = {}
        self._src: Dict[int, Dict[str, torch.Tensor]] = {}
        if not hip:
            return
        from . import native
        self.lib = native.require_native()
        assert self.lib.stsp_transfer_desc_size() == ctypes.sizeof(native.TransferDesc)
        self.dcode = native.dtype_code(dtype)
        pad = layout.cell_maps(rank)[0]
        plan = self.plan
        # ---- host-side contract checks: every store lands in the interior of the rank's rows
        assert plan.S == plan.T * plan.P * plan.P and pad.shape == (6 * layout.N ** 2,) and pad.max() < plan.S
        from .common import assert_interior
        assert_interior(plan, pad)
        t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.device)
        self.padmap = t(pad, torch.int32)
        self.ctr_t = t(np.moveaxis(grid.centers().reshape(-1, 3), -1, 0))
        self.area_t = t(grid.areas()[0])
        d = self.desc = native.TransferDesc()
        d.padmap, d.ctr_t, d.area_t = native.ptr(self.padmap), native.ptr(self.ctr_t), native.ptr(self.area_t)
        d.S, d.N, d.F = plan.S, layout.N, self.F
        for f in range(self.F):
            d.kind[f], d.depth[f] = self.kind[f], max(self.depth[f], 0)

    @classmethod
    def of_engine(cls, e) -> "Transfer":
        return cls(e.physics, e.layout, e.rank, e.grid, e.dtype, e.device, use_hip(e))

    def _source_tables(self, Ns: int, refine: bool) -> Dict[str, torch.Tensor]:
        """Device tables of the source grid C_Ns (the weights and neighbours for a refinement only)."""
        tabs = self._src.setdefault(Ns, {})
        gs = CubedSphereGrid(Ns, self.grid.radius)
        t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.device)
        if "area" not in tabs:
            tabs["area"] = t(gs.areas()[0])
            tabs["ctr"] = t(np.moveaxis(gs.centers().reshape(-1, 3), -1, 0))
        if refine and "nbr" not in tabs:
            nbr = mt.neighbor_table(Ns)
            assert nbr.shape == (6 * Ns * Ns, 4) and nbr.min() >= 0 and nbr.max() < 6 * Ns * Ns
            tabs["nbr"] = t(nbr, torch.int32)
            tabs["W"] = t(np.transpose(mt.gradient_weights(gs), (1, 2, 0)).reshape(12, -1))
        return tabs

    def twin(self, src: torch.Tensor, limiter: str = "bj") -> torch.Tensor:
        """The global target state [F, 6, N, N] float64 of the twin, on the host."""
        Ns, N = int(src.shape[-1]), self.layout.N
        way, _ = mt.direction(Ns, N)
        src = src.detach().cpu().to(torch.float64)
        if way == "copy":
            return src.clone()
        if way == "coarsen":
            return mt.coarsen(src, self.kind, CubedSphereGrid(Ns, self.grid.radius), self.grid)
        if Ns not in self._twins:
            self._twins[Ns] = mt.RefineTwin(CubedSphereGrid(Ns, self.grid.radius), self.grid)
        return self._twins[Ns](src, self.kind, self.depth, limiter)

    def apply(self, src, q: torch.Tensor, limiter: str = "bj") -> None:
        src = src if isinstance(src, torch.Tensor) else torch.as_tensor(np.asarray(src))
        if src.dim() != 4 or src.shape[0] != self.F or src.shape[1] != 6 or src.shape[2] != src.shape[3]:
            raise ValueError(f"grid transfer: a state [{self.F}, 6, Ns, Ns] expected, not {tuple(src.shape)}")
        if limiter not in mt.LIMITERS:
            raise ValueError(f"grid transfer: limiter in {mt.LIMITERS} expected, not {limiter!r}")
        Ns, N, plan = int(src.shape[-1]), self.layout.N, self.plan
        way, r = mt.direction(Ns, N)
        assert q.shape == (self.F, plan.S) and q.dtype == self.dtype and q.device.type == self.device.type
        qi = interior(q, plan.T, plan.n, plan.ng)
        if not self.hip or way == "copy":
            g = self.twin(src, limiter).numpy()
            n = plan.n
            for li, tid in enumerate(plan.tiles):
                f, I0, J0 = self.layout.tile_origin(tid)
                qi[:, li].copy_(torch.as_tensor(g[:, f, J0:J0 + n, I0:I0 + n]).to(self.dtype))
            return
        from . import native
        s64 = src.to(device=self.device, dtype=torch.float64).contiguous()
        tabs = self._source_tables(Ns, way == "refine")
        assert q.is_contiguous() and s64.data_ptr() % 8 == 0 and q.data_ptr() % 8 == 0 and s64.numel() == self.F * 6 * Ns * Ns
        assert 6 * max(N, Ns) ** 2 < (1 << 31)
        d = self.desc
        d.src, d.Q, d.Ns, d.r = native.ptr(s64), native.ptr(q), Ns, r
        d.coarsen, d.limiter = int(way == "coarsen"), int(limiter == "bj")
        d.ctr_s, d.area_s = native.ptr(tabs["ctr"]), native.ptr(tabs["area"])
        d.nbr, d.W = (native.ptr(tabs["nbr"]), native.ptr(tabs["W"])) if way == "refine" else (None, None)
        native.check(self.lib.stsp_transfer_launch(self.dcode, d, native.current_stream_handle(self.device)),
                     "grid transfer kernel")
