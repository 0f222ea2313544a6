"""Derived shallow-water fields of an engine's state: relative vorticity,
divergence, potential vorticity and the invariants (models/derived.py).

``DerivedFields(engine)`` owns the tables (chords, 1/dx + 1/dy), the output and
block-record buffers and the kernel descriptor.  With ``backend='hip'`` on a
GPU ``compute()`` is two ordinary launches of ``ops/csrc/derived_kernel.hip`` on
the caller's stream; with ``backend='torch'``, or on a CPU device, it runs the
PyTorch twin.  The ghost ring is gathered through the ghost map, the carried
corner ghosts and the receive buffer: on a rank with remote ghosts, exchange
first (``start()`` / ``finish()``; ``Engine.derived`` does).

All shape contracts the kernel relies on are checked here, on the host, once,
before anything is launched.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from ..models import derived as md
from .common import use_hip

BLOCK = 16


class DerivedFields:
    def __init__(self, engine):
        e = self.e = engine
        phys = e.physics
        if phys.name != "swe":
            raise ValueError(f"derived fields are defined for the shallow-water model, not {phys.name!r}")
        plan = e.plan
        self.T, self.n, self.ng = plan.T, plan.n, plan.ng
        self.g = float(phys.g)
        self.omega2 = 2.0 * float(phys.omega)
        self.tabs = md.derived_tables(e.geo, e.dtype, e.device)
        self.order = md.face_order(e.geo, e.device)
        self.hip = use_hip(e)
        self._dist = None
        # remote ghosts: the buffer the exchange of transport() fills.  A state with
        # more than the four SWE fields (tracers) exchanges all of them; the kernel
        # and the twin read rows of four, so finish() copies the SWE columns over
        self.F = int(phys.F)
        self.layer = 0          # layered shallow water: the layer whose rows 4 k .. 4 k + 3 are read
        self._recv_all = self.transport().recv
        self.recv = self._recv_all if self.F == 4 else self._recv_all.new_zeros((plan.num_recv, 4))
        if self.hip:
            self._setup_kernel()

    # ---- kernel -----------------------------------------------------------------
    def _setup_kernel(self) -> None:
        from . import native
        e, plan = self.e, self.e.plan
        self.lib = native.require_native()
        T, n, mg, S = self.T, self.n, self.ng, plan.S
        t, tabs = e.tens, self.tabs
        nb = -(-n // BLOCK)
        self.nblocks = T * nb * nb
        self.dcode = native.dtype_code(e.dtype)
        # ---- host-side shape contract checks --------------------------------
        assert e.physics.F >= 4      # (h, M) first; tracer fields behind them are not read
        for b in e.pool:
            assert b.shape == (self.F, S) and b.is_contiguous() and b.dtype == e.dtype
        assert S == T * (n + 2 * mg) ** 2 and mg >= 1
        gm, cgm = plan.ghost_map, plan.corner_map
        assert e.gmap.dtype == torch.int32 and e.gmap.shape == (T, 4, mg, n)
        assert cgm.shape == (T, 4, mg, mg) and cgm.dtype == np.int32
        recv = self.recv
        assert recv.shape == (plan.num_recv, 4) and recv.is_contiguous() and recv.dtype == e.dtype
        for m in (gm, cgm):
            if m.size:
                assert m.max() < S and (-1 - m[m < 0]).max(initial=-1) < plan.num_recv
        shapes = {"invA": (T, n, n), "area": (T, n, n), "b": (T, n, n), "ex": (T, n, n + 1), "ey": (T, n + 1, n),
                  "mx": (T, 3, n + 1), "my": (T, 3, n + 1), "ctr": (3, T, n, n), "pe_t": (T, 4, 3, n)}
        for k, s in shapes.items():
            assert t[k].shape == s and t[k].dtype == e.dtype, k
        for k, s in {"cdx": (T, 3, n, n + 1), "cdy": (T, 3, n + 1, n), "idxy": (T, n, n)}.items():
            assert tabs[k].shape == s and tabs[k].dtype == e.dtype and tabs[k].is_contiguous(), k
        assert t["pedge"].dtype == torch.int32 and t["pedge"].shape == (T,)
        assert t["pe_base"].dtype == torch.int32 and t["pe_base"].shape == (T, 4, 3, n)
        # the kernel reads the layer-0 pair (b, b + 1) at along-strip positions -1 .. n;
        # an end position must be a carried corner ghost wherever a panel-edge side uses it
        pb = e.geo.pe_base[:, :, 0]                                   # [T,4,n]
        assert pb.min(initial=0) >= -1 and pb.max(initial=0) + 1 <= n
        for ti in range(T):
            for side in range(4):
                if not (e.geo.pedge[ti] >> side) & 1:
                    continue
                for hi, used in ((0, (pb[ti, side] == -1).any()), (1, (pb[ti, side] + 1 == n).any())):
                    if used:
                        quad = ((side & 1) | (hi << 1)) if side < 2 else (hi | ((side & 1) << 1))
                        assert plan.corner_carried[ti, quad, 0, 0], "interpolation pair reaches a corner not carried"
        self.cgmap = torch.as_tensor(cgm, dtype=torch.int32, device=e.device)
        self.fields = torch.empty((3, T, n, n), dtype=e.dtype, device=e.device)
        self.partials = torch.zeros((self.nblocks, md.NINV), dtype=torch.float64, device=e.device)
        self.inv = torch.zeros(md.NINV, dtype=torch.float64, device=e.device)
        self.rz = t["ctr"][2].contiguous()
        self._keep = {k: t[k].contiguous() for k in ("invA", "area", "b", "ex", "ey", "mx", "my", "pe_t", "pedge",
                                                     "pe_base")}
        p, k = native.ptr, self._keep
        d = self.desc = native.DerivedDesc()
        d.recv = p(recv) if recv.numel() else 0
        d.gmap, d.cgmap = p(e.gmap), p(self.cgmap)
        d.pedge, d.pe_base, d.pe_t = p(k["pedge"]), p(k["pe_base"]), p(k["pe_t"])
        d.cdx, d.cdy, d.idxy = p(tabs["cdx"]), p(tabs["cdy"]), p(tabs["idxy"])
        d.mx, d.my, d.ex, d.ey = p(k["mx"]), p(k["my"]), p(k["ex"]), p(k["ey"])
        d.invA, d.area, d.b, d.rz = p(k["invA"]), p(k["area"]), p(k["b"]), p(self.rz)
        d.fields, d.partials, d.inv = p(self.fields), p(self.partials), p(self.inv)
        d.ntile, d.n, d.S, d.mg, d.pw = T, n, S, mg, plan.P
        d.nrecv = plan.num_recv
        d.nblocks = self.nblocks
        d.g, d.omega2 = self.g, self.omega2

    def set_layer(self, k: int) -> None:
        """Read layer ``k`` of a layered shallow-water state (rows 4 k .. 4 k + 3
        of the state, a contiguous slice, and the same columns of the receive
        buffer, copied over by ``finish``).  Set before ``start()``."""
        nl = int(getattr(self.e.physics, "nl", 1))
        if not 0 <= int(k) < nl:
            raise ValueError(f"derived fields of layer {k}: this run carries {nl} layer(s)")
        self.layer = int(k)

    # ---- exchange -------------------------------------------------------------------
    def transport(self):
        """The transport that delivers this rank's remote ghosts outside the
        step loop: the engine's own, or, where the native runtime owns the halo
        traffic (``NativeBuffers``), a ``TorchDistTransport`` of the rank's plan
        created on first use (the process group exists in every spmd mode)."""
        from ..parallel.comm import NativeBuffers, TorchDistTransport
        tr = self.e.transport
        if not isinstance(tr, NativeBuffers):
            return tr
        if self._dist is None:
            self._dist = TorchDistTransport(self.e.plan, self.e.physics.F, self.e.dtype, self.e.device)
        return self._dist

    def start(self, q: Optional[torch.Tensor] = None) -> None:
        if self.e.plan.num_recv:
            self.transport().start(self.e.state if q is None else q)

    def finish(self) -> None:
        if self.e.plan.num_recv:
            self.transport().finish()
            if self.F != 4:
                self.recv.copy_(self._recv_all[:, 4 * self.layer:4 * self.layer + 4])

    # ---- compute --------------------------------------------------------------------
    def compute(self, q: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(fields [3, T, n, n], inv [8] float64) of the padded state ``q``
        (default: the engine's state) as device tensors.  The HIP path returns
        its own buffers, overwritten by the next call."""
        e = self.e
        q = (e.state if q is None else q)[4 * self.layer:4 * self.layer + 4]   # (h, M): a contiguous view of four rows
        if not self.hip:
            recv = self.recv if e.plan.num_recv else None
            return e.physics.derived(q, recv, e.gmap, e.cmap, e.tens, self.tabs, self.order, self.T, self.n,
                                     self.ng, e.dt)
        from . import native
        assert q.shape == (4, e.plan.S) and q.is_contiguous() and q.dtype == e.dtype and q.is_cuda
        d = self.desc
        d.Q = native.ptr(q)
        d.dt = float(e.dt)
        native.check(self.lib.stsp_derived_launch(self.dcode, d, native.current_stream_handle(e.device)),
                     "derived kernel")
        return self.fields, self.inv
