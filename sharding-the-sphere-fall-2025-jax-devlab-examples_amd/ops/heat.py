"""Consistent thermal diffusion of an engine's scalar field (models/diffusion.py:
the scheme and the PyTorch twin; models/dissipation.py: the host tables).

``HeatOperator(engine)`` (an engine with one field) owns the tables, the
scratch buffer [4, S] (T, Gx, Gy, Gz), the Laplacian's output row and, for a
rank with remote ghosts, a second transport of 4 float64 rows for the scratch.  With ``backend='hip'`` on a GPU
both passes are ordinary launches of ``ops/csrc/heat_kernel.hip`` on the
caller's stream; with ``backend='torch'``, or on a CPU device, the twin runs.
``ConsistentCompute(engine)`` is the engine's compute class for a physics that
declares the two-pass operator (``Physics.two_pass``): a stage has four phases,

    stage_begin   start the exchange of Q                      (Engine)
    stage_mid     finish it, pass 1 (gradients), start the exchange of the scratch
    stage_end     finish it, pass 2 (fluxes, L, the stage combination)

and ``Engine.step`` / ``VirtualCluster.step`` run each phase on all engines
before the next.  No stage reads a ghost slot; ``end_step`` refreshes the
same-rank ghost slots of the new state by one indexed copy, so that they equal
their source cells as the output products expect.  One process per rank (spmd)
is not supported.

All shape contracts the kernels rely on are checked here, on the host, once,
before anything is launched.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..models import diffusion as mh
from ..models import dissipation as md
from ..models.integrators import Stage
from .common import assert_interior, use_hip

BLOCK = 16
TABLES = ("W", "cx", "cy", "kx", "ky", "invA")


class HeatDesc(ctypes.Structure):
    """Mirror of HeatDesc (stsp_kernels.h)."""
    _fields_ = [
        ("q", ctypes.c_void_p), ("recv", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("srecv", ctypes.c_void_p),
        ("gmap", ctypes.c_void_p), ("W", ctypes.c_void_p), ("cx", ctypes.c_void_p), ("cy", ctypes.c_void_p),
        ("kx", ctypes.c_void_p), ("ky", ctypes.c_void_p), ("invA", ctypes.c_void_p), ("x", ctypes.c_void_p),
        ("acc_in", ctypes.c_void_p), ("out", ctypes.c_void_p), ("acc_out", ctypes.c_void_p), ("lout", ctypes.c_void_p),
        ("ntile", ctypes.c_int), ("n", ctypes.c_int), ("S", ctypes.c_int), ("mg", ctypes.c_int), ("pw", ctypes.c_int),
        ("nrecv", ctypes.c_int), ("recv_stride", ctypes.c_int), ("nblocks", ctypes.c_int),
        ("pass_", ctypes.c_int), ("mode", ctypes.c_int),
        ("kappa", ctypes.c_double), ("a0", ctypes.c_double), ("a1", ctypes.c_double), ("a2dt", ctypes.c_double),
        ("c0", ctypes.c_double), ("c1", ctypes.c_double), ("c2dt", ctypes.c_double),
    ]


def _library():
    """The native library with the heat entry points declared and the
    descriptor's size compared with the mirror's."""
    from . import native
    lib = native.require_native()
    if not getattr(lib, "_heat_declared", False):
        lib.stsp_heat_desc_size.argtypes, lib.stsp_heat_desc_size.restype = [], ctypes.c_int
        if lib.stsp_heat_desc_size() != ctypes.sizeof(HeatDesc):
            raise RuntimeError(f"HeatDesc: ctypes mirror is {ctypes.sizeof(HeatDesc)} bytes, the library's "
                               f"{lib.stsp_heat_desc_size()} (stale libstsp.so?)")
        lib.stsp_heat_launch.argtypes = [ctypes.c_int, ctypes.POINTER(HeatDesc), ctypes.c_void_p]
        lib.stsp_heat_launch.restype = ctypes.c_int
        lib._heat_declared = True
    return lib


def _transport(engine, rows: int, dtype):
    """A transport of the engine's plan for buffers of ``rows`` rows: what the
    engine's own transport is, for another row count."""
    from ..parallel.comm import VirtualTransport
    tr = engine.transport
    if isinstance(tr, VirtualTransport):
        return tr.hub.sub(("heat", rows)).transport(engine.plan, rows, dtype, engine.device)
    raise ValueError("physics.operator: consistent (the two-pass Laplacian): one process per rank (spmd) is not "
                     "supported; run one rank or virtual ranks")


class HeatOperator:
    """Both passes of the consistent Laplacian of an engine's scalar field."""

    def __init__(self, engine):
        e = self.e = engine
        if e.physics.F != 1:
            raise ValueError(f"the consistent Laplacian of ops/heat.py takes one scalar field, not {e.physics.fields}")
        plan = e.plan
        self.T, self.n, self.ng, self.S = plan.T, plan.n, plan.ng, plan.S
        host = md.dissipation_tables(e.geo)
        self.lam_local = host["lam"]
        dev = md.device_tables(host, e.device)
        self.tabs = {k: dev[k] for k in TABLES}
        f64 = dict(dtype=torch.float64, device=e.device)
        self.scratch = torch.zeros((mh.HEAT_ROWS, self.S), **f64)
        self.lout = torch.zeros((1, self.S), **f64)
        self.tr_scratch = _transport(e, mh.HEAT_ROWS, torch.float64) if plan.num_recv else None
        self.hip = use_hip(e)
        if self.hip:
            self._setup_kernel()

    # ---- kernel -----------------------------------------------------------------
    def _setup_kernel(self) -> None:
        from . import native
        e, plan = self.e, self.e.plan
        self.lib = _library()
        T, n, mg, S = self.T, self.n, self.ng, self.S
        nb = -(-n // BLOCK)
        self.nblocks = T * nb * nb
        self.dcode = native.dtype_code(e.dtype)
        # ---- host-side shape contract checks --------------------------------
        for b in e.pool:
            assert b.shape == (1, S) and b.is_contiguous() and b.dtype == e.dtype and b.is_cuda
        assert S == T * (n + 2 * mg) ** 2 and plan.P == n + 2 * mg and mg >= 1
        assert S < (1 << 31) - 1 and self.nblocks < (1 << 31) - 1
        gm = plan.ghost_map
        assert e.gmap.dtype == torch.int32 and e.gmap.shape == (T, 4, mg, n) and e.gmap.is_contiguous()
        if gm.size:
            assert gm.max() < S and (-1 - gm[gm < 0]).max(initial=-1) < plan.num_recv
            # a same-rank source is an interior cell: pass 1 wrote its scratch rows
            assert_interior(plan, gm[:, :, 0, :])
        for buf, rows in ((self.scratch, mh.HEAT_ROWS), (self.lout, 1)):
            assert buf.shape == (rows, S) and buf.is_contiguous() and buf.dtype == torch.float64
        if plan.num_recv:
            for tr, rows, dt in ((e.transport, 1, e.dtype), (self.tr_scratch, mh.HEAT_ROWS, torch.float64)):
                assert tr.recv.shape == (plan.num_recv, rows) and tr.recv.is_contiguous() and tr.recv.dtype == dt
                assert tr.recv.is_cuda
        shapes = {"W": (4, 3, T, n, n), "kx": (3, T, n, n + 1), "ky": (3, T, n + 1, n), "cx": (T, n, n + 1),
                  "cy": (T, n + 1, n), "invA": (T, n, n)}
        for k, s in shapes.items():
            t = self.tabs[k]
            assert t.shape == s and t.dtype == torch.float64 and t.is_contiguous() and t.is_cuda, k
        # the same-rank ghost slots, refreshed by one indexed copy (refresh)
        self.hsrc = torch.as_tensor(plan.halo_src, dtype=torch.int32, device=e.device)
        self.hdst = torch.as_tensor(plan.halo_dst, dtype=torch.int32, device=e.device)
        assert plan.halo_src.shape == plan.halo_dst.shape
        if plan.halo_src.size:
            assert 0 <= min(plan.halo_src.min(), plan.halo_dst.min()) and max(plan.halo_src.max(), plan.halo_dst.max()) < S
            assert_interior(plan, plan.halo_src)
            assert not np.intersect1d(plan.halo_src, plan.halo_dst).size
        p, t = native.ptr, self.tabs
        d = self.desc = HeatDesc()
        d.scratch, d.lout = p(self.scratch), p(self.lout)
        d.srecv = p(self.tr_scratch.recv) if plan.num_recv else 0
        d.gmap = p(e.gmap)
        d.W, d.cx, d.cy, d.kx, d.ky, d.invA = p(t["W"]), p(t["cx"]), p(t["cy"]), p(t["kx"]), p(t["ky"]), p(t["invA"])
        d.ntile, d.n, d.S, d.mg, d.pw = T, n, S, mg, plan.P
        d.nrecv = plan.num_recv
        d.nblocks = self.nblocks
        d.recv_stride = 1

    def _ptr(self, buf: torch.Tensor) -> int:
        """Device address of a buffer of the pool's shape and type."""
        assert buf.shape == (1, self.S) and buf.is_contiguous() and buf.dtype == self.e.dtype and buf.is_cuda
        return int(buf.data_ptr())

    def _launch(self, what: str) -> None:
        from . import native
        native.check(self.lib.stsp_heat_launch(self.dcode, self.desc, native.current_stream_handle(self.e.device)),
                     what)

    # ---- phases (one engine; the callers interleave several) --------------------------------------
    def pass1(self, q: torch.Tensor, recv: Optional[torch.Tensor]) -> None:
        """The padded buffer ``q`` [1, S] and its gradient into the scratch;
        ``recv``: the finished exchange of ``q`` (None without remote ghosts)."""
        e = self.e
        if not self.hip:
            mh.heat_gradient_pass(q, recv, e.gmap, self.tabs, self.T, self.n, self.ng, self.scratch)
            return
        d = self.desc
        d.q = self._ptr(q)
        if recv is not None and recv.numel():
            assert recv.shape == (e.plan.num_recv, 1) and recv.is_contiguous() and recv.dtype == e.dtype
            assert recv.is_cuda
            d.recv = int(recv.data_ptr())
        else:
            assert e.plan.num_recv == 0
            d.recv = 0
        d.pass_, d.mode = 1, 0
        self._launch("heat gradient kernel")

    def start_scratch(self) -> None:
        if self.tr_scratch is not None:
            self.tr_scratch.start(self.scratch)

    def _finish_scratch(self) -> Optional[torch.Tensor]:
        return self.tr_scratch.finish() if self.tr_scratch is not None else None

    def pass2_laplacian(self) -> torch.Tensor:
        """L [T, n, n] (float64, a view of the output row) from the scratch."""
        e = self.e
        srecv = self._finish_scratch()
        Li = e.interior(self.lout)[0]
        if not self.hip:
            Li.copy_(mh.heat_flux_pass(self.scratch, srecv, e.gmap, self.tabs, self.T, self.n, self.ng))
            return Li
        d = self.desc
        d.pass_, d.mode = 2, 0
        self._launch("heat flux kernel (L)")
        return Li

    def pass2_stage(self, st: Stage, dt: float, kappa: float) -> None:
        """The stage combination with dq = kappa L into ``pool[st.out]`` (and the
        accumulator), rounded once to the state's type."""
        e = self.e
        srecv = self._finish_scratch()
        acc = st.acc_out >= 0
        if not self.hip:
            L = mh.heat_flux_pass(self.scratch, srecv, e.gmap, self.tabs, self.T, self.n, self.ng)
            iv = lambda b: e.interior(e.pool[b])[0]
            out, a = mh.heat_stage(L, st, dt, kappa, iv(st.X), iv(st.Q), iv(st.acc_in) if st.acc_in >= 0 else None)
            if acc:
                iv(st.acc_out).copy_(a)
            iv(st.out).copy_(out)
            return
        d = self.desc
        d.q, d.x, d.out = self._ptr(e.pool[st.Q]), self._ptr(e.pool[st.X]), self._ptr(e.pool[st.out])
        d.acc_in = self._ptr(e.pool[st.acc_in]) if acc and st.acc_in >= 0 else 0
        d.acc_out = self._ptr(e.pool[st.acc_out]) if acc else 0
        d.pass_, d.mode = 2, 2 if acc else 1
        d.kappa, d.a0, d.a1, d.a2dt = float(kappa), st.a0, st.a1, st.a2 * dt
        d.c0, d.c1, d.c2dt = st.c0, st.c1, st.c2 * dt
        self._launch("heat flux kernel (stage)")

    def refresh(self, q: torch.Tensor) -> None:
        """The same-rank ghost slots of ``q`` from their source cells."""
        if not self.hip:
            self.e.refresh_halos(q)
        elif self.hsrc.numel():
            from . import native
            assert self._ptr(q)
            native.copy_index(q, self.hsrc, q, self.hdst, 1, self.S, self.S)

    def laplacian(self) -> torch.Tensor:
        """L [T, n, n] (float64) of the engine's state (one rank)."""
        return laplacian_all([self])[0]


def laplacian_all(ops: Sequence[HeatOperator]) -> List[torch.Tensor]:
    """L of every engine's state ([T, n, n] float64 each), all ranks of the layout
    in one process: each phase on all of them before the next."""
    for o in ops:
        o.e.transport.start(o.e.state)
    for o in ops:
        o.pass1(o.e.state, o.e.transport.finish())
    for o in ops:
        o.start_scratch()
    return [o.pass2_laplacian().clone() for o in ops]


class ConsistentCompute:
    """The engine's stages for a physics with ``two_pass``: ``dq = kappa L Q``."""

    def __init__(self, engine):
        self.e = engine
        self.op = HeatOperator(engine)

    def stage(self, st: Stage, dt: float, recv: Optional[torch.Tensor], part: str = "all") -> None:
        """``interior``: nothing (pass 1 needs every neighbour); ``boundary``: pass 2
        (``recv`` is not used: ``stage_mid`` has consumed the exchange of Q)."""
        if part == "interior":
            return
        if part == "all":
            self.stage_mid(st, dt, recv)
        self.op.pass2_stage(st, dt, self.e.physics.kappa)

    def stage_mid(self, st: Stage, dt: float, recv: Optional[torch.Tensor]) -> None:
        """Pass 1 from the finished exchange of Q, then start the scratch exchange."""
        self.op.pass1(self.e.pool[st.Q], recv)
        self.op.start_scratch()

    def end_step(self) -> None:
        self.op.refresh(self.e.state)
