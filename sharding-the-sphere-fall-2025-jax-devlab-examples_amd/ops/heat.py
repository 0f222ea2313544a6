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

``HeatOperator.solve(b, tau)`` solves the Helmholtz problem (I - tau L) x = b, the
building block of the implicit steps (``implicit_step``: backward Euler and
Crank-Nicolson, ``physics.implicit``), by BiCGStab: with ``backend='hip'`` the
device-resident iteration of ``ops/csrc/helmholtz_kernel.hip``, else its twin
``models.diffusion.helmholtz_bicgstab``.

All shape contracts the kernels rely on are checked here, on the host, once,
before anything is launched.
"""
from __future__ import annotations

import ctypes
import math
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


class HelmDesc(ctypes.Structure):
    """Mirror of HelmDesc (stsp_kernels.h)."""
    _fields_ = [
        ("work", ctypes.c_void_p), ("scratch", ctypes.c_void_p), ("gmap", ctypes.c_void_p), ("W", ctypes.c_void_p),
        ("cx", ctypes.c_void_p), ("cy", ctypes.c_void_p), ("kx", ctypes.c_void_p), ("ky", ctypes.c_void_p),
        ("invA", ctypes.c_void_p), ("partials", ctypes.c_void_p), ("block", ctypes.c_void_p),
        ("ntile", ctypes.c_int), ("n", ctypes.c_int), ("S", ctypes.c_int), ("mg", ctypes.c_int), ("pw", ctypes.c_int),
        ("nblocks", ctypes.c_int), ("op", ctypes.c_int), ("iters", ctypes.c_int),
        ("tau", ctypes.c_double), ("tol", ctypes.c_double),
    ]


# stsp_kernels.h: STSP_HELM_ROWS, STSP_HELM_BLOCK, STSP_HELM_RECORD, STSP_HELM_MAX_ITERS
HELM_ROWS, HELM_BLOCK, HELM_RECORD, HELM_MAX_CHUNK = 8, 10, 8, 64
RX, RR, RH, RP, RV, RS, RT, RB = range(HELM_ROWS)


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
        lib.stsp_helmholtz_desc_size.argtypes, lib.stsp_helmholtz_desc_size.restype = [], ctypes.c_int
        if lib.stsp_helmholtz_desc_size() != ctypes.sizeof(HelmDesc):
            raise RuntimeError(f"HelmDesc: ctypes mirror is {ctypes.sizeof(HelmDesc)} bytes, the library's "
                               f"{lib.stsp_helmholtz_desc_size()} (stale libstsp.so?)")
        lib.stsp_helmholtz_launch.argtypes = [ctypes.POINTER(HelmDesc), ctypes.c_void_p]
        lib.stsp_helmholtz_launch.restype = ctypes.c_int
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
        self.work = None              # the solver's rows, blocks and descriptor: built by the first solve
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

    # ---- the Helmholtz solve ------------------------------------------------------------------------
    def _setup_solver(self) -> None:
        """The work rows [8, S] (x, r, rhat, p, v, s, t, b; float64, padded layout), and for
        the kernels the partials, the scalar block, the pinned record and the descriptor,
        with the shape contracts of ``helmholtz_kernel.hip`` checked."""
        e, plan = self.e, self.e.plan
        if plan.num_recv:
            raise ValueError("HeatOperator.solve: a rank with remote ghosts (virtual ranks): the inner products "
                             "of the iteration would need a fold across ranks; run one rank")
        if self.work is not None:
            return
        f64 = dict(dtype=torch.float64, device=e.device)
        self.area = 1.0 / self.tabs["invA"]
        work = torch.zeros((HELM_ROWS, self.S), **f64)
        if self.hip:
            from . import native
            self.partials = torch.zeros((2, self.nblocks), **f64)
            self.block = torch.zeros((HELM_BLOCK,), **f64)
            self.record = torch.zeros((HELM_BLOCK - HELM_RECORD,), dtype=torch.float64, pin_memory=True)
            assert work.shape == (HELM_ROWS, self.S) and work.is_contiguous() and work.is_cuda
            assert self.partials.is_contiguous() and self.block.is_contiguous()
            assert self.record.numel() * 8 == 16
            gm = plan.ghost_map                      # every neighbour across a tile side is a cell of this rank
            assert gm.size == 0 or (gm.min() >= 0 and gm.max() < self.S)
            d, h = HelmDesc(), self.desc
            d.work, d.partials, d.block = native.ptr(work), native.ptr(self.partials), native.ptr(self.block)
            for k in ("scratch", "gmap", "W", "cx", "cy", "kx", "ky", "invA", "ntile", "n", "S", "mg", "pw", "nblocks"):
                setattr(d, k, getattr(h, k))
            self.hdesc = d
        self.work = work

    def _row(self, r: int) -> torch.Tensor:
        """Interior view [T, n, n] of work row ``r``."""
        return self.e.interior(self.work[r:r + 1])[0]

    def _twin_laplacian(self, u: torch.Tensor) -> torch.Tensor:
        """L u [T, n, n] by the twin's two passes (row t of the work rows stages u)."""
        e = self.e
        self._row(RT).copy_(u)
        mh.heat_gradient_pass(self.work[RT:RT + 1], None, e.gmap, self.tabs, self.T, self.n, self.ng, self.scratch)
        return mh.heat_flux_pass(self.scratch, None, e.gmap, self.tabs, self.T, self.n, self.ng)

    def _launch_solver(self, op: int, iters: int, tau: float, tol: float) -> dict:
        """One call of the entry point (op 0: set up, 1: ``iters`` iterations), then the
        16-byte record: the only device-to-host traffic of a chunk."""
        from . import native
        d = self.hdesc
        d.op, d.iters, d.tau, d.tol = op, iters, tau, tol
        native.check(self.lib.stsp_helmholtz_launch(d, native.current_stream_handle(self.e.device)),
                     "helmholtz kernels")
        self.record.copy_(self.block[HELM_RECORD:], non_blocking=True)
        torch.cuda.current_stream(self.e.device).synchronize()
        flags, iters = self.record.numpy().view(np.int32)[2:4]
        return {"iterations": int(iters), "residual": float(self.record[0]), "flag": int(flags)}

    def solve(self, b: torch.Tensor, tau: float, x0: Optional[torch.Tensor] = None, tol: float = 1e-10,
              maxiter: int = 500, chunk: int = 8, out: Optional[torch.Tensor] = None):
        """x with (I - tau L) x = b, by unpreconditioned BiCGStab (L is not symmetric).

        ``b`` and ``x0`` (default: zero) are interior values [T, n, n] of any floating
        type; the iteration is float64 throughout and x is rounded once, to ``b``'s type
        (or copied into ``out``, an interior view, and rounded to its type).  Returns (x,
        record) with record = {iterations, residual: ||r|| / ||b|| in the area-weighted
        norm, flag: ``models.diffusion.HELM_CONVERGED``}.  With the kernels the scalars stay
        on the device: ``chunk`` iterations are launched at a time on the caller's stream,
        and the record is read back after each chunk.

        Raises ``RuntimeError`` (with the record as ``.record``) on a breakdown or when
        ``maxiter`` iterations do not reach ``||r|| <= tol ||b||``; the work row x then holds
        the last iterate.  One rank: a rank with remote ghosts (virtual ranks) raises
        ``ValueError``, because the inner products would need a fold across ranks."""
        shape = (self.T, self.n, self.n)
        tau, tol = float(tau), float(tol)
        if tuple(b.shape) != shape or (x0 is not None and tuple(x0.shape) != shape):
            raise ValueError(f"HeatOperator.solve: b and x0 of shape {shape} expected, not {tuple(b.shape)}")
        if not (math.isfinite(tau) and tol >= 0.0 and maxiter >= 1 and 1 <= chunk <= HELM_MAX_CHUNK):
            raise ValueError(f"HeatOperator.solve: finite tau, tol >= 0, maxiter >= 1 and 1 <= chunk <= "
                             f"{HELM_MAX_CHUNK} expected, not tau={tau}, tol={tol}, maxiter={maxiter}, chunk={chunk}")
        self._setup_solver()
        self._row(RB).copy_(b)
        if x0 is None:
            self._row(RX).zero_()
        else:
            self._row(RX).copy_(x0)
        if self.hip:
            rec = self._launch_solver(0, 0, tau, tol)
            while not rec["flag"] and rec["iterations"] < maxiter:
                rec = self._launch_solver(1, min(chunk, maxiter - rec["iterations"]), tau, tol)
        else:
            x, rec = mh.helmholtz_bicgstab(self._twin_laplacian, self.area, self._row(RB).clone(),
                                           self._row(RX).clone(), tau, tol, maxiter)
            self._row(RX).copy_(x)
        if rec["flag"] != mh.HELM_CONVERGED:
            err = RuntimeError(f"HeatOperator.solve: " + ("breakdown" if rec["flag"] else "no convergence") +
                               f" after {rec['iterations']} iterations, ||r|| / ||b|| = {rec['residual']:.3e} "
                               f"(tol {tol:g}, tau {tau:g})")
            err.record = rec
            raise err
        if out is None:
            out = torch.empty(shape, dtype=b.dtype, device=b.device)
        out.copy_(self._row(RX))
        return out, rec

    def implicit_step(self, dt: float, kappa: float, theta: float, tol: float = 1e-10, maxiter: int = 500) -> dict:
        """One step of the theta scheme on the engine's state,

            (I - theta dt kappa L) T' = T + (1 - theta) dt kappa L T,

        backward Euler (theta = 1) or Crank-Nicolson (1/2): the right-hand side from the two
        passes, the solve from T as the first guess; returns the solve's record."""
        e = self.e
        Ti = e.interior(e.state)[0]
        b = Ti.to(torch.float64)
        if theta != 1.0:
            b = b + ((1.0 - theta) * dt * kappa) * self.laplacian()
        _, rec = self.solve(b, theta * dt * kappa, x0=Ti, tol=tol, maxiter=maxiter, out=Ti)
        self.refresh(e.state)
        e.time += dt
        e._step_count += 1
        return rec


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
