"""Scale-selective dissipation of an engine's shallow-water state
(models/dissipation.py: the scheme, the host tables and the PyTorch twin).

``Dissipation(engine, order, nu, depth)`` owns the tables, the scratch buffer
[16, S], the inner field of order 2 and the exchanges.  With ``backend='hip'``
on a GPU every application is two ordinary launches of
``ops/csrc/dissipation_kernel.hip`` on the caller's stream (pass 1: cell
gradients into the scratch; pass 2: corrected fluxes and the update); with
``backend='torch'``, or on a CPU device, the twin runs.  A rank with remote
ghosts exchanges the pass-1 input before pass 1 and the scratch rows between
the passes.  Several engines of one process (virtual ranks) move in lockstep:
``apply_all`` / ``laplacian_all`` run every phase on all of them before the
next.  One process per rank (spmd) is not supported.

All shape contracts the kernel relies on are checked here, on the host, once,
before anything is launched.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from ..models import dissipation as md
from .common import assert_interior, use_hip

BLOCK = 16


class DissDesc(ctypes.Structure):
    """Mirror of DissDesc (stsp_kernels.h)."""
    _fields_ = [
        ("src", ctypes.c_void_p), ("recv", ctypes.c_void_p), ("scratch", ctypes.c_void_p),
        ("srecv", ctypes.c_void_p), ("out", ctypes.c_void_p), ("gmap", ctypes.c_void_p),
        ("W", ctypes.c_void_p), ("cx", ctypes.c_void_p), ("cy", ctypes.c_void_p), ("kx", ctypes.c_void_p),
        ("ky", ctypes.c_void_p), ("gb", ctypes.c_void_p), ("dbx", ctypes.c_void_p), ("dby", ctypes.c_void_p),
        ("invA", ctypes.c_void_p), ("ctr", ctypes.c_void_p),
        ("ntile", ctypes.c_int), ("n", ctypes.c_int), ("S", ctypes.c_int), ("mg", ctypes.c_int), ("pw", ctypes.c_int),
        ("nrecv", ctypes.c_int), ("recv_stride", ctypes.c_int), ("nblocks", ctypes.c_int),
        ("pass_", ctypes.c_int), ("mode", ctypes.c_int), ("use_b", ctypes.c_int), ("depth", ctypes.c_int),
        ("coef", ctypes.c_double),
    ]


def _library():
    """The native library with the dissipation entry points declared and the
    descriptor's size compared with the mirror's."""
    from . import native
    lib = native.require_native()
    if not getattr(lib, "_diss_declared", False):
        lib.stsp_dissipation_desc_size.argtypes, lib.stsp_dissipation_desc_size.restype = [], ctypes.c_int
        if lib.stsp_dissipation_desc_size() != ctypes.sizeof(DissDesc):
            raise RuntimeError(f"DissDesc: ctypes mirror is {ctypes.sizeof(DissDesc)} bytes, the library's "
                               f"{lib.stsp_dissipation_desc_size()} (stale libstsp.so?)")
        lib.stsp_dissipation_launch.argtypes = [ctypes.c_int, ctypes.POINTER(DissDesc), ctypes.c_void_p]
        lib.stsp_dissipation_launch.restype = ctypes.c_int
        lib._diss_declared = True
    return lib


def _transport(engine, rows: int, dtype):
    """A transport of the engine's plan for buffers of ``rows`` rows: what the
    engine's own transport is, for another row count."""
    from ..parallel.comm import VirtualTransport
    tr, plan = engine.transport, engine.plan
    if isinstance(tr, VirtualTransport):
        return tr.hub.sub(("dissipation", rows)).transport(plan, rows, dtype, engine.device)
    raise ValueError("dissipation: one process per rank (spmd) is not supported; run one rank or virtual ranks")


class Dissipation:
    def __init__(self, engine, order: int = 1, nu: float = 1.0e5, depth: bool = True):
        e = self.e = engine
        phys = e.physics
        if phys.name != "swe":
            raise ValueError(f"dissipation is defined for the shallow-water model, not {phys.name!r}")
        if order not in (1, 2):
            raise ValueError(f"dissipation: order must be 1 or 2, not {order!r}")
        if not nu > 0:
            raise ValueError(f"dissipation: nu must be positive, not {nu!r}")
        if getattr(phys, "nq", 0) and depth:
            raise ValueError("dissipation with tracers: only depth: false is accepted (diffusing h would change "
                             "the mixing ratios hq / h)")
        self.order, self.nu, self.depth = int(order), float(nu), bool(depth)
        plan = e.plan
        self.T, self.n, self.ng, self.S = plan.T, plan.n, plan.ng, plan.S
        self.F = int(phys.F)
        _, _, b = phys.global_fields(e.grid)
        host = md.dissipation_tables(e.geo, b)
        self.lam_local = self.lam = host["lam"]
        self.use_b = bool(np.any(b != 0))               # the tables of b are zero without a topography
        self.tabs = md.device_tables(host, e.device)
        f64 = dict(dtype=torch.float64, device=e.device)
        self.scratch = torch.zeros((md.ROWS, self.S), **f64)
        self.inner = torch.zeros((4, self.S), **f64)       # order 2: L w; laplacian(): input and output
        self.tr_state = _transport(e, self.F, e.dtype) if plan.num_recv else None
        self.tr_inner = _transport(e, 4, torch.float64) if plan.num_recv else None
        self.tr_scratch = _transport(e, md.ROWS, torch.float64) if plan.num_recv else None
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
        assert self.F >= 4                    # (h, M) first; tracer rows behind them are not touched
        for b in e.pool:
            assert b.shape == (self.F, S) and b.is_contiguous() and b.dtype == e.dtype
        assert S == T * (n + 2 * mg) ** 2 and mg >= 1 and S < (1 << 31) - 1 and self.nblocks < (1 << 31) - 1
        gm = plan.ghost_map
        assert e.gmap.dtype == torch.int32 and e.gmap.shape == (T, 4, mg, n) and e.gmap.is_contiguous()
        if gm.size:
            assert gm.max() < S and (-1 - gm[gm < 0]).max(initial=-1) < plan.num_recv
            # a same-rank source is an interior cell: pass 1 wrote its scratch rows
            assert_interior(plan, gm[:, :, 0, :])
        for buf, rows in ((self.scratch, md.ROWS), (self.inner, 4)):
            assert buf.shape == (rows, S) and buf.is_contiguous() and buf.dtype == torch.float64
        if plan.num_recv:
            for tr, rows, dt in ((self.tr_state, self.F, e.dtype), (self.tr_inner, 4, torch.float64),
                                 (self.tr_scratch, md.ROWS, torch.float64)):
                assert tr.recv.shape == (plan.num_recv, rows) and tr.recv.is_contiguous() and tr.recv.dtype == dt
        shapes = {"W": (4, 3, T, n, n), "kx": (3, T, n, n + 1), "ky": (3, T, n + 1, n), "gb": (3, T, n, n),
                  "ctr": (3, T, n, n), "cx": (T, n, n + 1), "cy": (T, n + 1, n), "dbx": (T, n, n + 1),
                  "dby": (T, n + 1, n), "invA": (T, n, n)}
        for k, s in shapes.items():
            t = self.tabs[k]
            assert t.shape == s and t.dtype == torch.float64 and t.is_contiguous() and t.is_cuda, k
        # the same-rank ghost slots of the four updated rows, refreshed by one indexed copy
        self.hsrc = torch.as_tensor(plan.halo_src, dtype=torch.int32, device=e.device)
        self.hdst = torch.as_tensor(plan.halo_dst, dtype=torch.int32, device=e.device)
        assert plan.halo_src.shape == plan.halo_dst.shape
        if plan.halo_src.size:
            assert 0 <= min(plan.halo_src.min(), plan.halo_dst.min()) and max(plan.halo_src.max(), plan.halo_dst.max()) < S
            assert_interior(plan, plan.halo_src)
            assert not np.intersect1d(plan.halo_src, plan.halo_dst).size
        p, t = native.ptr, self.tabs
        d = self.desc = DissDesc()
        d.scratch = p(self.scratch)
        d.srecv = p(self.tr_scratch.recv) if plan.num_recv else 0
        d.gmap = p(e.gmap)
        d.W, d.cx, d.cy, d.kx, d.ky = p(t["W"]), p(t["cx"]), p(t["cy"]), p(t["kx"]), p(t["ky"])
        d.gb, d.dbx, d.dby, d.invA, d.ctr = p(t["gb"]), p(t["dbx"]), p(t["dby"]), p(t["invA"]), p(t["ctr"])
        d.ntile, d.n, d.S, d.mg, d.pw = T, n, S, mg, plan.P
        d.nrecv = plan.num_recv
        d.nblocks = self.nblocks
        d.depth = int(self.depth)

    def _launch(self, what: str) -> None:
        from . import native
        native.check(self.lib.stsp_dissipation_launch(self.dcode, self.desc,
                                                      native.current_stream_handle(self.e.device)), what)

    # ---- phases (one engine; apply_all / laplacian_all interleave several) -------------------------
    def _src(self, swe: bool):
        return (self.e.state, self.tr_state) if swe else (self.inner, self.tr_inner)

    def start_src(self, swe: bool) -> None:
        q, tr = self._src(swe)
        if tr is not None:
            tr.start(q)

    def pass1(self, swe: bool) -> None:
        """Finish the exchange of the input, then the gradient pass into the scratch."""
        e = self.e
        q, tr = self._src(swe)
        recv = tr.finish() if tr is not None else None
        use_b = self.use_b and swe
        if not self.hip:
            md.gradient_pass(q, recv, e.gmap, self.tabs, self.T, self.n, self.ng, swe, use_b, self.scratch)
            return
        from . import native
        assert q.shape[1] == self.S and q.is_contiguous() and q.is_cuda
        assert q.dtype == (e.dtype if swe else torch.float64) and q.shape[0] == (self.F if swe else 4)
        d = self.desc
        d.src, d.recv = native.ptr(q), (native.ptr(recv) if recv is not None else 0)
        d.recv_stride = q.shape[0]
        d.out = 0
        d.pass_, d.mode, d.use_b, d.coef = 1, int(swe), int(use_b), 0.0
        self._launch("dissipation gradient kernel")

    def start_scratch(self) -> None:
        if self.tr_scratch is not None:
            self.tr_scratch.start(self.scratch)

    def pass2(self, use_b: bool, coef: Optional[float]) -> None:
        """Finish the exchange of the scratch, then the flux pass: ``coef``
        None writes L w to the inner buffer, else the state is updated by
        ``coef`` L w."""
        e = self.e
        srecv = self.tr_scratch.finish() if self.tr_scratch is not None else None
        use_b = self.use_b and use_b
        if not self.hip:
            Lw = md.flux_pass(self.scratch, srecv, e.gmap, self.tabs, self.T, self.n, self.ng, use_b)
            if coef is None:
                e.interior(self.inner).copy_(Lw)
            else:
                md.update(e.interior(e.state), Lw, coef, self.tabs, self.depth)
                e.refresh_halos(e.state)
            return
        from . import native
        d = self.desc
        q = e.state
        assert q.shape == (self.F, self.S) and q.is_contiguous() and q.dtype == e.dtype and q.is_cuda
        d.src, d.recv, d.recv_stride = 0, 0, 0
        d.out = native.ptr(self.inner if coef is None else q)
        d.pass_, d.mode, d.use_b = 2, int(coef is not None), int(use_b)
        d.coef = 0.0 if coef is None else float(coef)
        self._launch("dissipation flux kernel")
        if coef is not None and self.hsrc.numel():
            # the same-rank ghost slots of the updated rows (Engine.refresh_halos in one launch)
            native.copy_index(q, self.hsrc, q, self.hdst, 4, self.S, self.S)

    # ---- one engine -------------------------------------------------------------------------------
    def substeps(self, tau: float) -> int:
        return md.substeps(tau, self.nu, self.lam, self.order)

    def apply(self, tau: float) -> int:
        """One application of ``tau`` seconds to the engine's state (one rank);
        returns the number of sub-steps."""
        return apply_all([self], tau)

    def laplacian(self, x: torch.Tensor) -> torch.Tensor:
        """L x [C, T, n, n] (float64) of the scalars x [C <= 4, T, n, n] (one rank)."""
        return laplacian_all([self], [x])[0]


def _lockstep(ds: Sequence[Dissipation], swe: bool, use_b: bool, coef: Optional[float]) -> None:
    """Both passes of one application on every engine: each phase on all of
    them before the next (the virtual cluster's lockstep)."""
    for d in ds:
        d.start_src(swe)
    for d in ds:
        d.pass1(swe)
    for d in ds:
        d.start_scratch()
    for d in ds:
        d.pass2(use_b, coef)


def apply_all(ds: Sequence[Dissipation], tau: float) -> int:
    """One application of ``tau`` seconds on the engines of ``ds`` (all ranks
    of the layout, in one process), in m equal Euler sub-steps; returns m."""
    lam = max(d.lam_local for d in ds)
    for d in ds:
        d.lam = lam
    m = ds[0].substeps(tau)
    coef = (tau / m) * ds[0].nu
    for _ in range(m):
        if ds[0].order == 1:
            _lockstep(ds, True, True, coef)
        else:
            _lockstep(ds, True, True, None)           # inner = (L eta, L v)
            _lockstep(ds, False, False, -coef)        # w -= coef L inner
    return m


def laplacian_all(ds: Sequence[Dissipation], xs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """L x of every engine's scalars xs[j] [C <= 4, T, n, n]: [C, T, n, n] float64 each."""
    for d, x in zip(ds, xs):
        C = x.shape[0]
        if x.dim() != 4 or not 1 <= C <= 4 or tuple(x.shape[1:]) != (d.T, d.n, d.n):
            raise ValueError(f"laplacian: x [C <= 4, {d.T}, {d.n}, {d.n}] expected, not {tuple(x.shape)}")
        d.inner.zero_()
        d.e.interior(d.inner)[:C] = x.to(device=d.e.device, dtype=torch.float64)
    _lockstep(ds, False, False, None)
    return [d.e.interior(d.inner)[:x.shape[0]].clone() for d, x in zip(ds, xs)]
