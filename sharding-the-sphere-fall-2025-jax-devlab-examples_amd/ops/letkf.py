"""LETKF analysis of a batched ensemble state on the device (models/letkf.py:
the definitions and the PyTorch twin).

``Letkf(engine0, members)`` owns the descriptor of ``ops/csrc/letkf_kernel.hip``,
the cell centres, the same-rank ghost index lists, the work buffers (per number
of observations) and the error word.  ``analyse(batch, Y, p, y, sigma, Lc, rho)``
updates the batched padded state [M, F, S] in place: the preparation and the
analysis launch on the caller's stream, then one indexed copy that makes every
member's same-rank ghost slots current.  The error word is read back once per
call.  The engine supplies the shapes and the geometry; it is member 0.

All shape, alignment and range contracts the kernel relies on are checked here,
on the host, before anything is launched.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import numpy as np
import torch

from ..models import letkf as ml
from .common import assert_interior

BLOCK = 8


class LetkfDesc(ctypes.Structure):
    """Mirror of LetkfDesc (stsp_kernels.h)."""
    _fields_ = [
        ("Q", ctypes.c_void_p), ("Y", ctypes.c_void_p), ("yv", ctypes.c_void_p), ("p", ctypes.c_void_p),
        ("sigma", ctypes.c_void_p), ("centers", ctypes.c_void_p), ("Yp", ctypes.c_void_p), ("d", ctypes.c_void_p),
        ("nobs", ctypes.c_void_p), ("err", ctypes.c_void_p),
        ("member_stride", ctypes.c_longlong),
        ("M", ctypes.c_int), ("Mpad", ctypes.c_int), ("F", ctypes.c_int), ("K", ctypes.c_int),
        ("ntile", ctypes.c_int), ("n", ctypes.c_int), ("S", ctypes.c_int), ("mg", ctypes.c_int), ("pw", ctypes.c_int),
        ("nblocks", ctypes.c_int), ("localised", ctypes.c_int), ("pad_", ctypes.c_int),
        ("radius", ctypes.c_double), ("Lc", ctypes.c_double), ("rho", ctypes.c_double),
    ]


def _library():
    """The native library with the LETKF entry points declared and the
    descriptor's size compared with the mirror's."""
    from . import native
    lib = native.require_native()
    if not getattr(lib, "_letkf_declared", False):
        lib.stsp_letkf_desc_size.argtypes, lib.stsp_letkf_desc_size.restype = [], ctypes.c_int
        if lib.stsp_letkf_desc_size() != ctypes.sizeof(LetkfDesc):
            raise RuntimeError(f"LetkfDesc: ctypes mirror is {ctypes.sizeof(LetkfDesc)} bytes, the library's "
                               f"{lib.stsp_letkf_desc_size()} (stale libstsp.so?)")
        lib.stsp_letkf_launch.argtypes = [ctypes.c_int, ctypes.POINTER(LetkfDesc), ctypes.c_void_p]
        lib.stsp_letkf_launch.restype = ctypes.c_int
        lib._letkf_declared = True
    return lib


class Letkf:
    def __init__(self, engine, members: int):
        from . import native
        e = self.e = engine
        plan = e.plan
        if e.device.type != "cuda":
            raise RuntimeError("the LETKF kernel needs a GPU tensor device")
        if e.layout.num_ranks != 1:
            raise ValueError("the LETKF kernel runs on one rank")
        self.M = int(members)
        if not ml.MIN_M <= self.M <= ml.MAX_M:
            raise ValueError(f"members: the LETKF kernel takes {ml.MIN_M} .. {ml.MAX_M} members, got {self.M}")
        self.lib = _library()
        self.F = int(e.physics.F)
        self.Mpad = 16 if self.M <= 16 else 32
        T, n, mg, S = plan.T, plan.n, plan.ng, plan.S
        nb = -(-n // BLOCK)
        self.nblocks = T * nb * nb
        self.dcode = native.dtype_code(e.dtype)
        # ---- host-side shape contract checks --------------------------------
        assert S == T * (n + 2 * mg) ** 2 and plan.P == n + 2 * mg
        assert self.M * self.F * S < (1 << 40) and self.nblocks < (1 << 31) - 1
        ctr = np.ascontiguousarray(e.geo.center, dtype=np.float64)
        assert ctr.shape == (T, n, n, 3) and np.abs(np.linalg.norm(ctr, axis=-1) - 1.0).max() < 1e-12
        self.centers = torch.as_tensor(ctr, device=e.device)
        assert plan.halo_src.shape == plan.halo_dst.shape
        if plan.halo_src.size:
            assert 0 <= min(plan.halo_src.min(), plan.halo_dst.min()) and max(plan.halo_src.max(), plan.halo_dst.max()) < S
            assert_interior(plan, plan.halo_src)
            assert not np.intersect1d(plan.halo_src, plan.halo_dst).size
        self.hsrc = torch.as_tensor(plan.halo_src, dtype=torch.int32, device=e.device)
        self.hdst = torch.as_tensor(plan.halo_dst, dtype=torch.int32, device=e.device)
        self.nobs = torch.zeros(self.nblocks, dtype=torch.int32, device=e.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=e.device)
        self._work: Dict[int, tuple] = {}
        d = self.desc = LetkfDesc()
        d.centers, d.nobs, d.err = native.ptr(self.centers), native.ptr(self.nobs), native.ptr(self.err)
        d.member_stride = self.F * S
        d.M, d.Mpad, d.F = self.M, self.Mpad, self.F
        d.ntile, d.n, d.S, d.mg, d.pw = T, n, S, mg, plan.P
        d.nblocks = self.nblocks
        d.radius = float(e.grid.radius)

    def _buffers(self, K: int):
        """The work buffers of K observations (Yp [K, Mpad], d [K]), kept for the last few K."""
        if K not in self._work:
            if len(self._work) >= 4:
                self._work.pop(next(iter(self._work)))
            f64 = dict(dtype=torch.float64, device=self.e.device)
            self._work[K] = (torch.zeros((K, self.Mpad), **f64), torch.zeros(K, **f64))
        return self._work[K]

    def analyse(self, batch: torch.Tensor, Y: torch.Tensor, p: torch.Tensor, y: torch.Tensor, sigma: torch.Tensor,
                localisation: Optional[float], inflation: float) -> int:
        """The analysis of ``batch`` [M, F, S] in place from the members' samples
        ``Y`` [M, K] at ``p`` [K, 3] (values ``y``, errors ``sigma`` [K]); the
        most observations any cell saw.  ``RuntimeError`` when a cell's Jacobi
        did not converge (the state is then not to be used)."""
        from . import native
        e = self.e
        dev = self.centers.device
        K = int(Y.shape[1])
        if not 1 <= K <= ml.MAX_K:
            raise ValueError(f"points: {K} observations outside 1 .. {ml.MAX_K}")
        if not float(inflation) >= 1.0:
            raise ValueError(f"inflation: a factor >= 1 expected, not {inflation!r}")
        if localisation is not None and not float(localisation) > 0.0:
            raise ValueError(f"localisation: a positive length expected, not {localisation!r}")
        assert batch.shape == (self.M, self.F, e.plan.S) and batch.is_contiguous()
        assert batch.dtype == e.dtype and batch.is_cuda and batch.device == dev
        for a, shape in ((Y, (self.M, K)), (p, (K, 3)), (y, (K,)), (sigma, (K,))):
            assert a.shape == shape and a.dtype == torch.float64 and a.is_contiguous() and a.device == dev, shape
            assert a.data_ptr() % 8 == 0
        Yp, dd = self._buffers(K)
        d = self.desc
        d.Q, d.Y, d.yv, d.p, d.sigma = (native.ptr(batch), native.ptr(Y), native.ptr(y), native.ptr(p),
                                        native.ptr(sigma))
        d.Yp, d.d = native.ptr(Yp), native.ptr(dd)
        d.K = K
        d.localised = int(localisation is not None)
        d.Lc = float(localisation) if localisation is not None else 0.0
        d.rho = float(inflation)
        self.err.zero_()
        native.check(self.lib.stsp_letkf_launch(self.dcode, d, native.current_stream_handle(e.device)), "LETKF kernel")
        if self.hsrc.numel():
            native.copy_index(batch, self.hsrc, batch, self.hdst, self.M * self.F, e.plan.S, e.plan.S)
        err, nmax = int(self.err.item()), int(self.nobs.max().item())
        if err:
            raise RuntimeError(f"LETKF kernel: a cell's Jacobi eigen-iteration hit its sweep cap (error word {err}); "
                               f"the analysed state is not valid")
        return nmax
