"""Snapshot EOFs on the device (models/eof.py: the definitions and the PyTorch
twin).

``Eof(engine, snapshots, k, padded)`` owns the descriptor of
``ops/csrc/eof_kernel.hip``, the cell weights, the output buffers, the slabs'
partials and the error word.  ``compute(x, field)`` takes either contiguous
snapshots [S, T, n, n] in the engine's tile order (``padded=False``) or the
batched padded state [M, F, S_pad] (``padded=True``, the snapshots are the
members of one field) and is four ordinary launches on the caller's stream;
the error word is read back once per call.  The engine supplies the shapes and
the exact cell areas.

All shape contracts the kernel relies on are checked here, on the host, before
anything is launched.
"""
from __future__ import annotations

import ctypes
from typing import Dict

import numpy as np
import torch

from ..models import eof as me

TILE = 64            # cells of a tile of the two tall passes
MAX_SLABS = 1024     # workgroups of a tall pass (four per CU of an MI355X)


class EofDesc(ctypes.Structure):
    """Mirror of EofDesc (stsp_kernels.h)."""
    _fields_ = [
        ("X", ctypes.c_void_p), ("w", ctypes.c_void_p), ("partials", ctypes.c_void_p), ("C", ctypes.c_void_p),
        ("U", ctypes.c_void_p), ("values", ctypes.c_void_p), ("total", ctypes.c_void_p), ("pcs", ctypes.c_void_p),
        ("patterns", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("err", ctypes.c_void_p),
        ("snap_stride", ctypes.c_longlong),
        ("S", ctypes.c_int), ("Spad", ctypes.c_int), ("k", ctypes.c_int), ("Kpad", ctypes.c_int),
        ("padded", ctypes.c_int), ("cells", ctypes.c_int), ("fields", ctypes.c_int), ("field", ctypes.c_int),
        ("ntile", ctypes.c_int), ("n", ctypes.c_int), ("Sp", ctypes.c_int), ("mg", ctypes.c_int), ("pw", ctypes.c_int),
        ("slabs", ctypes.c_int), ("slab_tiles", ctypes.c_int),
    ]


def _library():
    """The native library with the EOF entry points declared and the
    descriptor's size compared with the mirror's."""
    from . import native
    lib = native.require_native()
    if not getattr(lib, "_eof_declared", False):
        lib.stsp_eof_desc_size.argtypes, lib.stsp_eof_desc_size.restype = [], ctypes.c_int
        if lib.stsp_eof_desc_size() != ctypes.sizeof(EofDesc):
            raise RuntimeError(f"EofDesc: ctypes mirror is {ctypes.sizeof(EofDesc)} bytes, the library's "
                               f"{lib.stsp_eof_desc_size()} (stale libstsp.so?)")
        lib.stsp_eof_launch.argtypes = [ctypes.c_int, ctypes.POINTER(EofDesc), ctypes.c_void_p]
        lib.stsp_eof_launch.restype = ctypes.c_int
        lib.stsp_eof_eigen_lds.argtypes, lib.stsp_eof_eigen_lds.restype = [ctypes.c_int], ctypes.c_int
        lib._eof_declared = True
    return lib


class Eof:
    def __init__(self, engine, snapshots: int, k: int, padded: bool):
        from . import native
        e = self.e = engine
        plan = e.plan
        if e.device.type != "cuda":
            raise RuntimeError("the EOF kernel needs a GPU tensor device")
        if e.layout.num_ranks != 1:
            raise ValueError("eof: the kernel runs on one rank")
        self.S = int(snapshots)
        self.k = me.check_args(self.S, k)
        self.padded = bool(padded)
        self.lib = _library()
        self.F = int(e.physics.F)
        T, n, mg, Sp = plan.T, plan.n, plan.ng, plan.S
        self.cells = T * n * n
        self.Spad, self.Kpad = 16 * (-(-self.S // 16)), 16 * (-(-self.k // 16))
        ntiles = -(-self.cells // TILE)
        self.slab_tiles = -(-ntiles // MAX_SLABS)
        self.slabs = -(-ntiles // self.slab_tiles)
        # ---- host-side shape contract checks --------------------------------
        assert Sp == T * (n + 2 * mg) ** 2 and plan.P == n + 2 * mg
        assert self.S * self.F * Sp < (1 << 40) and self.cells < (1 << 31) - TILE
        assert 1 <= self.slabs <= MAX_SLABS and self.slabs * self.slab_tiles >= ntiles > (self.slabs - 1) * self.slab_tiles
        area = np.ascontiguousarray(e.geo.area, dtype=np.float64)
        assert area.shape == (T, n, n) and (area > 0.0).all()
        self.area = torch.as_tensor(area, device=e.device)
        self.w = me.weights(self.area).contiguous()
        f64 = dict(dtype=torch.float64, device=e.device)
        self.partials = torch.empty((self.slabs, self.Spad, self.Spad), **f64)
        self.C = torch.zeros((self.Spad, self.Spad), **f64)
        self.U = torch.zeros((self.Kpad, self.Spad), **f64)
        self.values = torch.zeros(self.k, **f64)
        self.total = torch.zeros(1, **f64)
        self.pcs = torch.zeros((self.k, self.S), **f64)
        self.patterns = torch.empty((self.k, T, n, n), **f64)
        self.mean = torch.empty((T, n, n), **f64)
        self.err = torch.zeros(1, dtype=torch.int32, device=e.device)
        self.eigen_lds = int(self.lib.stsp_eof_eigen_lds(self.S))
        assert self.eigen_lds <= 160 * 1024
        p = native.ptr
        d = self.desc = EofDesc()
        d.w, d.partials, d.C, d.U = p(self.w), p(self.partials), p(self.C), p(self.U)
        d.values, d.total, d.pcs, d.patterns, d.mean, d.err = (p(self.values), p(self.total), p(self.pcs),
                                                               p(self.patterns), p(self.mean), p(self.err))
        d.S, d.Spad, d.k, d.Kpad = self.S, self.Spad, self.k, self.Kpad
        d.padded, d.cells = int(self.padded), self.cells
        d.fields, d.ntile, d.n, d.Sp, d.mg, d.pw = self.F, T, n, Sp, mg, plan.P
        d.snap_stride = self.F * Sp if self.padded else self.cells
        d.slabs, d.slab_tiles = self.slabs, self.slab_tiles

    def compute(self, x: torch.Tensor, field: int = 0) -> Dict[str, torch.Tensor]:
        """The decomposition of ``x`` (contiguous snapshots [S, T, n, n], or the
        batched state [M, F, S_pad] and its ``field``).  The tensors returned are
        this object's buffers, overwritten by the next call.  ``RuntimeError``
        when the Jacobi iteration did not converge."""
        from . import native
        e = self.e
        T, n = e.plan.T, e.plan.n
        if self.padded:
            if tuple(x.shape) != (self.S, self.F, e.plan.S):
                raise ValueError(f"eof: a batched state of shape {(self.S, self.F, e.plan.S)} expected, "
                                 f"not {tuple(x.shape)}")
            if not 0 <= int(field) < self.F:
                raise ValueError(f"eof: field {field} of a state with {self.F} fields")
        elif tuple(x.shape) != (self.S, T, n, n):
            raise ValueError(f"eof: snapshots of shape {(self.S, T, n, n)} expected, not {tuple(x.shape)}")
        assert x.is_contiguous() and x.is_cuda and x.device == self.mean.device
        assert x.data_ptr() % x.element_size() == 0
        d = self.desc
        d.X = native.ptr(x)
        d.field = int(field) if self.padded else 0
        self.err.zero_()
        native.check(self.lib.stsp_eof_launch(native.dtype_code(x.dtype), d, native.current_stream_handle(e.device)),
                     "EOF kernel")
        if int(self.err.item()):
            raise RuntimeError("EOF kernel: the Jacobi eigen-iteration hit its sweep cap; the decomposition is not valid")
        return {"values": self.values, "fraction": self.values / self.total[0], "total": self.total[0],
                "patterns": self.patterns, "pcs": self.pcs, "mean": self.mean}
