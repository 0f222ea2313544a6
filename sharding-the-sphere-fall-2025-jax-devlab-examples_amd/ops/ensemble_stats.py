"""Ensemble mean and variance of one field of a batched state on the device
(models/ensemble_stats.py: the definitions and the PyTorch twin).

``EnsembleStats(engine, members)`` owns the output fields [T, n, n] (float64),
the block records and the descriptor of ``ops/csrc/ensemble_kernel.hip``;
``compute(batch, field)`` takes the batched padded state [M, F, S] and is two
ordinary launches on the caller's stream.  The engine supplies the shapes and
the cell areas; it is member 0 of the ensemble.

All shape contracts the kernel relies on are checked here, on the host, before
anything is launched.
"""
from __future__ import annotations

import ctypes
from typing import Dict

import torch

from ..models import ensemble_stats as me

BLOCK = 16


class EnsStatsDesc(ctypes.Structure):
    """Mirror of EnsStatsDesc (stsp_kernels.h)."""
    _fields_ = [
        ("Q", ctypes.c_void_p), ("area", ctypes.c_void_p), ("mean", ctypes.c_void_p), ("var", ctypes.c_void_p),
        ("partials", ctypes.c_void_p), ("out", ctypes.c_void_p),
        ("member_stride", ctypes.c_longlong),
        ("members", ctypes.c_int), ("fields", ctypes.c_int), ("field", ctypes.c_int),
        ("ntile", ctypes.c_int), ("n", ctypes.c_int), ("S", ctypes.c_int), ("mg", ctypes.c_int), ("pw", ctypes.c_int),
        ("nblocks", ctypes.c_int),
    ]


def _library():
    """The native library with the statistics entry points declared and the
    descriptor's size compared with the mirror's."""
    from . import native
    lib = native.require_native()
    if not getattr(lib, "_ens_stats_declared", False):
        lib.stsp_ensemble_stats_desc_size.argtypes, lib.stsp_ensemble_stats_desc_size.restype = [], ctypes.c_int
        if lib.stsp_ensemble_stats_desc_size() != ctypes.sizeof(EnsStatsDesc):
            raise RuntimeError(f"EnsStatsDesc: ctypes mirror is {ctypes.sizeof(EnsStatsDesc)} bytes, the library's "
                               f"{lib.stsp_ensemble_stats_desc_size()} (stale libstsp.so?)")
        lib.stsp_ensemble_stats_launch.argtypes = [ctypes.c_int, ctypes.POINTER(EnsStatsDesc), ctypes.c_void_p]
        lib.stsp_ensemble_stats_launch.restype = ctypes.c_int
        lib._ens_stats_declared = True
    return lib


class EnsembleStats:
    def __init__(self, engine, members: int):
        from . import native
        e = self.e = engine
        plan = e.plan
        if e.device.type != "cuda":
            raise RuntimeError("the ensemble statistics kernel needs a GPU tensor device")
        self.lib = _library()
        self.M = int(members)
        self.F = int(e.physics.F)
        T, n, mg, S = plan.T, plan.n, plan.ng, plan.S
        nb = -(-n // BLOCK)
        self.nblocks = T * nb * nb
        self.dcode = native.dtype_code(e.dtype)
        # ---- host-side shape contract checks --------------------------------
        assert self.M >= 1
        assert S == T * (n + 2 * mg) ** 2 and plan.P == n + 2 * mg
        assert self.M * self.F * S < (1 << 40) and self.nblocks < (1 << 31) - 1
        self.area = e.tens["area"].contiguous()
        assert self.area.shape == (T, n, n) and self.area.dtype == e.dtype and self.area.is_cuda
        f64 = dict(dtype=torch.float64, device=e.device)
        self.mean = torch.empty((T, n, n), **f64)
        self.var = torch.empty((T, n, n), **f64)
        self.partials = torch.zeros((self.nblocks, 4), **f64)
        self.out = torch.zeros(4, **f64)
        p = native.ptr
        d = self.desc = EnsStatsDesc()
        d.area, d.mean, d.var, d.partials, d.out = p(self.area), p(self.mean), p(self.var), p(self.partials), p(self.out)
        d.member_stride = self.F * S
        d.members, d.fields = self.M, self.F
        d.ntile, d.n, d.S, d.mg, d.pw = T, n, S, mg, plan.P
        d.nblocks = self.nblocks

    def compute(self, batch: torch.Tensor, field: int = 0) -> Dict[str, object]:
        """Statistics of field ``field`` of ``batch`` [M, F, S].  The fields
        returned are this object's buffers, overwritten by the next call."""
        from . import native
        e = self.e
        assert batch.shape == (self.M, self.F, e.plan.S) and batch.is_contiguous()
        assert batch.dtype == e.dtype and batch.is_cuda and batch.device == self.mean.device
        if not 0 <= int(field) < self.F:
            raise ValueError(f"field {field} of a state with {self.F} fields")
        d = self.desc
        d.Q = native.ptr(batch)
        d.field = int(field)
        native.check(self.lib.stsp_ensemble_stats_launch(self.dcode, d, native.current_stream_handle(e.device)),
                     "ensemble statistics kernel")
        return me.summary(self.mean, self.var, self.out.tolist())
