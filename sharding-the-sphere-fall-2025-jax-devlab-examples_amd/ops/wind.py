"""Time-dependent winds of the advection model on the device
(models/advection.py: the flows, the transports and the PyTorch twin).

``WindCompute(engine)`` (an engine with ``backend='hip'`` on a GPU and an
``Advection`` whose flow depends on time) owns

* the factor tables of ``ops/csrc/wind_kernel.hip``, built once on the host in
  float64: for the streamfunction flows the vertex table [4, T, n+1, n+1] from
  slices of the global vertex array (a vertex shared by tiles or ranks of a panel
  carries the same bits on each), for the divergent flow the edge tables
  [5, T, n, n+1] and [5, T, n+1, n] from the edge midpoints, normals and lengths;
* the step count on the device, one int32.  ``set`` writes it from the host,
  ``tick`` adds one by a launch, ``update(c_s, dt)`` launches the kernel that
  refills the engine's ``ex`` / ``ey`` in place at t_s = (count + c_s) dt.

All launches go to the caller's stream, so a captured step replays with its
ticks: k captured steps evaluate k different winds on every replay.  ``set``
must not be captured (its value would be replayed); ``Engine`` calls it from
outside a step only.

All shape contracts the kernel relies on are checked here, on the host, once,
before anything is launched.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from ..models import initial_conditions as ic
from ..models.geometry import lonlat_vectors, xyz_to_lonlat
from .common import use_hip

BLOCK = 16
MAX_EDGES = 1 << 30       # x-edges of a rank: the kernel's edge index and block count stay in int


class WindDesc(ctypes.Structure):
    """Mirror of WindDesc (stsp_kernels.h)."""
    _fields_ = [
        ("ex", ctypes.c_void_p), ("ey", ctypes.c_void_p), ("vtab", ctypes.c_void_p), ("xtab", ctypes.c_void_p),
        ("ytab", ctypes.c_void_p), ("count", ctypes.c_void_p),
        ("ntile", ctypes.c_int), ("n", ctypes.c_int), ("nblocks", ctypes.c_int), ("mode", ctypes.c_int),
        ("dt", ctypes.c_double), ("cs", ctypes.c_double), ("omega", ctypes.c_double), ("pi_over_T", ctypes.c_double),
    ]


def _library():
    """The native library with the wind entry points declared and the
    descriptor's size compared with the mirror's."""
    from . import native
    lib = native.require_native()
    if not getattr(lib, "_wind_declared", False):
        lib.stsp_wind_desc_size.argtypes, lib.stsp_wind_desc_size.restype = [], ctypes.c_int
        if lib.stsp_wind_desc_size() != ctypes.sizeof(WindDesc):
            raise RuntimeError(f"WindDesc: ctypes mirror is {ctypes.sizeof(WindDesc)} bytes, the library's "
                               f"{lib.stsp_wind_desc_size()} (stale libstsp.so?)")
        lib.stsp_wind_launch.argtypes = [ctypes.c_int, ctypes.POINTER(WindDesc), ctypes.c_void_p]
        lib.stsp_wind_launch.restype = ctypes.c_int
        lib.stsp_wind_tick.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.stsp_wind_tick.restype = ctypes.c_int
        lib._wind_declared = True
    return lib


def vertex_table(phys, geo) -> np.ndarray:
    """[4, T, n+1, n+1] float64: sin lam, cos lam, P = R k cos^2 th, Q = -R u_rot sin th
    at the rank's tile vertices, so that psi = P sin^2(lam') c(t) + Q."""
    lon, lat = phys.vertex_lonlat(geo)
    R = geo.grid.radius
    k = ic.deform_amplitude(phys.flow, R, phys.period)
    urot = ic.deform_rotation(phys.flow, R, phys.period)
    return np.stack([np.sin(lon), np.cos(lon), R * k * np.cos(lat) ** 2, -R * urot * np.sin(lat)])


def edge_table(phys, geo, mid: np.ndarray, normal: np.ndarray, length: np.ndarray) -> np.ndarray:
    """[5, *edges] float64 of the divergent flow: sin lam, cos lam of the edge
    midpoints ``mid`` [..., 3] and the factors A, B, C of
    U = c(t) [A (1 - cos lam') + B sin lam'] + C  (``normal`` broadcast to mid)."""
    lon, lat = xyz_to_lonlat(mid)
    e, nn = lonlat_vectors(mid)
    em = np.sum(e * normal, axis=-1) * length
    nm = np.sum(nn * normal, axis=-1) * length
    R = geo.grid.radius
    k = ic.deform_amplitude(phys.flow, R, phys.period)
    urot = ic.deform_rotation(phys.flow, R, phys.period)
    return np.stack([np.sin(lon), np.cos(lon), -0.5 * k * np.sin(2.0 * lat) * np.cos(lat) ** 2 * em,
                     0.5 * k * np.cos(lat) ** 3 * nm, urot * np.cos(lat) * em])


class WindCompute:
    def __init__(self, engine):
        from . import native
        e = self.e = engine
        phys = e.physics
        if not use_hip(e):
            raise RuntimeError("the wind kernel needs backend='hip' on a GPU device")
        if getattr(phys, "flow", None) not in ic.DEFORM_FLOWS:
            raise ValueError(f"the wind kernel knows the flows {list(ic.DEFORM_FLOWS)}, not "
                             f"{getattr(phys, 'flow', None)!r} of {phys.name}")
        self.lib = _library()
        plan, geo = e.plan, e.geo
        T, n = plan.T, plan.n
        self.dcode = native.dtype_code(e.dtype)
        f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=e.device)
        self.count = torch.zeros(1, dtype=torch.int32, device=e.device)
        self.stream_form = phys.flow in ic.STREAM_FLOWS
        d = self.desc = WindDesc()
        if self.stream_form:
            self.vtab = f64(vertex_table(phys, geo))
            nb = -(-n // BLOCK)
            d.mode, d.nblocks = 0, T * nb * nb
            d.vtab = native.ptr(self.vtab)
        else:
            self.xtab = f64(edge_table(phys, geo, geo.xmid, geo.mx[:, None, :, :], geo.lx))
            self.ytab = f64(edge_table(phys, geo, geo.ymid, geo.my[:, :, None, :], geo.ly))
            d.mode, d.nblocks = 1, -(-2 * T * n * (n + 1) // 256)
            d.xtab, d.ytab = native.ptr(self.xtab), native.ptr(self.ytab)
        # ---- host-side shape contract checks --------------------------------
        t = e.tens
        for key, shape in (("ex", (T, n, n + 1)), ("ey", (T, n + 1, n))):
            assert t[key].shape == shape and t[key].is_contiguous() and t[key].dtype == e.dtype and t[key].is_cuda, key
        assert 0 < T * n * (n + 1) < MAX_EDGES and 0 < d.nblocks < (1 << 31) - 1
        if self.stream_form:
            assert self.vtab.shape == (4, T, n + 1, n + 1) and self.vtab.is_contiguous() and self.vtab.is_cuda
        else:
            assert self.xtab.shape == (5, T, n, n + 1) and self.xtab.is_contiguous() and self.xtab.is_cuda
            assert self.ytab.shape == (5, T, n + 1, n) and self.ytab.is_contiguous() and self.ytab.is_cuda
        assert self.count.shape == (1,) and self.count.dtype == torch.int32 and self.count.is_cuda
        # the tables are filled in place: the stage descriptors keep these addresses
        self._ex, self._ey = t["ex"], t["ey"]
        d.ex, d.ey, d.count = native.ptr(self._ex), native.ptr(self._ey), native.ptr(self.count)
        d.ntile, d.n = T, n
        d.omega = 2.0 * math.pi / phys.period if ic.deform_rotation(phys.flow, 1.0, phys.period) else 0.0
        d.pi_over_T = math.pi / phys.period

    def set(self, step_count: int) -> None:
        """Write the device's step count from the host (never inside a capture)."""
        assert 0 <= int(step_count) < (1 << 31) - 1
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the device's step count cannot be set inside a graph capture: the value would replay")
        self.count.fill_(int(step_count))

    def tick(self) -> None:
        from . import native
        native.check(self.lib.stsp_wind_tick(native.ptr(self.count), native.current_stream_handle(self.e.device)),
                     "wind tick")

    def update(self, cs: float, dt: float) -> None:
        """Refill ``ex`` / ``ey`` at t_s = (count + cs) dt."""
        from . import native
        t = self.e.tens
        assert t["ex"] is self._ex and t["ey"] is self._ey, "the transport tables were replaced, not refilled"
        d = self.desc
        d.cs, d.dt = float(cs), float(dt)
        native.check(self.lib.stsp_wind_launch(self.dcode, d, native.current_stream_handle(self.e.device)),
                     "wind kernel")
