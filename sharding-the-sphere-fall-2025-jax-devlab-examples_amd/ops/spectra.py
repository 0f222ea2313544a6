"""Spherical-harmonic analysis of an engine's fields, and synthesis of
coefficients on its cells (models/spectra.py).

``Spectra(engine, lmax)`` owns the rank's tables (mu, cos phi, lambda, w per
cell; the recurrence factors), one index table per source layout (the padded
state [F, T P P] and the unpadded [C, T, n, n] that ``DerivedFields.compute``
returns), the workgroup records and the kernel descriptor.  With
``backend='hip'`` on a GPU the analysis is two ordinary launches of
``ops/csrc/spectra_kernel.hip`` on the caller's stream; with
``backend='torch'``, or on a CPU device, it runs the PyTorch twin.  No ghost
slot is ever read.

One rank:   ``partial_fields(q)`` / ``partial_tiles(x)`` are the coefficients
            [C, 2, L+1, L+1] float64 (cos, sin; [l, m]).
Several:    every rank's partial is the sum over its own cells; the ranks'
            arrays are added in ascending rank order (``ops.common.add_partials``).

Synthesis:  ``synthesise(coeffs)`` is the band-limited field [C, T, n, n] float64
            of coefficients [C, 2, L+1, L+1] at this rank's cell centres: one
            launch of ``ops/csrc/synth_kernel.hip`` over (cell batches) x (order
            chunks), and a fold of the chunks where there are several; the twin
            (``models.spectra.synthesise``) otherwise.  Every rank synthesises
            its own cells from the same coefficients.

All shape contracts the kernels rely on are checked here, on the host, before
anything is launched.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from ..models import spectra as ms
from .common import assert_interior, use_hip

BATCH = 128            # cells per batch of the kernel (its workgroup size)
GROUP = 32             # degrees per group


class Spectra:
    def __init__(self, engine, lmax: int):
        e = self.e = engine
        plan = e.plan
        self.lmax = L = ms.check_lmax(lmax, e.layout.N)
        self.tab = ms.rank_tables(e.geo, L, e.device)
        self.S = plan.S
        self.cells = plan.T * plan.n * plan.n
        pad, unp = ms.rank_index(plan)
        self.pad = torch.as_tensor(pad, device=e.device)
        self.unp = torch.as_tensor(unp, device=e.device)
        self.hip = use_hip(e)
        self._pack_index = None                     # synthesis: (l, m) of the packed rows, on the device
        self._abT = None                            # synthesis: the factors a, b as [m][l]
        self._bounds = {}                           # synthesis: chunks -> (host int array, device int32 tensor)
        # ---- host-side shape contract checks ------------------------------------
        t = self.tab
        assert t.cells == self.cells and self.cells >= 1
        assert t.cell.dtype == torch.float64 and t.cell.shape == (self.cells, 4) and t.cell.is_contiguous()
        for x in (t.a, t.b):
            assert x.dtype == torch.float64 and x.shape == (L + 1, L + 1) and x.is_contiguous()
        assert t.c.dtype == torch.float64 and t.c.shape == (L + 1,)
        for ix, lim in ((self.pad, self.S), (self.unp, self.cells)):
            assert ix.dtype == torch.int32 and ix.shape == (self.cells,) and ix.is_contiguous()
            assert int(ix.min()) >= 0 and int(ix.max()) < lim
        # the padded table addresses interior cells only
        assert_interior(plan, pad)
        if self.hip:
            from . import native
            self.lib = native.require_native()
            self.dcode = native.dtype_code(e.dtype)
            assert t.cell.data_ptr() % 32 == 0
            # slabs: a grid of about twice the compute units, every slab whole batches, none empty
            cus = torch.cuda.get_device_properties(e.device).multi_processor_count
            self._cus = cus
            nbatch = -(-self.cells // BATCH)
            want = max(1, min(nbatch, round(2 * cus / (L + 1)), 65535))
            per = -(-nbatch // want)
            self.slab_cells = per * BATCH
            self.slabs = -(-nbatch // per)
            assert (self.slabs - 1) * self.slab_cells < self.cells <= self.slabs * self.slab_cells
            self.RP = -(-(L + 1) // GROUP) * GROUP
            self.partial = torch.empty((self.slabs, L + 1, self.RP, 16), dtype=torch.float64, device=e.device)

    # ---- kernel ----------------------------------------------------------------------
    def _analyse(self, x: torch.Tensor, idx: torch.Tensor, lim: int) -> torch.Tensor:
        from . import native
        e, t, L = self.e, self.tab, self.lmax
        if x.dim() != 2 or x.shape[1] != lim:
            raise ValueError(f"spectra: [C, {lim}] expected, not {tuple(x.shape)}")
        C = x.shape[0]
        if not 1 <= C <= ms.MAX_CHANNELS:
            raise ValueError(f"spectra: 1 .. {ms.MAX_CHANNELS} channels per call, not {C}")
        assert x.is_contiguous() and x.dtype == e.dtype and x.is_cuda
        out = torch.zeros((C, 2, L + 1, L + 1), dtype=torch.float64, device=e.device)
        d = native.SpectraDesc()
        d.Q, d.idx, d.cell = native.ptr(x), native.ptr(idx), native.ptr(t.cell)
        d.a, d.b, d.c = native.ptr(t.a), native.ptr(t.b), native.ptr(t.c)
        d.partial, d.out = native.ptr(self.partial), native.ptr(out)
        d.cs, d.cells, d.C, d.lmax = lim, self.cells, C, L
        d.slabs, d.slab_cells, d.RP = self.slabs, self.slab_cells, self.RP
        native.check(self.lib.stsp_spectra_launch(self.dcode, d, native.current_stream_handle(e.device)),
                     "spectra kernel")
        return out

    # ---- this rank's part of the coefficients: [C, 2, L+1, L+1] float64 --------------------
    def partial_fields(self, q: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Every channel of the padded state ``q`` [F, S] (default: the engine's)."""
        q = self.e.state if q is None else q
        if self.hip:
            return self._analyse(q, self.pad, self.S)
        if q.dim() != 2 or q.shape[1] != self.S:
            raise ValueError(f"spectra: [C, {self.S}] expected, not {tuple(q.shape)}")
        return ms.analyse(q[:, self.pad.long()], self.tab)

    def partial_tiles(self, x: torch.Tensor) -> torch.Tensor:
        """The channels of an unpadded array ``x`` [C, T, n, n]."""
        x = x.reshape(x.shape[0], -1)
        if self.hip:
            return self._analyse(x.contiguous(), self.unp, self.cells)
        return ms.analyse(x, self.tab)

    # ---- synthesis: coefficients [C, 2, L+1, L+1] to this rank's cells [C, T, n, n] ----------
    def default_chunks(self) -> int:
        """Order chunks of the synthesis launch: the fewest that make the grid
        (cell batches x chunks) at least twice the compute units."""
        if not self.hip:
            return 1
        nbatch = -(-self.cells // BATCH)
        return max(1, min(self.lmax + 1, -(-2 * self._cus // nbatch)))

    def synthesise(self, coeffs: torch.Tensor, chunks: Optional[int] = None) -> torch.Tensor:
        """[C, T, n, n] float64 on the engine's device: the band-limited field of
        ``coeffs`` [C, 2, L+1, L+1] float64 (cos, sin; [l, m]) at this rank's cell
        centres.  Entries with m > l and S_l0 are not read.  ``chunks``: the
        kernel's order chunks (default: ``default_chunks()``); the twin ignores
        all but its range."""
        e, t, L = self.e, self.tab, self.lmax
        if not isinstance(coeffs, torch.Tensor) or coeffs.dim() != 4 or coeffs.shape[1] != 2 \
                or coeffs.shape[2] != coeffs.shape[3]:
            raise ValueError(f"synthesise: coefficients [C, 2, L+1, L+1] expected, not "
                             f"{tuple(getattr(coeffs, 'shape', ()))}")
        if coeffs.dtype != torch.float64:
            raise ValueError(f"synthesise: float64 coefficients expected, not {coeffs.dtype}")
        C = coeffs.shape[0]
        if not 1 <= C <= ms.MAX_CHANNELS:
            raise ValueError(f"synthesise: 1 .. {ms.MAX_CHANNELS} channels per call, not {C}")
        if coeffs.shape[2] != L + 1:
            raise ValueError(f"synthesise: coefficients to degree {coeffs.shape[2] - 1}, this object's lmax is {L}")
        if chunks is None:
            chunks = self.default_chunks()
        bounds = ms.chunk_bounds(L, chunks)            # ValueError outside 1 .. L + 1
        plan = e.plan
        coeffs = coeffs.to(e.device)
        if not self.hip:
            out = ms.synthesise(ms.clean_coeffs(coeffs), t)
            return out.reshape(C, plan.T, plan.n, plan.n)
        from . import native
        if self._pack_index is None:
            self._pack_index = tuple(torch.as_tensor(x, device=e.device) for x in ms.pack_index(L))
        K = ms.pack_coeffs(coeffs, self._pack_index)
        assert K.shape == (ms.packed_rows(L), 16) and K.is_contiguous()
        if chunks not in self._bounds:
            host = (ctypes.c_int * (chunks + 1))(*bounds)
            self._bounds[chunks] = (host, torch.tensor(bounds, dtype=torch.int32, device=e.device))
        host, dev = self._bounds[chunks]
        assert host[0] == 0 and host[chunks] == L + 1 and all(host[k] < host[k + 1] for k in range(chunks))
        out = torch.empty((C, self.cells), dtype=torch.float64, device=e.device)
        rec = None
        if chunks > 1:
            rec = torch.empty((chunks, C, self.cells), dtype=torch.float64, device=e.device)
        d = native.SynthDesc()
        d.K, d.idx, d.cell = native.ptr(K), native.ptr(self.unp), native.ptr(t.cell)
        if self._abT is None:
            # the recurrence walks l at fixed m: [m][l] copies make its factors consecutive in memory
            self._abT = (t.a.T.contiguous(), t.b.T.contiguous())
        d.a, d.b, d.c = native.ptr(self._abT[0]), native.ptr(self._abT[1]), native.ptr(t.c)
        d.bounds, d.bounds_dev = ctypes.addressof(host), native.ptr(dev)
        d.rec, d.out = (native.ptr(rec) if rec is not None else None), native.ptr(out)
        d.k_rows, d.rec_elems = K.shape[0], (rec.numel() if rec is not None else 0)
        d.cells, d.idx_limit, d.C, d.lmax, d.chunks = self.cells, self.cells, C, L, chunks
        native.check(self.lib.stsp_synth_launch(d, native.current_stream_handle(e.device)), "synthesis kernel")
        return out.reshape(C, plan.T, plan.n, plan.n)

    @staticmethod
    def power(coeffs: torch.Tensor) -> torch.Tensor:
        """[C, L+1] power per degree of the coefficients [C, 2, L+1, L+1]."""
        return ms.power(coeffs)
