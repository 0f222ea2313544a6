"""The gfx950 gradient synthesis kernel (ops/csrc/grad_synth_kernel.hip) against its
termwise PyTorch twin (models/spectra.py::gradient) and through the solver.  Bound: the
project's fp64 bound for the synthesis, per channel max |kernel - twin| <= 1e-12 max |twin|
(the rearrangement measures 3e-15 on the CPU).  Every figure is printed before it is asserted."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine
from stsphere.models import spectra as ms
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout

pytestmark = pytest.mark.gpu

BOUND = 1e-12
# (N, tiles per edge, lmax).  (9, 1): a cell centre on each pole and a ragged last batch of 102
# cells; 2N - 1 is the largest degree; 31, 32, 33 put order 1's rows at and across the group of 32
CASES = [(9, 1, 1), (9, 1, 2), (9, 1, 17), (12, 1, 1), (12, 1, 2), (12, 1, 23),
         (24, 2, 1), (24, 2, 2), (24, 2, 31), (24, 2, 32), (24, 2, 33), (24, 2, 47)]


@functools.lru_cache(maxsize=None)
def _engines(N, t):
    cpu = Engine(ShallowWater("tc5"), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N))
    gpu = Engine(ShallowWater("tc5"), cpu.layout, grid=cpu.grid, dtype=torch.float64, device="cuda:0", backend="hip",
                 dt=cpu.dt)
    return gpu, cpu


def _random(C, L, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn((C, 2, L + 1, L + 1), dtype=torch.float64, generator=g)
    c = c * torch.tril(torch.ones(L + 1, L + 1, dtype=torch.float64))
    c[:, 1, :, 0] = 0.0
    return c / (torch.arange(L + 1, dtype=torch.float64)[:, None] + 1.0) ** 2


def _diff(got, ref):
    got, ref = got.reshape(ref.shape[0], -1).cpu(), ref.reshape(ref.shape[0], -1)
    return ((got - ref).abs().amax(1) / ref.abs().amax(1)).tolist()


def _check(tag, N, t, L, c, chunk_list):
    gpu, cpu = _engines(N, t)
    sp = gpu.spectra(L)
    assert sp.hip and not cpu.spectra(L).hip
    ref = ms.gradient(c, cpu.spectra(L).tab, cpu.grid.radius)
    bad = []
    for chunks in chunk_list:
        got = sp.gradient(c.to(gpu.device), chunks=chunks)
        again = sp.gradient(c.to(gpu.device), chunks=chunks)
        assert got.dtype == torch.float64 and got.shape == (c.shape[0], 2, gpu.plan.T, gpu.plan.n, gpu.plan.n)
        d = _diff(got, ref)
        print(f"{tag} C{N} t={t} lmax {L} chunks {chunks}: " + " ".join(f"{v:.1e}" for v in d))
        bad += [(chunks, v) for v in d if not v <= BOUND]
        assert torch.equal(got, again), "two calls differ"
    assert not bad, bad


@pytest.mark.parametrize("C", [1, 2, 3])
@pytest.mark.parametrize("N,t,L", CASES)
def test_kernel_against_twin(N, t, L, C):
    """Random coefficients; one chunk, two, one per order and the default; three
    channels take two launches.  Two calls agree bit for bit."""
    chunk_list = sorted({1, min(2, L), L, _engines(N, t)[0].spectra(L).default_grad_chunks()})
    _check(f"random C={C}", N, t, L, _random(C, L, 100 * C + L), chunk_list)


@pytest.mark.parametrize("which", ["C_L0", "C_LL", "S_LL", "C_(m+1)m", "C_L(L-1)"])
def test_single_coefficients(which):
    """C9, lmax 17, one coefficient in the second channel: the order-0 rider
    alone (C_L0), the sectoral start alone (C_LL, S_LL: Hf and every row but the
    first are zero), the second row of a column (C_(m+1)m, whose shifted entry
    sits on the sectoral row), and l = L of order L - 1, the shifted column's
    last row."""
    L = 17
    c = torch.zeros((2, 2, L + 1, L + 1), dtype=torch.float64)
    l, m, s = {"C_L0": (L, 0, 0), "C_LL": (L, L, 0), "S_LL": (L, L, 1), "C_(m+1)m": (6, 5, 0),
               "C_L(L-1)": (L, L - 1, 0)}[which]
    c[1, s, l, m] = 1.5
    gpu, cpu = _engines(9, 1)
    ref = ms.gradient(c, cpu.spectra(L).tab, cpu.grid.radius)
    for chunks in (1, L):
        got = gpu.spectra(L).gradient(c.to(gpu.device), chunks=chunks).reshape(2, 2, -1).cpu()
        d = float((got[1] - ref[1]).abs().max() / ref[1].abs().max())
        print(f"{which} chunks {chunks}: {d:.1e}; the empty channel {float(got[0].abs().max()):.1e}")
        assert d <= BOUND and float(got[0].abs().max()) == 0.0


def test_default_chunks_and_lmax_zero():
    gpu, _ = _engines(24, 2)
    cus = torch.cuda.get_device_properties(gpu.device).multi_processor_count
    k = gpu.spectra(33).default_grad_chunks()
    assert k == max(1, min(33, -(-2 * cus // 27)))
    z = gpu.spectra(0).gradient(torch.ones((1, 2, 1, 1), dtype=torch.float64))
    assert z.is_cuda and z.shape == (1, 2, gpu.plan.T, 12, 12) and float(z.abs().max()) == 0.0


def _cfg(out, device_type):
    return {"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": device_type},
            "grid": {"N": 24, "dtype": "float64"}, "physics": {"model": "swe", "case": "tc5"}, "time": {"nsteps": 4},
            "io": {"output_dir": str(out)}}


def test_solver_winds(tmp_path):
    """A two-tile HIP solver against the torch-backend solver on the same state."""
    hip, ref = S.Solver(_cfg(tmp_path / "a", "gpu"), verbose=False), S.Solver(_cfg(tmp_path / "b", "cpu"), verbose=False)
    hip.initialize()
    ref.initialize()
    hip.step(2)
    assert hip.engines[0].spectra(20).hip and not ref.engines[0].spectra(20).hip
    ref.engines[0].set_state(hip.engines[0].tiles_view().cpu())
    for name in ("rotational_wind", "divergent_wind"):
        a, b = getattr(hip, name)(20), getattr(ref, name)(20)
        d = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"solver {name}: {d:.1e}")
        assert a.shape == (2, 6, 24, 24) and a.dtype == np.float64 and d <= BOUND
    hip.close()
    ref.close()


def test_launcher_refuses_contract_violations():
    """Every bad field returns nonzero before anything is launched (no pointer
    but the host chunk bounds is dereferenced)."""
    from stsphere.ops import native
    lib = native.load()
    L, C, cells, chunks = 5, 2, 864, 3
    host = (ctypes.c_int * 4)(1, 2, 4, 6)

    def desc(**kw):
        d = native.GradSynthDesc()
        for k in ("K", "idx", "cell", "a", "b", "c", "bounds_dev", "rec", "out"):
            setattr(d, k, 0x1000)
        d.bounds = ctypes.addressof(host)
        d.k_rows, d.rec_elems, d.inv_radius = ms.grad_rows(L), chunks * 2 * C * cells, 1.0
        d.cells, d.idx_limit, d.C, d.lmax, d.chunks = cells, cells, C, L, chunks
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert ctypes.sizeof(native.GradSynthDesc) == lib.stsp_grad_synth_desc_size()
    assert lib.stsp_grad_synth_launch(None, None) == 1
    bad = [dict(K=None), dict(idx=None), dict(cell=None), dict(a=None), dict(b=None), dict(c=None), dict(out=None),
           dict(bounds=None), dict(bounds_dev=None), dict(rec=None),
           dict(C=0), dict(C=3), dict(lmax=0), dict(lmax=1024), dict(cells=0), dict(inv_radius=0.0),
           dict(inv_radius=float("nan")), dict(cell=0x1010), dict(idx=0x1002), dict(idx_limit=cells + 1),
           dict(k_rows=ms.packed_rows(L)), dict(chunks=0), dict(chunks=6), dict(chunks=2),
           dict(rec_elems=chunks * 2 * C * cells - 1)]
    for kw in bad:
        assert lib.stsp_grad_synth_launch(ctypes.byref(desc(**kw)), None) == 1, kw
    for b in ((0, 2, 4, 6), (1, 2, 2, 6), (1, 4, 2, 6), (1, 2, 4, 5), (1, 2, 4, 7)):
        host[:4] = b
        assert lib.stsp_grad_synth_launch(ctypes.byref(desc()), None) == 1, b
