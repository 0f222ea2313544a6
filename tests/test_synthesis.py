"""Spherical-harmonic synthesis (models/spectra.py, ops/spectra.py, the solver's
``synthesise`` / ``filtered_field`` / ``band_field`` / ``streamfunction`` /
``velocity_potential`` and the ``synth`` command) with the PyTorch twin on the
CPU.  Every figure is printed before anything is asserted."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import stsphere as S
from stsphere.engine import Engine
from stsphere.models import spectra as ms
from stsphere.models.geometry import DAY, CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout


def _solver(tmp, N=12, nd=1, t=1, case="tc5", model="swe", **io):
    s = S.Solver({"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
                  "grid": {"N": N}, "physics": {"model": model, "case": case}, "time": {"nsteps": 12, "cfl": 0.9},
                  "io": dict({"output_dir": str(tmp)}, **io)}, verbose=False)
    s.initialize()
    return s


def _garbage(c, value=1e300):
    """``c`` with ``value`` in every m > l entry and in S_l0."""
    L = c.shape[-1] - 1
    bad = c.clone()
    bad[..., torch.triu(torch.ones(L + 1, L + 1, dtype=torch.bool), 1)] = value
    bad[:, 1, :, 0] = value
    return bad


def _random_coeffs(C, L, seed):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn((C, 2, L + 1, L + 1), dtype=torch.float64, generator=g)
    c = c * torch.tril(torch.ones(L + 1, L + 1, dtype=torch.float64))
    c[:, 1, :, 0] = 0.0
    return c


# ---- 1. TC2: psi = -R u0 sin(lat), chi = 0 ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tc2(N):
    """(psi error / max |exact|, max |chi| / max |psi|) of the TC2 initial state at lmax = 12."""
    e = Engine(ShallowWater("tc2"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N))
    sp = e.spectra(12)
    c = sp.partial_tiles(e.derived()[0][:2])
    psi_c, chi_c = ms.helmholtz(c[0], c[1], e.grid.radius)
    psi, chi = sp.synthesise(torch.stack([psi_c, chi_c]))
    u0 = 2.0 * math.pi * e.grid.radius / (12.0 * DAY)
    exact = -e.grid.radius * u0 * sp.tab.cell[:, 0].reshape(psi.shape)
    return float((psi - exact).abs().max() / exact.abs().max()), float(chi.abs().max() / psi.abs().max())


def test_tc2_streamfunction():
    """Second order in the cell width.  Measured with the twin: psi error 9.14e-4
    at C24 and 2.27e-4 at C48 (ratio 4.02), chi / psi 2.2e-5 at C24."""
    (e24, x24), (e48, x48) = _tc2(24), _tc2(48)
    print(f"tc2 psi error: C24 {e24:.3e} C48 {e48:.3e} ratio {e24 / e48:.3f}; chi / psi: C24 {x24:.3e} C48 {x48:.3e}")
    assert e24 <= 1.2e-3 and e48 <= 3e-4
    assert 3.5 <= e24 / e48 <= 4.5
    assert x24 <= 3e-5


def test_tc2_streamfunction_through_the_solver(tmp_path):
    """``Solver.streamfunction`` is the same chain (C24)."""
    s = _solver(tmp_path, N=24, case="tc2")
    psi = s.streamfunction(12)
    assert psi.shape == (6, 24, 24) and psi.dtype == np.float64
    u0 = 2.0 * math.pi * s.grid.radius / (12.0 * DAY)
    exact = -s.grid.radius * u0 * ms.grid_tables(s.grid, 12).cell[:, 0].numpy().reshape(6, 24, 24)
    err = np.abs(psi - exact).max() / np.abs(exact).max()
    print(f"solver tc2 psi error C24 {err:.3e}")
    assert err <= 1.2e-3


# ---- 2. a cell centre on the pole ------------------------------------------------------------------
def test_pole_cell_at_odd_N():
    """C9, lmax = 17: at the north pole (mu = 1, cos phi = 0 exactly) only m = 0
    contributes and P_l0(1) = sqrt(2l + 1).  Measured difference 8e-16 of the
    value; bound 1e-12 of sum_l |C_l0| sqrt(2l + 1)."""
    e = Engine(ShallowWater("tc5"), TileLayout(9, 1, 1, ng=2), grid=CubedSphereGrid(9))
    L = 17
    sp = e.spectra(L)
    cell = sp.tab.cell
    at = torch.nonzero((cell[:, 1] == 0.0) & (cell[:, 0] == 1.0)).reshape(-1)
    assert at.numel() == 1 and float(cell[at[0], 2]) == 0.0
    c = _random_coeffs(2, L, 11)
    f = sp.synthesise(c).reshape(2, -1)[:, at[0]]
    root = torch.sqrt(2.0 * torch.arange(L + 1, dtype=torch.float64) + 1.0)
    want, scale = (c[:, 0, :, 0] * root).sum(1), (c[:, 0, :, 0].abs() * root).sum(1)
    d = (f - want).abs() / scale
    print("pole cell: " + " ".join(f"{v:.1e}" for v in d.tolist()))
    assert bool(torch.isfinite(sp.synthesise(c)).all()) and float(d.max()) <= 1e-12


# ---- 3. linearity, exact to rounding ---------------------------------------------------------------
def test_linearity_and_identities(tmp_path):
    s = _solver(tmp_path)
    s.step(2)
    L = 23
    h = s.global_field("h")
    full = s.band_field("h", L)
    assert full.shape == (6, 12, 12) and full.dtype == np.float64
    for k in (0, 7, 22):
        lo, hi = s.band_field("h", L, 0, k), s.band_field("h", L, k + 1, L)
        d = np.abs(lo + hi - full).max() / np.abs(h).max()
        print(f"band split at {k}: {d:.2e}")
        assert d <= 1e-12
    assert np.array_equal(s.filtered_field("h", L, np.ones(L + 1)), full)
    assert np.array_equal(s.band_field("h", L, 0, L), full)
    c = torch.as_tensor(np.stack([s.sh_coefficients("vorticity", L), s.sh_coefficients("divergence", L)]))
    psi_c, chi_c = ms.helmholtz(c[0], c[1], s.grid.radius)
    assert np.array_equal(s.streamfunction(L), s.synthesise(psi_c.numpy()))
    both = s.synthesise(torch.stack([psi_c, chi_c]).numpy())
    assert both.shape == (2, 6, 12, 12) and np.array_equal(both[1], s.velocity_potential(L))
    # the definitions
    assert ms.band_factors(5, 2, 3).tolist() == [0, 0, 1, 1, 0, 0] and ms.band_factors(2).tolist() == [1, 1, 1]
    f = ms.exp_factors(8, 4, 2)
    assert float(f[0]) == 1.0 and abs(float(f[4]) - math.exp(-1.0)) <= 1e-15 and bool((f[1:] < f[:-1]).all())
    il = ms.inverse_laplacian_factors(3, 2.0)
    assert il.tolist() == [0.0, -2.0, -4.0 / 6.0, -4.0 / 12.0]
    x = torch.ones(2, 4, 4, dtype=torch.float64)
    assert torch.equal(ms.scale_degrees(x, il)[1], il[:, None].expand(4, 4))


# ---- 4. the upper triangle and S_l0 are not read -------------------------------------------------
def test_upper_triangle_is_not_read():
    e = Engine(ShallowWater("tc5"), TileLayout(12, 2, 1, ng=2), grid=CubedSphereGrid(12))
    sp = e.spectra(17)
    c = _random_coeffs(3, 17, 5)
    a, b = sp.synthesise(c), sp.synthesise(_garbage(c))
    assert a.shape == (3, e.plan.T, e.plan.n, e.plan.n) and a.dtype == torch.float64
    assert bool(torch.isfinite(b).all()) and torch.equal(a, b)
    assert torch.equal(a.reshape(3, -1), ms.synthesise(c, sp.tab))


# ---- 5. what the kernel reads ---------------------------------------------------------------------
@pytest.mark.parametrize("C,L", [(1, 0), (3, 1), (8, 17), (5, 33)])
def test_packing_round_trips(C, L):
    c = _random_coeffs(C, L, 3 + L)
    p = ms.pack_coeffs(c)
    assert p.shape == (ms.packed_rows(L), 16) and p.dtype == torch.float64
    assert torch.equal(ms.unpack_coeffs(p, C, L), c)
    assert torch.equal(ms.pack_coeffs(_garbage(c)), p)
    assert bool((p[:, 2 * C:] == 0).all()) and bool((p[:L + 1, 1::2] == 0).all())
    l, m = ms.pack_index(L)
    assert np.array_equal(np.arange(len(l)), m * (L + 1) - m * (m - 1) // 2 + l - m) and bool((l >= m).all())
    for ch, s, ll, mm in ((0, 0, L, 0), (C - 1, 1, L, L), (C - 1, 0, L, L // 2)):
        row = mm * (L + 1) - mm * (mm - 1) // 2 + ll - mm
        assert float(p[row, 2 * ch + s]) == float(c[ch, s, ll, mm])


@pytest.mark.parametrize("L", [0, 1, 17, 33, 95, 1023])
def test_chunk_bounds(L):
    """Contiguous, none empty, 0 .. L exactly once; about equal rows: no chunk
    holds more than the ideal share plus one order's rows."""
    total = ms.packed_rows(L)
    for k in sorted({1, 2, 3, min(7, L + 1), L + 1} & set(range(1, L + 2))):
        b = ms.chunk_bounds(L, k)
        assert len(b) == k + 1 and b[0] == 0 and b[-1] == L + 1 and all(x < y for x, y in zip(b, b[1:]))
        rows = [sum(L + 1 - m for m in range(x, y)) for x, y in zip(b, b[1:])]
        assert sum(rows) == total and max(rows) <= total / k + (L + 1)
    for bad in (0, L + 2, -1, 1.5, True):
        with pytest.raises(ValueError):
            ms.chunk_bounds(L, bad)


# ---- 6. host errors ----------------------------------------------------------------------------------
def test_host_errors(tmp_path):
    e = Engine(ShallowWater("tc5"), TileLayout(12, 1, 1, ng=2), grid=CubedSphereGrid(12))
    sp = e.spectra(5)
    ok = torch.zeros(2, 2, 6, 6, dtype=torch.float64)
    assert sp.synthesise(ok).shape == (2, 6, 12, 12)
    assert sp.synthesise(ok, chunks=6).shape == (2, 6, 12, 12)
    for bad in (torch.zeros(2, 6, 6, dtype=torch.float64), torch.zeros(2, 3, 6, 6, dtype=torch.float64),
                torch.zeros(2, 2, 6, 5, dtype=torch.float64),                       # shape
                ok.float(),                                                         # dtype
                torch.zeros(0, 2, 6, 6, dtype=torch.float64), torch.zeros(9, 2, 6, 6, dtype=torch.float64),   # C
                torch.zeros(2, 2, 5, 5, dtype=torch.float64), torch.zeros(2, 2, 7, 7, dtype=torch.float64)):  # L
        with pytest.raises(ValueError):
            sp.synthesise(bad)
    for chunks in (0, 7, -1):
        with pytest.raises(ValueError):
            sp.synthesise(ok, chunks=chunks)
    s = _solver(tmp_path / "a")
    for call in (lambda: s.band_field("nope", 5), lambda: s.filtered_field("nope", 5, np.ones(6)),
                 lambda: s.band_field("u", 5), lambda: s.band_field("h", 24),
                 lambda: s.filtered_field("h", 5, np.ones(5)), lambda: s.band_field("h", 5, 4, 3),
                 lambda: s.synthesise(np.zeros((2, 6, 5))), lambda: s.synthesise(np.zeros((2, 25, 25))),
                 lambda: s.streamfunction(24)):
        with pytest.raises(ValueError):
            call()
    assert s.band_field("pv", 5).shape == (6, 12, 12)
    d = _solver(tmp_path / "b", model="diffusion", case="lima_flag")
    assert d.band_field(d.fields[0], 5).shape == (6, 12, 12)
    for call in (lambda: d.streamfunction(5), lambda: d.velocity_potential(5), lambda: d.band_field("vorticity", 5)):
        with pytest.raises(ValueError, match="shallow-water"):
            call()


def test_launcher_refuses_contract_violations():
    """The launcher checks every shape contract again and returns nonzero before
    anything is launched (so this runs without a GPU; no pointer but the host
    chunk bounds is dereferenced)."""
    import ctypes
    from stsphere.ops import native
    lib = native.load()
    L, C, cells, chunks = 5, 2, 864, 3
    host = (ctypes.c_int * 8)(0, 2, 4, 6, 0, 0, 0, 0)

    def desc(**kw):
        d = native.SynthDesc()
        for k in ("K", "idx", "cell", "a", "b", "c", "bounds_dev", "rec", "out"):
            setattr(d, k, 0x1000)
        d.bounds = ctypes.addressof(host)
        d.k_rows, d.rec_elems = ms.packed_rows(L), chunks * C * cells
        d.cells, d.idx_limit, d.C, d.lmax, d.chunks = cells, cells, C, L, chunks
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    assert ctypes.sizeof(native.SynthDesc) == lib.stsp_synth_desc_size()
    assert lib.stsp_synth_launch(None, None) == 1
    bad = [dict(K=None), dict(idx=None), dict(cell=None), dict(a=None), dict(b=None), dict(c=None), dict(out=None),
           dict(bounds=None), dict(bounds_dev=None), dict(rec=None),
           dict(C=0), dict(C=9), dict(lmax=-1), dict(lmax=1024), dict(cells=0),
           dict(cell=0x1010), dict(idx=0x1002), dict(idx_limit=cells + 1), dict(idx_limit=cells - 1),
           dict(k_rows=ms.packed_rows(L) - 1), dict(chunks=0), dict(chunks=7), dict(chunks=2), dict(chunks=4),
           dict(rec_elems=chunks * C * cells - 1)]
    for kw in bad:
        assert lib.stsp_synth_launch(ctypes.byref(desc(**kw)), None) == 1, kw
    for b in ((1, 2, 4, 6), (0, 2, 2, 6), (0, 4, 2, 6), (0, 2, 4, 5), (0, 2, 4, 7)):
        host[:4] = b
        assert lib.stsp_synth_launch(ctypes.byref(desc()), None) == 1, b


# ---- 7. ranks --------------------------------------------------------------------------------------
def _products(s):
    return {"psi": s.streamfunction(9), "chi": s.velocity_potential(9), "band": s.band_field("h", 9, 2, 6)}


def test_six_virtual_ranks_equal_one_rank(tmp_path):
    one, six = _solver(tmp_path / "a"), _solver(tmp_path / "b", nd=6)
    assert six.mode == "virtual" and len(six.engines) == 6
    one.step(2)
    six.step(2)
    a, b = _products(one), _products(six)
    for n in a:
        d = np.abs(a[n] - b[n]).max() / np.abs(a[n]).max()
        print(f"six virtual ranks {n}: {d:.2e}")
        assert a[n].shape == (6, 12, 12) and d <= 1e-12, n


def _spmd_worker(rank, world, port, cfg, steps, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    s = S.Solver(cfg, verbose=False)
    try:
        s.initialize()
        s.step(steps)
        got = _products(s)
        if rank == 0:
            np.savez(os.path.join(outdir, "r0.npz"), **got)
        else:
            assert all(v is None for v in got.values())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_gloo_two_ranks_equal_one_rank(tmp_path):
    """SPMD ranks: the coefficients are broadcast from rank 0, every rank
    synthesises its own cells, rank 0 assembles; other ranks get None."""
    import socket
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    one = _solver(tmp_path)
    cfg = dict(one.config, parallelization=dict(one.config["parallelization"], num_devices=2))
    mp.spawn(_spmd_worker, args=(2, port, cfg, 3, str(tmp_path)), nprocs=2, join=True)
    one.step(3)
    got, ref = np.load(os.path.join(str(tmp_path), "r0.npz")), _products(one)
    for n in ref:
        d = np.abs(got[n] - ref[n]).max() / np.abs(ref[n]).max()
        print(f"two gloo ranks {n}: {d:.2e}")
        assert d <= 1e-12, n


# ---- 8. the command --------------------------------------------------------------------------------
def test_cli(tmp_path):
    from stsphere.__main__ import main as cli
    s = _solver(tmp_path / "run", history_interval=6)
    s.run()
    hc = str(tmp_path / "run" / "history.zarr")
    out = str(tmp_path / "psi.npz")
    assert cli(["synth", hc, "streamfunction", "9", out]) == 0
    r = np.load(out)
    ref = s.streamfunction(9)
    assert r["field"].shape == (3, 6, 12, 12) and r["time"].shape == (3,)
    d = np.abs(r["field"][-1] - ref).max() / np.abs(ref).max()
    print(f"cli streamfunction, last frame: {d:.2e}")
    assert d <= 1e-12
    assert cli(["synth", hc, "velocity_potential", "9", out]) == 0
    assert np.abs(np.load(out)["field"][-1] - s.velocity_potential(9)).max() <= 1e-12 * np.abs(ref).max()
    assert cli(["synth", hc, "h", "9", out, "--band", "2", "6"]) == 0
    ref = s.band_field("h", 9, 2, 6)
    assert np.abs(np.load(out)["field"][-1] - ref).max() <= 1e-12 * np.abs(ref).max()
    for bad in (["synth", hc, "pv", "9", out], ["synth", hc, "u", "9", out], ["synth", hc, "h", "24", out]):
        with pytest.raises(ValueError):
            cli(bad)
    # streamfunction needs h, mx, my, mz: the same error as ``ke``
    t = _solver(tmp_path / "sel", history_interval=12, history_fields=["h"])
    t.run()
    with pytest.raises(ValueError, match="no array"):
        cli(["synth", str(tmp_path / "sel" / "history.zarr"), "streamfunction", "9", out])
