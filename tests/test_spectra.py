"""Spherical-harmonic spectra (models/spectra.py): the PyTorch twin, its host
errors and the solver plumbing, on the CPU.  The quadrature is the midpoint
rule on the cubed-sphere cells, second order in the cell width: that is what
the bounds assert (lmax = 12 unless stated)."""
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
from stsphere.utils import zarr_lite

LMAX = 12
HARMONICS = [(3, 2, "c"), (5, 5, "s"), (8, 4, "c"), (12, 7, "s")]


@functools.lru_cache(maxsize=None)
def _tables(N, lmax=LMAX):
    return ms.grid_tables(CubedSphereGrid(N), lmax)


@functools.lru_cache(maxsize=None)
def _one_harmonic(N, l, m, part):
    """(own coefficient - 1, largest other |coefficient|, Parseval relative
    difference) of the sampled harmonic (l, m, part) at C<N>."""
    tb = _tables(N)
    f = ms.sample_harmonic(tb, l, m, part)
    c = ms.analyse(f[None], tb)
    s = 0 if part == "c" else 1
    own = float(c[0, s, l, m])
    total = float(ms.power(c)[0].sum())
    meansq = float((tb.cell[:, 3] * f * f).sum())
    c[0, s, l, m] = 0.0
    return own - 1.0, float(c.abs().max()), total / meansq - 1.0


@pytest.mark.parametrize("l,m,part", HARMONICS)
def test_normalisation_and_leakage(l, m, part):
    """C24: the own coefficient within 3e-4 of 1 (measured 1.7e-4 to 2.6e-4),
    every other coefficient <= 4e-4 (measured <= 2.5e-4)."""
    own, leak, _ = _one_harmonic(24, l, m, part)
    print(f"C24 ({l},{m},{part}): own - 1 = {own:.3e}, leakage {leak:.3e}")
    assert abs(own) <= 3e-4 and leak <= 4e-4


def test_second_order():
    """C24 -> C48: the own-coefficient error of each of the four harmonics falls
    by a factor in 3.5 .. 4.5 (measured 4.01 to 4.22), and so does the leakage
    bound's own quantity, the largest leakage over the four (measured 4.05).
    Per harmonic the leakage ratios are 4.55, 4.05, 3.99, 4.24: the 4.55 is
    (3,2,c), whose leakage (3.9e-5) is six times below the largest."""
    own, leak = {}, {}
    for N in (24, 48):
        r = [_one_harmonic(N, *h) for h in HARMONICS]
        own[N], leak[N] = [abs(x[0]) for x in r], [x[1] for x in r]
    for h, a, b, la, lb in zip(HARMONICS, own[24], own[48], leak[24], leak[48]):
        print(f"{h}: own ratio {a / b:.3f}, leakage ratio {la / lb:.3f}")
        assert 3.5 <= a / b <= 4.5, h
    ratio = max(leak[24]) / max(leak[48])
    print(f"largest leakage ratio {ratio:.3f}")
    assert 3.5 <= ratio <= 4.5


@pytest.mark.parametrize("l", [0, 1])
def test_constant_and_solid_body_are_exact(l):
    """(0,0) and (1,0): own coefficient 1 to rounding (cube symmetry and the
    exact areas); leakage <= 8e-4 at C24 (measured 5.5e-4 and 6.3e-4)."""
    own, leak, _ = _one_harmonic(24, l, 0, "c")
    print(f"C24 ({l},0,c): own - 1 = {own:.3e}, leakage {leak:.3e}")
    assert abs(own) <= 1e-14 and leak <= 8e-4


@pytest.mark.parametrize("l,m,part", HARMONICS)
def test_parseval(l, m, part):
    """sum_l S_l equals sum_c w_c f_c^2 within 3e-4 relative at C24 (measured <= 2.6e-4)."""
    _, _, d = _one_harmonic(24, l, m, part)
    print(f"C24 ({l},{m},{part}): Parseval {d:.3e}")
    assert abs(d) <= 3e-4


@functools.lru_cache(maxsize=None)
def _engine(N, case, t=1):
    return Engine(ShallowWater(case), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N))


def _nonmean(c):
    """Power [L+1 (m)] per order of coefficients [2, L+1, L+1] without (0, 0)."""
    c = c.clone()
    c[:, 0, 0] = 0.0
    return (c * c).sum(dim=(0, 1))


@pytest.mark.parametrize("N,bound", [(24, 1e-5), (48, 1e-6)])
def test_tc6_is_wavenumber_four(N, bound):
    """TC6 initial h: the fraction of non-mean power outside m in {0, 4, 8}
    (measured 6.0e-7 at C24, 3.6e-8 at C48)."""
    e = _engine(N, "tc6")
    pm = _nonmean(e.spectra(LMAX).partial_fields()[0])
    frac = float(1.0 - (pm[0] + pm[4] + pm[8]) / pm.sum())
    print(f"C{N} tc6: power outside m = 0, 4, 8: {frac:.3e}")
    assert 0.0 <= frac <= bound


def test_tc2_is_degree_two():
    """TC2 (alpha = 0) initial h: (2,0) carries >= 0.9999 of the non-mean power
    at C24 (measured 0.999975)."""
    c = _engine(24, "tc2").spectra(LMAX).partial_fields()[0]
    frac = float(c[0, 2, 0] ** 2 / _nonmean(c).sum())
    print(f"C24 tc2: (2,0) fraction {frac:.6f}")
    assert frac >= 0.9999


@pytest.mark.parametrize("N,bound", [(24, 2.5e-3), (48, 6e-4)])
def test_ke_spectrum_of_solid_body_rotation(N, bound):
    """TC2: v = u0 cos(lat) east is all in degree 1, E_1 = u0^2 / 3 (measured
    error 1.64e-3 at C24, 4.06e-4 at C48); sum_l E_l against the area mean of
    |M|^2 / (2 h^2) to the same bounds; at C24 the rest holds <= 1e-6 E_1
    (measured 6.8e-8)."""
    e = _engine(N, "tc2")
    sp = e.spectra(LMAX)
    c = sp.partial_tiles(e.derived()[0][:2])
    E = ms.ke_spectrum(c[0], c[1], e.grid.radius)
    u0 = 2.0 * math.pi * e.grid.radius / (12.0 * DAY)
    q = e.tiles_view().reshape(4, -1)
    mean = float((sp.tab.cell[:, 3] * 0.5 * (q[1:] ** 2).sum(0) / q[0] ** 2).sum())
    d1, dt = float(E[1] / (u0 * u0 / 3.0) - 1.0), float(E.sum() / mean - 1.0)
    rest = float((E.sum() - E[1]) / E[1])
    print(f"C{N} tc2: E_1 error {d1:.3e}, sum E_l vs mean KE {dt:.3e}, rest / E_1 {rest:.3e}")
    assert float(E[0]) == 0.0 and abs(d1) <= bound and abs(dt) <= bound
    if N == 24:
        assert rest <= 1e-6


def test_round_trip():
    """analyse(synthesise(c)) of a random band-limited c (lmax = 8) returns c
    within the C24 leakage bound 4e-4 times the 1-norm of c."""
    tb = _tables(24, 8)
    g = torch.Generator().manual_seed(7)
    c = torch.randn((2, 2, 9, 9), dtype=torch.float64, generator=g)
    c = c * torch.tril(torch.ones(9, 9, dtype=torch.float64))
    c[:, 1, :, 0] = 0.0
    back = ms.analyse(ms.synthesise(c, tb), tb)
    for k in range(2):
        err = float((back[k] - c[k]).abs().max())
        print(f"round trip channel {k}: {err:.3e} (bound {4e-4 * float(c[k].abs().sum()):.3e})")
        assert err <= 4e-4 * float(c[k].abs().sum())
    assert bool((back[:, 1, :, 0] == 0).all()) and bool((torch.triu(back, 1) == 0).all())


def test_layouts_agree():
    """tiles_per_edge 1, 2 and 3 at C24: only the cell order differs; within
    1e-12 of the largest coefficient (measured 2e-16).  Padded and unpadded
    sources of one array are the same call of the twin."""
    ref = _engine(24, "tc6", 1).spectra(LMAX).partial_fields()
    assert ref.shape == (4, 2, LMAX + 1, LMAX + 1) and ref.dtype == torch.float64
    for t in (2, 3):
        e = _engine(24, "tc6", t)
        sp = e.spectra(LMAX)
        assert e.spectra(LMAX) is sp and e.spectra(5) is not sp
        got = sp.partial_fields()
        for k in range(4):
            d = float((got[k] - ref[k]).abs().max() / ref[k].abs().max())
            print(f"t = {t} channel {k}: {d:.2e}")
            assert d <= 1e-12
        assert torch.equal(sp.partial_tiles(e.tiles_view().contiguous()), got)


def test_ghost_independence():
    e = Engine(ShallowWater("tc5"), TileLayout(12, 2, 1, ng=2), grid=CubedSphereGrid(12))
    sp = e.spectra(7)
    before = sp.partial_fields()
    keep = e.tiles_view().clone()
    e.state.fill_(float("nan"))
    e.tiles_view().copy_(keep)
    assert torch.equal(sp.partial_fields(), before)


def test_fp32_input_gives_float64_output():
    e = Engine(ShallowWater("tc5"), TileLayout(12, 1, 1, ng=2), grid=CubedSphereGrid(12), dtype=torch.float32)
    c = e.spectra(5).partial_fields()
    assert c.dtype == torch.float64 and e.spectra(5).tab.cell.dtype == torch.float64
    ref = ms.analyse(e.tiles_view().reshape(4, -1).double(), e.spectra(5).tab)
    assert torch.equal(c, ref)
    assert ms.power(c).dtype == torch.float64 and ms.power(c).shape == (4, 6)


def test_lmax_zero_and_host_errors(tmp_path):
    e = _engine(24, "tc5")
    c = e.spectra(0).partial_fields()
    assert c.shape == (4, 2, 1, 1) and float(c[0, 1, 0, 0]) == 0.0
    w = e.spectra(0).tab.cell[:, 3]
    assert abs(float(c[0, 0, 0, 0]) / float((w * e.tiles_view()[0].reshape(-1)).sum()) - 1.0) <= 1e-14
    assert e.spectra(47).lmax == 47
    for bad in (48, -1, 1024):
        with pytest.raises(ValueError):
            e.spectra(bad)
    with pytest.raises(ValueError):
        ms.check_lmax(1024, 720)
    assert ms.check_lmax(1023, 720) == 1023
    with pytest.raises(ValueError):
        e.spectra(3).partial_tiles(torch.zeros(9, 6, 24, 24, dtype=torch.float64))
    s = _solver(tmp_path)
    for name in ("u", "v"):
        with pytest.raises(ValueError, match="ke_spectrum"):
            s.spectrum(name, 5)
    with pytest.raises(ValueError):
        s.spectrum("nope", 5)
    with pytest.raises(ValueError):
        s.spectrum("h", 24)
    d = _solver(tmp_path, model="diffusion", case="lima_flag")
    assert d.spectrum(d.fields[0], 5).shape == (6,)
    for call in (lambda: d.spectrum("vorticity", 5), lambda: d.ke_spectrum(5)):
        with pytest.raises(ValueError, match="shallow-water"):
            call()
    with pytest.raises(ValueError, match="io.spectra"):
        _solver(tmp_path, history_interval=5, spectra=24)


def _solver(tmp, N=12, nd=1, t=1, case="tc5", model="swe", **io):
    s = S.Solver({"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
                  "grid": {"N": N}, "physics": {"model": model, "case": case}, "time": {"nsteps": 10, "cfl": 0.9},
                  "io": dict({"output_dir": str(tmp)}, **io)}, verbose=False)
    s.initialize()
    return s


NAMES = ("h", "mz", "vorticity", "divergence", "pv")


def test_six_virtual_ranks_equal_one_rank(tmp_path):
    """Six one-panel virtual ranks, partial sums added in rank order, against
    one rank: within 1e-12 of the largest coefficient."""
    one, six = _solver(tmp_path / "a"), _solver(tmp_path / "b", nd=6)
    assert six.mode == "virtual" and len(six.engines) == 6
    one.step(2)
    six.step(2)
    for n in NAMES:
        a, b = one.sh_coefficients(n, 9), six.sh_coefficients(n, 9)
        assert a.shape == (2, 10, 10) and a.dtype == np.float64
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), n
        assert np.abs(one.spectrum(n, 9) - six.spectrum(n, 9)).max() <= 1e-12 * one.spectrum(n, 9).max(), n
    ka, kb = one.ke_spectrum(9), six.ke_spectrum(9)
    assert ka.shape == (10,) and ka[0] == 0.0 and np.abs(ka - kb).max() <= 1e-12 * ka.max()
    # the solver's numbers are the twin's on the gathered state
    g = torch.as_tensor(one.gather_global())
    ref = ms.power(ms.analyse(g.reshape(4, -1), ms.grid_tables(one.grid, 9)))
    assert np.abs(one.spectrum("h", 9) - ref[0].numpy()).max() <= 1e-12 * float(ref[0].max())


def test_history_spectra(tmp_path):
    """``io.spectra`` writes history_spectra.zarr: power per degree of the
    history fields and ``ke``, ``degree``, ``time``, ``step``; the last frame is
    ``Solver.spectrum`` at the end of the run."""
    s = _solver(tmp_path / "run", history_interval=5, spectra=7)
    s.run()
    hs = str(tmp_path / "run" / "history_spectra.zarr")
    assert sorted(zarr_lite.list_arrays(hs)) == sorted(("h", "mx", "my", "mz", "ke", "degree", "time", "step"))
    assert list(zarr_lite.read_array(hs, "step")) == [0, 5, 10]
    assert list(zarr_lite.read_array(hs, "degree")) == list(range(8))
    assert np.array_equal(zarr_lite.read_array(hs, "time"), zarr_lite.read_array(
        str(tmp_path / "run" / "history.zarr"), "time"))
    for n in ("h", "mx", "my", "mz"):
        a = zarr_lite.read_array(hs, n)
        assert a.shape == (3, 8) and np.array_equal(a[-1], s.spectrum(n, 7)), n
    assert np.array_equal(zarr_lite.read_array(hs, "ke")[-1], s.ke_spectrum(7))
    # selected fields, another model, and nothing without the key
    s = _solver(tmp_path / "sel", history_interval=10, history_fields=["h", "pv"], spectra=5)
    s.run()
    hs = str(tmp_path / "sel" / "history_spectra.zarr")
    assert sorted(zarr_lite.list_arrays(hs)) == sorted(("h", "pv", "ke", "degree", "time", "step"))
    assert np.array_equal(zarr_lite.read_array(hs, "pv")[-1], s.spectrum("pv", 5))
    s = _solver(tmp_path / "off", history_interval=10)
    s.run()
    assert not os.path.exists(tmp_path / "off" / "history_spectra.zarr")


def test_cli_and_plot(tmp_path):
    """``spectrum`` on the cube history gives the frames of history_spectra.zarr
    (first and last frame: a CPU run writes the cube history's middle frames
    from a view of the state); ``plot --spectrum`` and ``spectrum_plot`` draw."""
    from stsphere.__main__ import main as cli
    from stsphere.utils.viz import spectrum_plot
    s = _solver(tmp_path / "run", history_interval=5, spectra=7)
    s.run()
    hc, hs = str(tmp_path / "run" / "history.zarr"), str(tmp_path / "run" / "history_spectra.zarr")
    for n in ("h", "mz", "ke"):
        out = str(tmp_path / f"{n}.npz")
        assert cli(["spectrum", hc, n, "7", out]) == 0
        r, ref = np.load(out), zarr_lite.read_array(hs, n)
        assert r["spectrum"].shape == (3, 8) and list(r["degree"]) == list(range(8))
        for k in (0, -1):
            assert np.abs(r["spectrum"][k] - ref[k]).max() <= 1e-12 * ref[k].max(), (n, k)
    for bad in ("u", "pv"):
        with pytest.raises(ValueError):
            cli(["spectrum", hc, bad, "7", str(tmp_path / "x.npz")])
    with pytest.raises(ValueError):
        cli(["spectrum", hc, "h", "24", str(tmp_path / "x.npz")])
    out = tmp_path / "plots"
    assert cli(["plot", hc, "h", str(out), "--products", "six", "--spectrum", "7"]) == 0
    assert (out / "h_spectrum.png").stat().st_size > 1000
    p = spectrum_plot(s.ke_spectrum(7), str(tmp_path / "ke.png"), title="ke", ylabel="E_l")
    assert os.path.getsize(p) > 1000


def _spmd_worker(rank, world, port, cfg, steps, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    s = S.Solver(cfg, verbose=False)
    try:
        s.initialize()
        s.step(steps)
        got = {n: s.sh_coefficients(n, 9) for n in NAMES}
        got["ke"] = s.ke_spectrum(9)
        if rank == 0:
            np.savez(os.path.join(outdir, "r0.npz"), **got)
        else:
            assert all(v is None for v in got.values())
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_gloo_two_ranks_equal_one_rank(tmp_path):
    """SPMD ranks: the coefficient arrays are added on rank 0; other ranks get None."""
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
    got = np.load(os.path.join(str(tmp_path), "r0.npz"))
    for n in NAMES:
        ref = one.sh_coefficients(n, 9)
        assert np.abs(got[n] - ref).max() <= 1e-12 * np.abs(ref).max(), n
    ref = one.ke_spectrum(9)
    assert np.abs(got["ke"] - ref).max() <= 1e-12 * ref.max()


def test_area_mean_is_summed_error_free():
    """The coefficient (0, 0) is the sum of the products w f to an ulp, however
    much cancels (TC6 one step in: the means of mx and my are 1e-17 of sum |w f|),
    so it does not depend on the cell order of the layout."""
    ref = None
    for t in (1, 2, 3):
        e = Engine(ShallowWater("tc6"), TileLayout(24, t, 1, ng=2), grid=CubedSphereGrid(24))
        e.step(1)
        sp = e.spectra(3)
        wf = e.tiles_view().reshape(4, -1) * sp.tab.cell[:, 3]
        exact = [math.fsum(r.tolist()) for r in wf]
        got = sp.partial_fields()[:, 0, 0, 0].tolist()
        for k in range(4):
            assert abs(got[k] - exact[k]) <= 2.3e-16 * abs(exact[k]), (t, k, got[k], exact[k])
        assert abs(exact[1]) <= 1e-15 * float(wf[1].abs().sum())
        ref = exact if ref is None else ref
        for k in range(4):
            assert abs(exact[k] - ref[k]) <= 2.3e-16 * abs(ref[k]), (t, k)
    x = torch.tensor([[1e16, 1.0, -1e16, 1.0, 1e-3]], dtype=torch.float64)
    assert float(ms.exact_sum(x)[0]) == 2.001 and float(ms.exact_sum(x[:, :1])[0]) == 1e16
