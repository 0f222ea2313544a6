"""Monotone PPM for the shallow-water tracers, the PyTorch twin on the CPU
(``ShallowWaterTracers(..., tracer_limiter="ppm")``): the mixing ratios are
reconstructed by PPM whose interface values are confined between their two
cells, (h, v) keep the configured PLR limiter on the same three-layer window.

Bounds: bit identity where the scheme promises it; for the rest the figures
measured when the scheme was prototyped (constancy 8.9e-16, mass drift 1.9e-15,
cap inside [0, 1] exactly) with the margins of ``test_tracers.py``; the
accuracy ratio (0.55 at C24, unweighted) must stay below 0.7."""
import functools
import math
import os
from unittest import mock

import numpy as np
import pytest
import torch
import yaml

import stsphere as S
from stsphere.engine import Engine, VirtualCluster
from stsphere.models import base
from stsphere.models import swe as swe_mod
from stsphere.models.base import PPM, _inner_face, extend, ppm_faces, reconstruct
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater, ShallowWaterTracers
from stsphere.parallel.layout import TileLayout
from stsphere.utils import checkpoint as ckpt
from stsphere.utils.history import read_history

from rough_states import global_of, install
from tracer_states import rough_mixing_ratios

DAY = 86400.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ppm_parent_rough_q.npz")


@functools.lru_cache(maxsize=None)
def _grid(N):
    return CubedSphereGrid(N)


def _engine(phys, N, t, ng=3, **kw):
    return Engine(phys, TileLayout(N, t, 1, ng=ng), grid=_grid(N), dtype=torch.float64, device="cpu", backend="torch",
                  **kw)


def _ppm(case, tracers, lim=2):
    return ShallowWaterTracers(case, tracers=tracers, limiter=lim, tracer_limiter="ppm")


def test_halo_and_kernel_params():
    p = _ppm("tc5", ["cap"], 1)
    assert p.halo == 3 and p.kernel_params()["tracer_limiter"] == 4 and p.kernel_params()["limiter"] == 1
    q = ShallowWaterTracers("tc5", tracers=["cap"], limiter=1)
    assert q.halo == 2 and q.kernel_params()["tracer_limiter"] == 0
    assert ShallowWaterTracers("tc5", tracers=["cap"], tracer_limiter=4).tracer_limiter == PPM
    with pytest.raises(ValueError, match="tracer_limiter"):
        ShallowWaterTracers("tc5", tracers=["cap"], tracer_limiter="mc")
    with pytest.raises(ValueError, match="PPM"):       # PPM for (h, v) stays refused, with PPM tracers too
        ShallowWaterTracers("tc5", tracers=["cap"], limiter=4, tracer_limiter="ppm")
    with pytest.raises(ValueError, match="halo 3"):
        _engine(p, 12, 1, ng=2)


@pytest.mark.parametrize("lim", [0, 1, 2, 3])
@pytest.mark.parametrize("t", [1, 2])
def test_swe_rows_untouched_and_constants_stay_constant(t, lim):
    """TC5 C12, 10 steps: (h, M) on the three-layer window are bit-identical to
    a plain ShallowWater run on an ng = 2 layout; q = 0.75 and q = 1 stay
    constant."""
    a = _engine(_ppm("tc5", [0.75, "constant"], lim), 12, t)
    b = _engine(ShallowWater("tc5", limiter=lim), 12, t, ng=2, dt=a.dt)
    a.step(10)
    b.step(10)
    va = a.tiles_view()
    assert torch.equal(va[:4], b.tiles_view())
    for k, c in enumerate((0.75, 1.0)):
        dev = (va[4 + k] / va[0] - c).abs().max().item()
        print(f"t={t} lim={lim} q={c}: max deviation {dev:.2e}")
        assert dev < 1e-13


def _cap_run(phys, N):
    e = _engine(phys, N, 1)
    A = e.tens["area"]
    m0 = (e.tiles_view()[4] * A).sum().item()
    e.step(40)
    v = e.tiles_view()
    q = v[4] / v[0]
    return q.min().item(), q.max().item(), abs((v[4] * A).sum().item() - m0) / abs(m0)


@pytest.mark.parametrize("lim", [1, 2, 3])
@pytest.mark.parametrize("case,N", [("tc5", 12), ("tc6", 16)])
def test_cap_bounds_and_mass(case, N, lim):
    """A 0/1 cap, 40 steps: the monotone PPM keeps q in [0, 1] and the tracer
    mass drifts by rounding; the same run on the unclamped ``ppm_faces`` leaves
    [0, 1] by more than 0.01 (the fourth-order interface value is not confined
    between its cells), so the test can fail."""
    lo, hi, drift = _cap_run(_ppm(case, ["cap"], lim), N)
    print(f"{case} C{N} lim={lim} monotone PPM: q min {lo:.3e} max - 1 {hi - 1:.3e}; relative mass drift {drift:.2e}")
    assert -1e-12 <= lo and hi <= 1.0 + 1e-12
    assert drift < 1e-13

    def unclamped(*a, **k):
        k.pop("monotone", None)
        return reconstruct(*a, **k)
    with mock.patch.object(swe_mod, "reconstruct", unclamped):
        ulo, uhi, udrift = _cap_run(_ppm(case, ["cap"], lim), N)
    print(f"{case} C{N} lim={lim} unclamped PPM: q min {ulo:.3e} max - 1 {uhi - 1:.3e}; drift {udrift:.2e}")
    assert max(-ulo, uhi - 1.0) > 0.01
    assert udrift < 1e-13


def test_decomposition_independent():
    """t = 1, t = 2 and 4 virtual ranks after 20 steps: bit-identical."""
    N = 12
    mk = lambda: _ppm("tc5", ["cap", "gradient"])   # noqa: E731
    a = _engine(mk(), N, 1)
    b = _engine(mk(), N, 2, dt=a.dt)
    vc = VirtualCluster(mk, TileLayout(N, 2, 4, ng=3), grid=_grid(N), dtype=torch.float64, device="cpu",
                        backend="torch", dt=a.dt)
    for x in (a, b, vc):
        x.step(20)
    ga = global_of(a)
    assert torch.equal(ga, global_of(b))
    assert torch.equal(ga, global_of(vc.engines))


def _cfg(out, tracers=("cosine_bell",), tracer_limiter="ppm", case="tc2", N=12, nd=1, t=1, time=None, **io):
    c = {"parallelization": {"tiles_per_edge": t, "num_devices": nd, "device_type": "cpu"},
         "grid": {"N": N}, "physics": {"model": "swe", "case": case, "limiter": "mc"},
         "time": time or {"nsteps": 6, "dt": 400.0}, "io": dict({"output_dir": str(out)}, **io)}
    if tracers is not None:
        c["physics"]["tracers"] = list(tracers)
    if tracer_limiter is not None:
        c["physics"]["tracer_limiter"] = tracer_limiter
    return c


def test_accuracy_cosine_bell_on_tc2(tmp_path):
    """A cosine bell carried three days by the TC2 flow at C24: the l2 error of
    ``Solver.tracer_error_norms`` with PPM tracers is below 0.7 of the MC
    tracers' (prototype: 0.55 unweighted)."""
    norms = {}
    for tl in (None, "ppm"):
        s = S.Solver(_cfg(tmp_path / str(tl), tracer_limiter=tl, N=24, time={"days": 3.0}), verbose=False)
        s.initialize()
        assert s.layout.ng == (3 if tl else 2)
        s.step(int(math.ceil(3.0 * DAY / s.dt)))
        norms[tl] = s.tracer_error_norms(0)
        q = s.tracer(0)
        print(f"C24 TC2 cosine bell, 3 days, {s.step_count} steps, tracer_limiter={tl}: "
              f"l1 {norms[tl]['l1']:.4e} l2 {norms[tl]['l2']:.4e} linf {norms[tl]['linf']:.4e} "
              f"peak {q.max():.4f} min {q.min():.3e}")
        assert s.error_norms() is not None       # TC2: the depth has a closed form too
    ratio = norms["ppm"]["l2"] / norms[None]["l2"]
    print(f"l2 ratio PPM / MC: {ratio:.3f}")
    assert ratio < 0.7


def test_option_off_is_the_parent_bit_for_bit():
    """``ppm_faces``, ``_inner_face`` and ``reconstruct`` with ``monotone`` off
    against the outputs of the code before the option existed
    (tests/golden/ppm_parent_rough_q.npz, on ``rough_mixing_ratios(2, 16)``;
    the panel-edge tables come from the fixture too); with it on they differ."""
    z = {k: torch.as_tensor(v) for k, v in np.load(GOLDEN).items()}
    q = rough_mixing_ratios(2, 16)
    g, n = 3, 10
    aL, aR = ppm_faces(q, g, n)
    assert torch.equal(aL, z["faces_aL"]) and torch.equal(aR, z["faces_aR"])
    lo = torch.tensor([True, False, True, False, True, True])[:, None, None]
    hi = torch.tensor([False, True, True, False, False, True])[:, None, None]
    aL, aR = ppm_faces(q, g, n, lo, hi)
    assert torch.equal(aL, z["faces_edge_aL"]) and torch.equal(aR, z["faces_edge_aR"])
    lines = q.unfold(-1, 6, 1)
    assert torch.equal(_inner_face(lines, PPM), z["inner_ppm"]) and torch.equal(_inner_face(lines, 2), z["inner_mc"])
    assert torch.equal(_inner_face(lines, 2, monotone=True), z["inner_mc"])          # PPM only
    N = 16
    e = _engine(ShallowWater("tc5", limiter=4), N, 1)
    install(e, torch.cat([q, 1.0 - q]))
    w = extend(e.pool[0], None, e.gmap, e.plan.T, e.plan.n, 3, cmap=e.cmap)[:2]
    tens = {k: z[k] for k in ("pedge", "pe_base", "pe_t")}
    (xL, xR, _, _), (yL, yR, _, _) = reconstruct(w, tens, 3, N, PPM)
    for name, x in (("rec_xL", xL), ("rec_xR", xR), ("rec_yL", yL), ("rec_yR", yR)):
        assert torch.equal(x, z[name]), name
    (xL, _, _, _), (_, yR, _, _) = reconstruct(w, {}, 3, N, PPM)
    assert torch.equal(xL, z["plain_xL"]) and torch.equal(yR, z["plain_yR"])
    # on: the clamp acts on these data (17-19 % of the interfaces), also at the panel edges
    assert not torch.equal(ppm_faces(q, g, n, monotone=True)[0], z["faces_aL"])
    assert not torch.equal(_inner_face(lines, PPM, monotone=True), z["inner_ppm"])
    (mL, mR, _, _), _ = reconstruct(w, tens, 3, N, PPM, monotone=True)
    assert not torch.equal(mL[..., 0], z["rec_xL"][..., 0]) and not torch.equal(mR, z["rec_xR"])
    x = torch.tensor([0.3, -1.0, 2.0])
    assert base.clamp_between(x, torch.tensor(1.0), torch.tensor(0.0)).tolist() == pytest.approx([0.3, 0.0, 1.0])


def test_config_to_solver_history_restart(tmp_path):
    p = tmp_path / "c.yaml"
    cfg = _cfg(tmp_path / "run", tracers=["cosine_bell", "cap"], history_interval=3, checkpoint_interval=3,
               history_fields=["h", "q0", "q1"])
    p.write_text(yaml.safe_dump(cfg))
    s = S.Solver(str(p), verbose=False)
    summary = s.run()
    assert isinstance(s.physics, ShallowWaterTracers) and s.physics.tracer_limiter == PPM
    assert s.layout.ng == 3 and s.cfg.grid.halo == 2 and s.step_count == 6
    for k in ("l1", "l2", "linf"):
        assert np.isfinite(summary[f"tracer0_err_{k}"]) and f"tracer1_err_{k}" not in summary
        assert np.isfinite(summary[f"err_{k}"])
    assert summary["tracer0_err_l2"] == s.tracer_error_norms()["l2"] and s.tracer_error_norms(1) is None
    g = s.gather_global()
    hist = str(tmp_path / "run" / "history.zarr")
    assert np.array_equal(read_history(hist, "q0")[-1], s.tracer(0))
    assert np.array_equal(read_history(hist, "q1")[-1], g[5] / g[0])
    # restart from step 3 on another tiling: the same trajectory
    root = str(tmp_path / "run" / "checkpoints")
    assert ckpt.list_checkpoints(root) == [3, 6]
    c2 = _cfg(tmp_path / "run", tracers=["cosine_bell", "cap"], nd=2, t=2, restore=ckpt.step_dir(root, 3))
    s2 = S.Solver(c2, verbose=False)
    s2.initialize()
    assert s2.step_count == 3 and s2.layout.ng == 3
    s2.step(3)
    assert np.array_equal(s2.gather_global(), g)


def test_config_errors_and_exact(tmp_path):
    with pytest.raises(ValueError, match="tracer_limiter"):
        S.Solver(_cfg(tmp_path, tracers=None), verbose=False).initialize()
    with pytest.raises(ValueError, match="tracer_limiter"):
        S.Solver(_cfg(tmp_path, tracers=[]), verbose=False).initialize()
    for bad in ("mc", "none", 4):
        with pytest.raises(ValueError, match="tracer_limiter"):
            S.Solver(_cfg(tmp_path, tracer_limiter=bad), verbose=False).initialize()
    c = _cfg(tmp_path)
    c["physics"]["limiter"] = "ppm"
    with pytest.raises(ValueError, match="PPM"):
        S.Solver(c, verbose=False).initialize()
    assert _ppm("tc5", ["cosine_bell"]).tracer_exact(_grid(12), 0.0, 0) is None
    p = _ppm("tc2", ["cap", "cosine_bell"])
    assert p.tracer_exact(_grid(12), 0.0, 0) is None
    assert np.allclose(p.tracer_exact(_grid(12), 0.0, 1), p.tracer_fields(_grid(12))[1], rtol=0, atol=1e-14)
    s = S.Solver(_cfg(tmp_path, case="tc5"), verbose=False)
    s.initialize()
    assert s.tracer_error_norms() is None
    plain = S.Solver(_cfg(tmp_path, tracers=None, tracer_limiter=None), verbose=False)
    plain.initialize()
    assert plain.tracer_error_norms() is None


def test_shipped_config():
    with open(os.path.join(S.__path__[0], "configs", "c48_tracers_ppm_1gpu.yaml")) as f:
        c = yaml.safe_load(f)
    ph = c["physics"]
    assert (ph["case"], ph["tracers"], ph["limiter"], ph["tracer_limiter"]) == ("tc2", ["cosine_bell", "cap"], "mc", "ppm")


def test_block_rule_and_lds_bytes():
    """The LDS rule: 16 x 16 fp64 with four PPM tracers is 70 016 bytes and is
    not chosen; what fits is chosen as before."""
    from stsphere.ops.hip_compute import TRACER_LDS_MAX, choose_tracer_block, tracer_lds_bytes
    assert tracer_lds_bytes(16, 16, 4, 8, 0) == 63824 and tracer_lds_bytes(16, 16, 4, 8, 4) == 70016
    assert tracer_lds_bytes(16, 8, 4, 8, 4) == 43904 and tracer_lds_bytes(16, 16, 3, 8, 4) == 65456
    assert TRACER_LDS_MAX == 65536
    # 6 tiles of 48^2: 54 blocks of 16 x 16, 108 of 16 x 8; 100 CUs -> 16 x 16 where it fits
    assert choose_tracer_block(48, 6, 100) == (16, 16)
    assert choose_tracer_block(48, 6, 100, 4, 8, 0) == (16, 16)
    assert choose_tracer_block(48, 6, 100, 3, 8, 4) == (16, 16)
    assert choose_tracer_block(48, 6, 100, 4, 8, 4) == (16, 8)
    assert choose_tracer_block(48, 6, 100, 4, 4, 4) == (16, 16)
    assert choose_tracer_block(48, 6, 256, 2, 8, 4) == (16, 8)
