"""The lat-lon input kernel (ops/csrc/latlon_in_kernel.hip) through
``Solver.set_from_latlon`` / ``Ensemble.set_from_latlon`` against the twin
(models/latlon_in.py) on the same inputs.

fp64 metric: per state field, max |kernel - twin| over the cells relative to the
field's source scale (max |h|; max |h| max |(u, v)|; max |h| max |q_k|).  Bound:
8 x the same metric between the twin in ``numpy.longdouble`` and in float64 on the
CPU over these cases (kernel and twin differ in the last bits of tan / asin / atan2
/ sincos, and the interpolant's sensitivity to position scales with nlon; measured
1.51e-15, profiles/latlon_in/README.md); 8 covers one more rounding per tap in
another association and stays orders of magnitude below any indexing error.
fp32 state: the twin's float64 result rounded to float32, within one float32 ulp of
max |field|."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from stsphere.driver import Solver, make_physics
from stsphere.ensemble import Ensemble
from stsphere.engine import Engine
from stsphere.models import latlon_in as ml
from stsphere.models.swe import ShallowWater
from stsphere.parallel.layout import TileLayout
from stsphere.utils.config import load_config
from test_latlon_in import source, tc2

pytestmark = pytest.mark.gpu

LONGDOUBLE_DISCREPANCY = 1.51e-15     # twin in longdouble against float64, largest over the cases (CPU)
TOL64 = 8.0 * LONGDOUBLE_DISCREPANCY
GRIDS = {"poles": (13, 24, True), "centred": (12, 24, False)}


@functools.lru_cache(maxsize=None)
def inputs(kind, phys):
    """(lat, lon, arrays, per-field scales) of a case's source."""
    lat, lon = source(*GRIDS[kind])
    h, u, v = tc2(lat, lon)
    if phys == "adv":
        return lat, lon, {"q": h}, [np.abs(h).max()]
    q0, q1 = np.cos(lat)[:, None] * np.sin(lon)[None, :], h / 3000.0
    hm, wm = np.abs(h).max(), np.sqrt(u * u + v * v).max()
    return lat, lon, dict(h=h, u=u, v=v, q0=q0, q1=q1), [hm] + [hm * wm] * 3 + [hm * np.abs(q0).max(), hm * np.abs(q1).max()]


def config(N, t, dtype, phys, device="gpu"):
    physics = {"model": "advection"} if phys == "adv" else {"model": "swe", "case": "tc2", "tracers": ["constant"] * 2}
    return {"parallelization": {"num_devices": 6 if t > 1 else 1, "tiles_per_edge": t, "device_type": device},
            "grid": {"N": N, "dtype": dtype}, "physics": physics}


@functools.lru_cache(maxsize=None)
def solver(N, t, dtype, phys):
    s = Solver(config(N, t, dtype, phys), verbose=False)
    s.initialize()
    return s


@functools.lru_cache(maxsize=None)
def twin(N, kind, order, q, phys, ft=np.float64):
    """[F, 6, N, N] of the twin in ``ft``."""
    lat, lon, arrays, _ = inputs(kind, phys)
    g = ml.source_grid(lat, lon)
    plan = ml.channel_plan(make_physics(load_config(config(N, 1, "float64", phys)).physics), list(arrays))
    out = ml.ingest_tiles(g, plan, ml.prepare(g, plan, arrays, ft), TileLayout(N, 1, 1), 0, order, q)
    return np.stack([out[f] for f in sorted(out)])


def metric(a, b, scales):
    return max(float(np.abs(a[f] - b[f]).max() / s) for f, s in enumerate(scales))


@pytest.mark.parametrize("phys", ["swe", "adv"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("q", ml.QUADRATURES)
@pytest.mark.parametrize("order", ml.ORDERS)
@pytest.mark.parametrize("kind", list(GRIDS))
@pytest.mark.parametrize("N,t", [(5, 1), (17, 1), (12, 2)])
def test_kernel_against_twin(N, t, kind, order, q, dtype, phys):
    lat, lon, arrays, scales = inputs(kind, phys)
    s = solver(N, t, dtype, phys)
    s.set_from_latlon(lat, lon, order=order, quadrature=q, **arrays)
    got, ref = s.gather_global(), twin(N, kind, order, q, phys)
    for e in s.engines:                              # the same-rank ghost slots hold their sources
        assert torch.equal(e.state[:, e.halo_dst], e.state[:, e.halo_src])
    if dtype == "float64":
        err = metric(got, ref, scales)
        print(f"fp64 metric {err:.3e} (bound {TOL64:.1e})")
        assert err <= TOL64
    else:
        r32 = ref.astype(np.float32)
        for f in range(len(ref)):
            assert np.abs(got[f] - r32[f].astype(np.float64)).max() <= np.spacing(np.abs(r32[f]).max())


def test_reproducible_and_partition_independent():
    lat, lon, arrays, _ = inputs("poles", "swe")
    out = []
    for t in (1, 1, 2):
        s = Solver(config(12, t, "float64", "swe"), verbose=False)
        s.initialize()
        s.set_from_latlon(lat, lon, order=3, quadrature=4, **arrays)
        out.append(s.gather_global())
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def test_in_place_on_a_batched_ensemble():
    lat, lon, arrays, _ = inputs("centred", "swe")
    arrays = {k: arrays[k] for k in ("h", "u", "v")}
    lay = TileLayout(8, 1, 1, ng=2)
    ens = Ensemble(lambda: ShallowWater("tc2"), lay, 3, amplitude=1e-2, device="cuda", backend="hip", mode="batched",
                   steps_per_graph=2)
    ens.run(2)                                       # captures the graph
    before = ens.states().clone()
    ptr = ens.batch[0].data_ptr()
    ens.set_from_latlon(lat, lon, members=[1], **arrays)
    solo = Solver(dict(config(8, 1, "float64", "swe"), physics={"model": "swe", "case": "tc2"}), verbose=False)
    solo.initialize()
    solo.set_from_latlon(lat, lon, **arrays)
    start = ens.states().clone()
    assert ens.batch[0].data_ptr() == ptr and torch.equal(start[1], solo.engines[0].tiles_view())
    assert torch.equal(start[0], before[0]) and torch.equal(start[2], before[2])
    ens.run(2)                                       # a replay of the captured graph
    assert ens._graph is not None and ens._graph.graph_steps == 4
    torch.cuda.synchronize()
    for m in range(3):
        e = Engine(ShallowWater("tc2"), lay, device="cuda", backend="hip", dt=ens.dt, block=ens.block)
        e.set_state(start[m])
        e.step(2)
        assert torch.equal(e.tiles_view(), ens.engines[m].tiles_view())


def test_launcher_validation():
    from stsphere.ops import native
    lat, lon, arrays, _ = inputs("poles", "swe")
    s = solver(5, 1, "float64", "swe")
    s.set_from_latlon(lat, lon, **arrays)            # fills the descriptor
    op = s.engines[0].latlon_in(lat, lon)
    assert op.lib.stsp_latlon_in_desc_size() == ctypes.sizeof(native.LatLonInDesc)
    for field, value, code in (("work", None, 1), ("phases", 4, 1), ("pw", 3, 1), ("nlat", 3, 4), ("nlon", 23, 4),
                               ("dlon", 0.0, 4), ("lon0", 7.0, 4), ("C", 5, 5), ("nq", 5, 5), ("order", 2, 6),
                               ("quad", 3, 6)):
        d = native.LatLonInDesc.from_buffer_copy(op.desc)
        setattr(d, field, value)
        assert op.lib.stsp_latlon_in_launch(1, d, None) == code, field
    assert op.lib.stsp_latlon_in_launch(7, native.LatLonInDesc.from_buffer_copy(op.desc), None) == 2
