"""The plumbing the output products share: the cell maps of a rank, name
resolution per model, the staging helper of the run loop and the descriptor
table of the native binding."""
import ctypes
import os

import numpy as np
import pytest
import torch

from stsphere.driver import Solver, stage
from stsphere.models import latlon as ml
from stsphere.models import points as mp
from stsphere.parallel.layout import TileLayout


# ---- cell maps -----------------------------------------------------------------------

@pytest.mark.parametrize("nd", [1, 3, 24])
def test_cell_maps_match_a_per_cell_loop(nd):
    L = TileLayout(8, 2, nd, ng=2)
    n, P, g = L.n, L.n + 4, 2
    for rank in range(nd):
        pad, unp = L.cell_maps(rank)
        rp, ru = np.full(6 * 64, -1, np.int32), np.full(6 * 64, -1, np.int32)
        for c in range(6 * 64):
            tid, i, j = (int(v) for v in L.locate(np.int64(c)))
            if L.owner[tid] != rank:
                continue
            li = L.rank_tiles[rank].index(tid)
            rp[c] = (li * P + j + g) * P + i + g
            ru[c] = (li * n + j) * n + i
        assert pad.dtype == unp.dtype == np.int32
        assert np.array_equal(pad, rp) and np.array_equal(unp, ru), rank
        again = mp.rank_maps(L, rank)
        assert np.array_equal(again[0], pad) and np.array_equal(again[1], unp)


@pytest.mark.parametrize("nd", [1, 3])
def test_latlon_rank_index_is_the_map_of_its_sources(nd):
    L = TileLayout(8, 2, nd, ng=2)
    tab = ml.tables_for(8, *ml.default_grid(8, 16))
    for rank in range(nd):
        pad, unp = L.cell_maps(rank)
        ip, iu = tab.rank_index(L, rank)
        assert ip.shape == iu.shape == (8 * 16, 4) and ip.dtype == iu.dtype == np.int32
        assert np.array_equal(ip, pad[tab.src]) and np.array_equal(iu, unp[tab.src])


# ---- name resolution -------------------------------------------------------------------

def _solver(model, case):
    s = Solver({"parallelization": {"tiles_per_edge": 1, "num_devices": 1, "device_type": "cpu"},
                "grid": {"N": 8}, "physics": {"model": model, "case": case}}, verbose=False)
    s.initialize()
    return s


def test_names_of_the_shallow_water_model():
    s = _solver("swe", "tc5")
    names = ["h", "vorticity", "u", "mz", "pv", "v", "divergence"]
    want = [("prog", 0), ("der", 0), ("wind", 0), ("prog", 3), ("der", 2), ("wind", 1), ("der", 1)]
    assert s._resolve_names(names, "lat-lon") == want and s._resolve_names(names, "sample") == want
    assert s._resolve_names(["pv", "h"], "spectrum", winds=False) == [("der", 2), ("prog", 0)]
    with pytest.raises(ValueError) as e:
        s._resolve_names(["h", "nope"], "lat-lon")
    assert str(e.value) == f"unknown lat-lon field 'nope'; choose from {s.latlon_names()}"
    with pytest.raises(ValueError) as e:
        s._resolve_names(["nope"], "sample")
    assert str(e.value) == f"unknown sample field 'nope'; choose from {s.latlon_names()}"
    with pytest.raises(ValueError) as e:
        s._resolve_names(["nope"], "spectrum", winds=False)
    assert str(e.value) == f"unknown spectrum field 'nope'; choose from {s.spectrum_names()}"
    assert "u" in s.latlon_names() and "u" not in s.spectrum_names()


def test_names_of_the_advection_model():
    s = _solver("advection", None)
    f = s.fields[0]
    for what in ("lat-lon", "sample"):
        assert s._resolve_names([f], what) == [("prog", 0)]
        with pytest.raises(ValueError) as e:
            s._resolve_names([f, "vorticity"], what)
        assert str(e.value) == "derived fields are defined for the shallow-water model, not 'advection'"
        with pytest.raises(ValueError) as e:
            s._resolve_names(["u"], what)
        assert str(e.value) == "winds are defined for the shallow-water model, not 'advection'"
    assert s._resolve_names([f], "spectrum", winds=False) == [("prog", 0)]
    with pytest.raises(ValueError) as e:
        s._resolve_names(["pv"], "spectrum", winds=False)
    assert str(e.value) == "derived fields are defined for the shallow-water model, not 'advection'"
    # the public methods raise the same text
    with pytest.raises(ValueError, match="winds are defined for the shallow-water model, not 'advection'"):
        s.latlon_field("v", 8, 16)
    with pytest.raises(ValueError, match="derived fields are defined for the shallow-water model"):
        s.sample(["pv"], [0.1], [0.2])


@pytest.mark.parametrize("model,case", [("swe", "tc5"), ("advection", None)])
def test_a_wind_has_no_spectrum(model, case):
    s = _solver(model, case)
    msg = ("'u' is a vector component, not a scalar on the sphere: it has no spherical-harmonic spectrum; "
           "use ke_spectrum for the winds")
    with pytest.raises(ValueError) as e:
        s._resolve_names([s.fields[0], "u"], "spectrum", winds=False)
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        s.spectrum("u", 4)
    assert str(e.value) == msg


# ---- staging helper ----------------------------------------------------------------------

def test_stage_of_a_cpu_tensor_copies_without_an_event():
    v = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    ev, h = stage(v, False)
    assert ev is None and torch.equal(h, v) and h.dtype == v.dtype
    assert h.data_ptr() != v.data_ptr()
    h[0, 0] = -1.0
    assert v[0, 0] == 0.0
    # a CPU tensor never takes the pinned path, and a list shares one (absent) event
    ev, hs = stage([v, v[0]], True)
    assert ev is None and len(hs) == 2 and torch.equal(hs[0], v) and torch.equal(hs[1], v[0])
    assert hs[0].data_ptr() != v.data_ptr() and hs[1].data_ptr() != v.data_ptr()


# ---- descriptor table --------------------------------------------------------------------

def test_descriptor_mirrors_match_the_library():
    """Every descriptor of the table: the library as built exports its launch
    symbol and reports the size of the ctypes mirror.  The library is opened
    here, not through ``native.load`` (which makes the same comparison and
    raises): a stale mirror or a missing symbol fails this test."""
    from stsphere.ops import native
    if not os.path.exists(native.lib_path()):
        pytest.skip("library not built")
    lib = ctypes.CDLL(native.lib_path(), mode=ctypes.RTLD_GLOBAL)
    names = [cls.__name__ for _, _, cls, _ in native.DESCRIPTORS]
    assert sorted(names) == sorted(["StageDesc", "FusedDesc", "March3Desc", "DerivedDesc", "LatLonDesc",
                                    "PointsDesc", "SpectraDesc", "SynthDesc"])
    for launch, argtypes, cls, (query, args) in native.DESCRIPTORS:
        assert hasattr(lib, launch), launch
        assert argtypes.count(ctypes.POINTER(cls)) == 1 and argtypes[-1] is ctypes.c_void_p, launch
        size = getattr(lib, query)
        size.argtypes, size.restype = [ctypes.c_int] * len(args), ctypes.c_int
        assert size(*args) == ctypes.sizeof(cls), cls.__name__
