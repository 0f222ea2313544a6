#!/usr/bin/env python
"""Event-time the lat-lon regridding (ops/latlon.py::LatLon, the gather and
finish launches of ops/csrc/latlon_kernel.hip) on one GPU, and the same
quantities computed by the PyTorch twin (models/latlon.py) on the same GPU
tensors.  Warm repetitions, each timed with its own pair of device events; one
JSON line per size and product (the four prognostic fields with their zonal
means; u, v with theirs) with the median, the fastest repetition, the bytes the
launches must move at least (tables once, every distinct source value once,
the outputs written and read back by the finish launch) and the rate that
makes.

    python tools/latlon_probe.py                        # C96 t=2 -> 181x360, C720 t=2 -> 721x1440
    python tools/latlon_probe.py --sizes 96x2:181x360 --dtype fp32
"""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, reps, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x2:181x360,720x2:721x1440",
                    help="comma list of NxT:NLATxNLON (cells per panel edge x tiles per edge : target grid)")
    ap.add_argument("--dtype", default="fp64", choices=["fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--no-twin", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from stsphere.engine import Engine
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("latlon_probe needs a GPU")
    dtype = torch.float64 if a.dtype == "fp64" else torch.float32
    esize = 8 if a.dtype == "fp64" else 4
    for size in a.sizes.split(","):
        src, dst = size.split(":")
        N, t = (int(v) for v in src.split("x"))
        nlat, nlon = (int(v) for v in dst.split("x"))
        # node-centred target: both pole rows and the column lon = 0
        lat = np.linspace(-0.5 * math.pi, 0.5 * math.pi, nlat)
        lon = np.arange(nlon) * (2.0 * math.pi / nlon)
        grid = CubedSphereGrid(N)
        L = TileLayout(N, t, 1, ng=2)
        hip = Engine(ShallowWater("tc5"), L, grid=grid, dtype=dtype, device="cuda", backend="hip")
        ll = hip.latlon(lat, lon)
        ref = None
        if not a.no_twin:
            ref = Engine(ShallowWater("tc5"), L, grid=grid, dtype=dtype, device="cuda", backend="torch", dt=hip.dt)
            lt = ref.latlon(lat, lon)
        K, cells = ll.K, 6 * N * N
        for product, C, Cout, fn, tw in (("fields", 4, 4, ll.fields, ref and lt.fields),
                                         ("winds", 3, 2, ll.winds, ref and lt.winds)):
            k = timed(fn, a.reps, a.warm)
            nsrc = C + (1 if product == "winds" else 0)
            # tables, distinct source values (at most four per point and channel), the
            # partial written and read back, the winds' vectors and output
            nbytes = K * 48 + nsrc * min(cells, 4 * K) * esize + 2 * C * K * esize
            if product == "winds":
                nbytes += K * 48 + Cout * K * esize
            rec = {"N": N, "tiles_per_edge": t, "dtype": a.dtype, "nlat": nlat, "nlon": nlon, "points": K,
                   "product": product, "reps": a.reps, "kernel_us_median": statistics.median(k),
                   "kernel_us_min": min(k), "min_bytes": nbytes,
                   "bytes_per_s": nbytes / (statistics.median(k) * 1e-6)}
            if ref is not None:
                w = timed(tw, a.reps, a.warm)
                rec.update(twin_us_median=statistics.median(w), twin_us_min=min(w),
                           twin_over_kernel=statistics.median(w) / statistics.median(k))
                (f0, z0), (f1, z1) = fn(), tw()
                scale = f1.abs().amax((1, 2)).clamp_min(1e-300)      # a channel that is 0 (mz of TC5 at t = 0)
                rec["max_diff_vs_twin"] = float(((f0 - f1).abs().amax((1, 2)) / scale).max())
                rec["max_zonal_diff_vs_twin"] = float(((z0 - z1).abs().amax(1) / scale).max())
            print(json.dumps(rec), flush=True)
        del hip, ll, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
