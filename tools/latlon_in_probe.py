#!/usr/bin/env python
"""Event-time the lat-lon input (ops/latlon_in.py::LatLonIn, the preparation and
the ingest launch of ops/csrc/latlon_in_kernel.hip) on one GPU for a 721 x 1440
source with h, u, v: every (order, quadrature) interleaved in each repetition,
each launch timed with its own pair of device events.  One JSON line per size and
setting with the medians, the difference against the twin (models/latlon_in.py)
evaluated for the same GPU tensors, and one streaming pass (a copy) over the state.

    python tools/latlon_in_probe.py                      # C96 and C720
    python tools/latlon_in_probe.py --sizes 96 --dtype fp32 --no-twin
"""
import argparse
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def event_us(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96,720", help="comma list of N (cells per panel edge)")
    ap.add_argument("--source", default="721x1440")
    ap.add_argument("--dtype", default="fp64", choices=["fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--no-twin", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    from stsphere.engine import Engine
    from stsphere.models import latlon_in as ml
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("latlon_in_probe needs a GPU")
    dtype = torch.float64 if a.dtype == "fp64" else torch.float32
    nlat, nlon = (int(v) for v in a.source.split("x"))
    lat = np.linspace(-0.5 * math.pi, 0.5 * math.pi, nlat)
    lon = np.arange(nlon) * (2.0 * math.pi / nlon)
    la, lo = np.meshgrid(lat, lon, indexing="ij")
    host = {"h": 3000.0 - 500.0 * np.sin(la) ** 2 + 50.0 * np.cos(la) * np.sin(3 * lo),
            "u": 30.0 * np.cos(la) + 5.0 * np.sin(la) * np.cos(lo), "v": -5.0 * np.sin(lo)}
    arrays = {k: torch.as_tensor(v, device="cuda") for k, v in host.items()}
    settings = [(o, q) for o in ml.ORDERS for q in ml.QUADRATURES]
    for N in (int(v) for v in a.sizes.split(",")):
        e = Engine(ShallowWater("tc2"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), dtype=dtype, device="cuda",
                   backend="hip")
        op = e.latlon_in(lat, lon)
        buf = torch.empty_like(e.state)
        ts = {s: ([], []) for s in settings}
        copy = []
        for r in range(a.warm + a.reps):
            for o, q in settings:
                t1 = event_us(lambda: op.ingest(arrays, o, q, phases=1))
                t2 = event_us(lambda: op.ingest(arrays, o, q, phases=2))
                if r >= a.warm:
                    ts[(o, q)][0].append(t1)
                    ts[(o, q)][1].append(t2)
            if r >= a.warm:
                copy.append(event_us(lambda: buf.copy_(e.state)))
        g, plan = op.grid, ml.channel_plan(e.physics, list(arrays))
        work = None if a.no_twin else ml.prepare(g, plan, host)
        for o, q in settings:
            rec = {"N": N, "dtype": a.dtype, "nlat": nlat, "nlon": nlon, "order": o, "quadrature": q, "reps": a.reps,
                   "prepare_us_median": statistics.median(ts[(o, q)][0]),
                   "ingest_us_median": statistics.median(ts[(o, q)][1]), "ingest_us_min": min(ts[(o, q)][1]),
                   "state_copy_us_median": statistics.median(copy), "state_bytes": e.state.numel() * e.state.element_size()}
            if work is not None and (N <= 96 or q == 1):          # the twin of C720 with q > 1 takes minutes on the host
                op.ingest(arrays, o, q)
                ref = ml.ingest_tiles(g, plan, work, e.layout, 0, o, q)
                got = e.tiles_view().double().cpu().numpy()
                rec["max_diff_vs_twin"] = max(float(np.abs(got[f] - ref[f]).max() / np.abs(ref[f]).max()) for f in ref)
            print(json.dumps(rec), flush=True)
        del e, op, buf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
