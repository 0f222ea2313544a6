#!/usr/bin/env python
"""Event-time the derived-field kernel (ops/derived.py::DerivedFields.compute,
two launches of ops/csrc/derived_kernel.hip) on one GPU, and the same
quantities computed by the PyTorch twin (models/derived.py) on the GPU
tensors, the only other way to get them.  Warm repetitions, each timed with
its own pair of device events; one JSON line per size with the median, the
fastest repetition and the time to stream the state once (4 fields read, 3
written) at the measured copy rate of the device.

    python tools/derived_probe.py                     # C96 t=2 fp64 and C720 t=2 fp64
    python tools/derived_probe.py --sizes 96x2 --dtype fp32
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STREAM_RATE = 2.1e12      # B/s, the documented copy rate (docs/ARCHITECTURE.md)


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
    ap.add_argument("--sizes", default="96x2,720x2", help="comma list of NxT (cells per panel edge x tiles per edge)")
    ap.add_argument("--dtype", default="fp64", choices=["fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--no-twin", action="store_true")
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("derived_probe needs a GPU")
    dtype = torch.float64 if a.dtype == "fp64" else torch.float32
    esize = 8 if a.dtype == "fp64" else 4
    for size in a.sizes.split(","):
        N, t = (int(v) for v in size.split("x"))
        grid = CubedSphereGrid(N)
        L = TileLayout(N, t, 1, ng=2)
        hip = Engine(ShallowWater("tc5"), L, grid=grid, dtype=dtype, device="cuda", backend="hip")
        d = hip.derived_fields
        k = timed(d.compute, a.reps, a.warm)
        cells = 6 * N * N
        rec = {"N": N, "tiles_per_edge": t, "dtype": a.dtype, "cells": cells, "blocks": d.nblocks, "reps": a.reps,
               "kernel_us_median": statistics.median(k), "kernel_us_min": min(k),
               "stream_once_us": 7 * esize * cells / STREAM_RATE * 1e6,
               "table_bytes_per_cell": 13 * esize, "state_bytes_per_cell": 7 * esize}
        rec["kernel_over_stream"] = rec["kernel_us_median"] / rec["stream_once_us"]
        if not a.no_twin:
            ref = Engine(ShallowWater("tc5"), L, grid=grid, dtype=dtype, device="cuda", backend="torch", dt=hip.dt)
            w = timed(ref.derived_fields.compute, a.reps, a.warm)
            rec.update(twin_us_median=statistics.median(w), twin_us_min=min(w),
                       twin_over_kernel=statistics.median(w) / statistics.median(k))
            f0, i0 = d.compute()
            f1, i1 = ref.derived_fields.compute()
            rec["max_field_diff_vs_twin"] = float(((f0 - f1).abs().amax((1, 2, 3)) / f1.abs().amax((1, 2, 3))).max())
            scale = i1.abs()[:6].clone()
            scale[3] = scale[4]          # circulation over abs_circulation
            rec["max_inv_diff_vs_twin"] = float(((i0 - i1).abs()[:6] / scale).max())
            del ref
        print(json.dumps(rec), flush=True)
        del hip, d
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
