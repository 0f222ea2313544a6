#!/usr/bin/env python
"""Event-time the spherical-harmonic analysis (ops/spectra.py::Spectra, the
analysis and fold launches of ops/csrc/spectra_kernel.hip) of the four
prognostic channels on one GPU, the same coefficients computed by the PyTorch
twin (models/spectra.py) on the same GPU tensors, and one streaming pass over
the state (a device copy of it: what any kernel that reads the state once
costs at least).  Warm repetitions, each timed with its own pair of device
events; one JSON line per size with the medians, the fastest repetition, the
fused multiply-adds of the tall products (cells x sum_m (L + 1 - m) x 16
columns) and the rate that makes.

    python tools/spectra_probe.py                       # C96 t=2 lmax 95, C720 t=2 lmax 255
    python tools/spectra_probe.py --sizes 96x2:95 --dtype fp32 --twin-reps 0
"""
import argparse
import json
import os
import statistics
import sys
import time

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
    ap.add_argument("--sizes", default="96x2:95,720x2:255",
                    help="comma list of NxT:LMAX (cells per panel edge x tiles per edge : largest degree)")
    ap.add_argument("--dtype", default="fp64", choices=["fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--twin-reps", type=int, default=1, help="0: skip the twin")
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine
    from stsphere.models import spectra as ms
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("spectra_probe needs a GPU")
    dtype = torch.float64 if a.dtype == "fp64" else torch.float32
    for size in a.sizes.split(","):
        src, lmax = size.split(":")
        N, t = (int(v) for v in src.split("x"))
        L = int(lmax)
        t0 = time.perf_counter()
        hip = Engine(ShallowWater("tc5"), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N), dtype=dtype,
                     device="cuda", backend="hip")
        hip.step(2)
        sp = hip.spectra(L)
        print(f"C{N} lmax {L}: engine, two steps and tables in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        k = timed(sp.partial_fields, a.reps, a.warm)
        print(f"C{N} lmax {L}: kernel {statistics.median(k) * 1e-3:.2f} ms", file=sys.stderr, flush=True)
        spare = torch.empty_like(hip.state)
        c = timed(lambda: spare.copy_(hip.state), a.reps, a.warm)
        cells = 6 * N * N
        fma = cells * ((L + 1) * (L + 2) // 2) * 16
        rec = {"N": N, "tiles_per_edge": t, "dtype": a.dtype, "lmax": L, "cells": cells, "channels": 4,
               "slabs": sp.slabs, "slab_cells": sp.slab_cells, "reps": a.reps,
               "kernel_us_median": statistics.median(k), "kernel_us_min": min(k),
               "state_copy_us_median": statistics.median(c), "state_bytes": hip.state.numel() * hip.state.element_size(),
               "matrix_fma": fma, "matrix_flops_per_s": 2.0 * fma / (statistics.median(k) * 1e-6)}
        if a.twin_reps:
            # the twin takes seconds to minutes (88 s at C720, lmax 255): no warm call, and
            # the last timed call's result is the one compared
            x = hip.state[:, sp.pad.long()].contiguous()
            w, ref = [], None
            for _ in range(a.twin_reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                ref = ms.analyse(x, sp.tab)
                e1.record()
                e1.synchronize()
                w.append(e0.elapsed_time(e1) * 1e3)
            got = sp.partial_fields()
            rec.update(twin_us_median=statistics.median(w), twin_over_kernel=statistics.median(w) / statistics.median(k),
                       max_diff_vs_twin=float(((got - ref).abs().amax((1, 2, 3)) / ref.abs().amax((1, 2, 3))).max()))
        print(json.dumps(rec), flush=True)
        del hip, sp, spare
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
