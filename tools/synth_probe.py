#!/usr/bin/env python
"""Event-time the spherical-harmonic synthesis (ops/spectra.py::Spectra.synthesise,
the launches of ops/csrc/synth_kernel.hip, with the torch gather that packs the
coefficients) of four channels on one GPU, against

* the analysis of the same shape (``Spectra.partial_fields``, four channels,
  ops/csrc/spectra_kernel.hip): the same number of multiply-adds, cells x
  sum_m (L + 1 - m) x 16 columns, measured in the same run;
* the PyTorch twin (models/spectra.py::synthesise) on the same GPU tensors.  It
  holds a whole Legendre column [L + 1 - m, cells] at a time; where that does
  not fit in the free memory the twin is skipped and the record says so.

Warm repetitions, each timed with its own pair of device events; one JSON line
per size with the medians, the fastest repetition, the chunk count and the
multiply-add rate.

    python tools/synth_probe.py                       # C96 t=2 lmax 95, C720 t=2 lmax 255
    python tools/synth_probe.py --sizes 96x2:95 --twin-reps 0 --chunks 1,2,4
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--twin-reps", type=int, default=1, help="0: skip the twin")
    ap.add_argument("--chunks", default="", help="comma list of further chunk counts to time besides the default")
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine
    from stsphere.models import spectra as ms
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("synth_probe needs a GPU")
    for size in a.sizes.split(","):
        src, lmax = size.split(":")
        N, t = (int(v) for v in src.split("x"))
        L = int(lmax)
        t0 = time.perf_counter()
        hip = Engine(ShallowWater("tc5"), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N), dtype=torch.float64,
                     device="cuda", backend="hip")
        hip.step(2)
        sp = hip.spectra(L)
        print(f"C{N} lmax {L}: engine, two steps and tables in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        an = timed(sp.partial_fields, a.reps, a.warm)
        co = sp.partial_fields()                         # the four prognostic channels' own coefficients
        sy = timed(lambda: sp.synthesise(co), a.reps, a.warm)
        pk = timed(lambda: ms.pack_coeffs(co, sp._pack_index), a.reps, a.warm)
        print(f"C{N} lmax {L}: analysis {statistics.median(an) * 1e-3:.2f} ms, synthesis "
              f"{statistics.median(sy) * 1e-3:.2f} ms", file=sys.stderr, flush=True)
        cells = 6 * N * N
        fma = cells * ((L + 1) * (L + 2) // 2) * 16
        rec = {"N": N, "tiles_per_edge": t, "lmax": L, "cells": cells, "channels": 4, "reps": a.reps,
               "chunks": sp.default_chunks(), "bounds": ms.chunk_bounds(L, sp.default_chunks()),
               "synth_us_median": statistics.median(sy), "synth_us_min": min(sy),
               "pack_us_median": statistics.median(pk),
               "analysis_us_median": statistics.median(an), "analysis_us_min": min(an),
               "analysis_slabs": sp.slabs,
               "synth_over_analysis": statistics.median(sy) / statistics.median(an),
               "matrix_fma": fma, "synth_matrix_flops_per_s": 2.0 * fma / (statistics.median(sy) * 1e-6),
               "analysis_matrix_flops_per_s": 2.0 * fma / (statistics.median(an) * 1e-6)}
        for k in [int(v) for v in a.chunks.split(",") if v]:
            if 1 <= k <= L + 1:
                rec[f"synth_us_median_chunks_{k}"] = statistics.median(timed(lambda: sp.synthesise(co, chunks=k), a.reps, a.warm))
        if a.twin_reps:
            # the twin holds P [L + 1, cells] and the stack of its rows: about twice that, plus the products
            need = 3 * (L + 1) * cells * 8
            free = torch.cuda.mem_get_info()[0]
            if need > free:
                rec.update(twin_skipped=f"the twin needs about {need / 2 ** 30:.1f} GiB, {free / 2 ** 30:.1f} GiB are free")
            else:
                # seconds to minutes: no warm call, and the last timed call's result is the one compared
                w, ref = [], None
                for _ in range(a.twin_reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ref = ms.synthesise(co, sp.tab)
                    e1.record()
                    e1.synchronize()
                    w.append(e0.elapsed_time(e1) * 1e3)
                got = sp.synthesise(co).reshape(4, -1)
                rec.update(twin_us_median=statistics.median(w),
                           twin_over_synth=statistics.median(w) / statistics.median(sy),
                           max_diff_vs_twin=float(((got - ref).abs().amax(1) / ref.abs().amax(1)).max()))
        print(json.dumps(rec), flush=True)
        del hip, sp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
