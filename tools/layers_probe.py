#!/usr/bin/env python
"""Event-time one SSP-RK3 step of two-layer shallow water
(ops/csrc/swe_layer_stage.hip) against plain shallow water on the stage kernel
(stage_kernel.hip, the path of ``runtime.fused: off``) with the same block
shape, on one GPU: fp64, MC limiter, three launches per step, replayed from a
hipGraph of ``--reps`` steps (eager launches from Python measure the host's
launch rate at C96, not the kernels).

The two configurations are timed interleaved (round r times each once,
``--reps`` steps each), so a drift of the box hits both alike.  One JSON line
per size: median us/step of each, the ratio of the two-layer step to the plain
one, and the least bytes a step moves per cell (every stage reads and writes
its fields once: 8 against 4).  Two layers are expected to cost about two plain
steps; the ratio is reported, nothing is gated on it.

    python tools/layers_probe.py                      # C96 and C360
    python tools/layers_probe.py --sizes 96x2 --block 16,16
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x2,360x3", help="N x tiles per edge, comma separated")
    ap.add_argument("--block", default="", help="bx,by for both configurations (default: the layer kernel's choice)")
    ap.add_argument("--reps", type=int, default=50, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warm", type=int, default=10)
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine, GraphStepper
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import LayeredShallowWater, ShallowWater
    from stsphere.ops.hip_compute import choose_layer_block
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("layers_probe: needs a GPU (no timing without one)")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for size in a.sizes.split(","):
        N, t = (int(v) for v in size.split("x"))
        block = tuple(int(v) for v in a.block.split(",")) if a.block else choose_layer_block(N // t, 6 * t * t, cus, 8)
        grid, L = CubedSphereGrid(N), TileLayout(N, t, 1, ng=2)
        mk = lambda p: Engine(p, L, grid=grid, device="cuda", backend="hip", block=block)   # noqa: E731
        eng = {"swe": mk(ShallowWater("tc5", limiter=2)),
               "layers2": mk(LayeredShallowWater("tc5", depths=[2000.0, 5960.0], density_ratio=0.9, limiter=2))}
        run = {}
        dt = min(e.dt for e in eng.values())
        for k, e in eng.items():
            e.dt = dt
            run[k] = GraphStepper(e, steps_per_graph=a.reps)
            run[k].run(run[k].k * max(1, a.warm // run[k].k + 1))   # k: whole graphs (a multiple of the buffer period)
        torch.cuda.synchronize()
        ts = {k: [] for k in eng}
        for _ in range(a.rounds):
            for k, e in eng.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run[k].run(run[k].k)
                e1.record()
                e1.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / run[k].k)
        for k, e in eng.items():
            assert bool(torch.isfinite(e.tiles_view()).all()), k
        esize, stages = 8, 3
        rec = {"N": N, "tiles_per_edge": t, "block": list(block), "cells": 6 * N * N, "reps": a.reps,
               "rounds": a.rounds, "launches": "one per stage, graph replay"}
        base = statistics.median(ts["swe"])
        for k in eng:
            F = eng[k].physics.F
            med = statistics.median(ts[k])
            rec[k] = {"us_per_step": round(med, 2), "min": round(min(ts[k]), 2), "max": round(max(ts[k]), 2),
                      "ratio_to_swe": round(med / base, 3), "fields": F,
                      "min_bytes_per_cell_step": 2 * F * esize * stages, "byte_ratio_to_swe": F / 4}
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
