#!/usr/bin/env python
"""Event-time one SSP-RK3 step of shallow water with NQ = 1, 2, 4 tracers
(ops/csrc/swe_tracer_stage.hip; PLR tracers and the monotone PPM) against plain shallow water on the stage
kernel (stage_kernel.hip, the path of ``runtime.fused: off``) with the same
block shape, on one GPU: fp64, MC limiter, three launches per step, replayed
from a hipGraph of ``--reps`` steps (eager launches from Python measure the
host's launch rate at C96, about 7 us per launch, not the kernels).

The configurations are timed interleaved (round r times every configuration
once, ``--reps`` steps each), so a drift of the box hits all of them alike.
One JSON line per size: median us/step of each configuration, its ratio to
plain SWE, and the least bytes a step moves per cell (every stage reads and
writes 4 + NQ fields once) against the 4 fields of plain SWE.

``nqK_ppm`` rows: the same tracers on the monotone PPM (``tracer_limiter:
ppm``, a layout with three ghost layers), with the ratio to the PLR-tracer row
of the same NQ and the ratio of window cells per block ((bx + 6)(by + 6) against
(bx + 4)(by + 4)); the least bytes per cell are those of the PLR row.  All
configurations of a size share one block shape: the tracer kernel's choice for
the largest configuration timed (``--no-ppm`` leaves the PPM rows out).

    python tools/tracer_probe.py                      # C96 and C360
    python tools/tracer_probe.py --sizes 96x2 --block 16,16 --nq 1
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
    ap.add_argument("--block", default="", help="bx,by for every configuration (default: the tracer kernel's choice)")
    ap.add_argument("--reps", type=int, default=50, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--nq", default="1,2,4", help="tracer counts, comma separated")
    ap.add_argument("--no-ppm", action="store_true", help="PLR tracers only")
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine, GraphStepper
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater, ShallowWaterTracers
    from stsphere.ops.hip_compute import choose_tracer_block
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("tracer_probe: needs a GPU (no timing without one)")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    names = ["cap", "cosine_bell", "gradient", "constant"]
    for size in a.sizes.split(","):
        N, t = (int(v) for v in size.split("x"))
        nqs = [int(v) for v in a.nq.split(",")]
        block = tuple(int(v) for v in a.block.split(",")) if a.block else \
            choose_tracer_block(N // t, 6 * t * t, cus, max(nqs), 8, 0 if a.no_ppm else 4)
        grid, L, L3 = CubedSphereGrid(N), TileLayout(N, t, 1, ng=2), TileLayout(N, t, 1, ng=3)
        mk = lambda p, lay=L: Engine(p, lay, grid=grid, device="cuda", backend="hip", block=block)   # noqa: E731
        eng = {"swe": mk(ShallowWater("tc5", limiter=2))}
        for nq in nqs:
            eng[f"nq{nq}"] = mk(ShallowWaterTracers("tc5", tracers=names[:nq], limiter=2))
        if not a.no_ppm:
            for nq in nqs:
                eng[f"nq{nq}_ppm"] = mk(ShallowWaterTracers("tc5", tracers=names[:nq], limiter=2,
                                                            tracer_limiter="ppm"), L3)
        run = {}
        for k, e in eng.items():
            e.dt = eng["swe"].dt
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
            if k.endswith("_ppm"):
                rec[k]["ratio_to_plr"] = round(med / statistics.median(ts[k[:-4]]), 3)
                rec[k]["window_cells_ratio"] = round((block[0] + 6) * (block[1] + 6) / ((block[0] + 4) * (block[1] + 4)), 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
