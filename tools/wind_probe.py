#!/usr/bin/env python
"""Time the time-dependent wind of the advection model (ops/csrc/wind_kernel.hip)
on one GPU, and run the deformational-flow tests there.

Part 1, per size (default C96 t = 2 and C720 t = 3, fp64, MC): device-event time
of one SSP-RK3 step of ``deform_nd`` (per stage one table launch ahead of the
stage kernel, per step one tick) against one step of ``solid_body`` (static
tables) with the same block, both eager through ``Engine.step`` and replayed
through ``engine.GraphStepper``.  The configurations are timed interleaved in one
process (round r times each of them once, ``--reps`` steps per window).
``least_bytes_per_cell`` (fp64): a stage of the stage kernel reads Q, X and 1 / A
per cell and one ex and one ey per cell (each edge has two cells; the second read
hits a line the block already holds) and writes one value, 48 B; the table launch
reads four vertex factors per vertex, one vertex per cell, and writes one ex and
one ey per cell, 48 B more.

Part 2 (``--norms``): twelve days of ``deform_nd`` with each of the three cases
at C48 and C96 with MC and PPM through ``Solver.run``: the error norms at t = T,
the extrema and the relative mass drift.

One JSON line per size and per run.

    python tools/wind_probe.py
    python tools/wind_probe.py --sizes 96x2 --norms
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEAST_BYTES = {"stage": 8 * (1 + 1 + 1 + 2 + 1), "wind": 8 * (4 + 2)}
STAGES = 3


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn(reps)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def steps(N, t, reps, rounds):
    import torch
    from stsphere.engine import Engine, GraphStepper
    from stsphere.models.advection import Advection
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.parallel.layout import TileLayout
    grid = CubedSphereGrid(N)
    kw = dict(grid=grid, device="cuda", backend="hip", integrator="ssprk3")
    mk = lambda flow, **k: Engine(Advection("cosine_bells", flow=flow), TileLayout(N, t, 1, ng=2), **kw, **k)
    d_e = mk("deform_nd")
    block = (d_e.compute.bx, d_e.compute.by)
    dt = d_e.dt
    s_e, d_g, s_g = mk("solid_body", block=block, dt=dt), mk("deform_nd", dt=dt), mk("solid_body", block=block, dt=dt)
    assert d_e.clock is not None and s_e.clock is None and (d_g.compute.bx, d_g.compute.by) == block
    gd, gs = GraphStepper(d_g, steps_per_graph=reps), GraphStepper(s_g, steps_per_graph=reps)
    fns = {"deform_eager": d_e.step, "solid_eager": s_e.step, "deform_graph": gd.run, "solid_graph": gs.run}
    for fn in fns.values():
        fn(reps)
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(_time(fn, reps))
    for e in (d_e, s_e, d_g, s_g):
        assert bool(torch.isfinite(e.tiles_view()).all())
    assert int(d_g.clock.count) == d_g.step_count and int(d_e.clock.count) == d_e.step_count
    rec = {"N": N, "tiles_per_edge": t, "cells": 6 * N * N, "dtype": "float64", "integrator": "ssprk3",
           "limiter": "mc", "block": list(block), "reps": reps, "rounds": rounds,
           "launches_per_step": {"deform": 2 * STAGES + 1, "solid": STAGES},
           "least_bytes_per_cell": {"solid_step": STAGES * LEAST_BYTES["stage"],
                                    "deform_step": STAGES * (LEAST_BYTES["stage"] + LEAST_BYTES["wind"])}}
    for k, v in ts.items():
        rec[k] = {"us": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
    for mode in ("eager", "graph"):
        rec[f"ratio_{mode}"] = round(rec[f"deform_{mode}"]["us"] / rec[f"solid_{mode}"]["us"], 3)
        rec[f"deform_{mode}"]["least_GB_per_s"] = round(
            rec["least_bytes_per_cell"]["deform_step"] * 6 * N * N / rec[f"deform_{mode}"]["us"] * 1e-3, 1)
    print(json.dumps(rec), flush=True)


def norms(sizes, cases, limiters):
    import tempfile
    from stsphere.driver import Solver
    out = tempfile.mkdtemp(prefix="wind_probe_")
    for N in sizes:
        for case in cases:
            for lim in limiters:
                c = {"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": "gpu"},
                     "grid": {"N": N, "dtype": "float64"},
                     "physics": {"model": "advection", "case": case, "flow": "deform_nd", "limiter": lim},
                     "time": {"integrator": "ssprk3", "cfl": 0.9, "days": 12},
                     "io": {"output_dir": os.path.join(out, f"{N}_{case}_{lim}")}}
                s = Solver(c, verbose=False)
                r = s.run()
                rec = {"part": "norms", "N": N, "case": case, "limiter": lim, "flow": "deform_nd", "steps": r["steps"],
                       "runtime": r["runtime"], "graph_steps": r["graph_steps"], "wall_s": round(r["wall_s"], 3)}
                rec.update({k: r[k] for k in ("err_l1", "err_l2", "err_linf", "q_min", "q_max", "mass_drift")})
                s.close()
                print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x2,720x3", help="N x tiles per edge, comma separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--norms", action="store_true", help="part 2: the twelve-day error norms")
    ap.add_argument("--no-steps", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wind_probe: needs a GPU (no timing without one)")
    if not a.no_steps:
        for size in a.sizes.split(","):
            N, t = (int(v) for v in size.split("x"))
            steps(N, t, a.reps, a.rounds)
    if a.norms:
        norms((48, 96), ("cosine_bells", "gaussian_hills", "slotted_cylinders"), ("mc", "ppm"))


if __name__ == "__main__":
    main()
