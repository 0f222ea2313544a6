#!/usr/bin/env python
"""Time the consistent thermal diffusion (ops/csrc/heat_kernel.hip) on one GPU.

Part 1, per size (default C96 t = 2 and C720 t = 3, fp64, SSP-RK3): device-event
time of one step of the consistent operator (per stage two launches, per step
one indexed copy of the ghost slots), against one step of the two-point operator
on the stage kernel with the same 16 x 16 block, both stepped eagerly through
``Engine.step``, and against one streaming copy of the state (16 bytes per
cell).  The configurations are timed interleaved (round r times each of them
once, ``--reps`` steps per window).

Part 2, C96: ``Solver.run`` cell-updates/s with ``physics.operator: consistent``
(eager) and ``two_point`` (the native runtime's graph replay), interleaved the
same way.

One JSON line per size and one for part 2.  ``least_bytes_per_cell``: what the
two passes of one stage must move per cell (fp64 state): pass 1 reads 1 value
and 12 weights and writes 4 scratch rows (136 B); pass 2 reads 4 scratch rows,
2 + 6 edge-table values, 1 / A, X and Q and writes 1 (128 B).  The neighbours'
rows are re-reads of lines a block already touches and are not counted.

    python tools/heat_probe.py
    python tools/heat_probe.py --sizes 96x2 --no-run
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEAST_BYTES = {"pass1": 8 * (1 + 12 + 4), "pass2": 8 * (4 + 2 + 6 + 1 + 1 + 1 + 1)}
STAGES = 3


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def steps(N, t, reps, rounds):
    import torch
    from stsphere.engine import Engine
    from stsphere.models.diffusion import ConsistentDiffusion, Diffusion
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.parallel.layout import TileLayout
    grid = CubedSphereGrid(N)
    kw = dict(grid=grid, device="cuda", backend="hip", integrator="ssprk3")
    con = Engine(ConsistentDiffusion(case="harmonic32"), TileLayout(N, t, 1, ng=2), **kw)
    two = Engine(Diffusion(case="harmonic32"), TileLayout(N, t, 1, ng=2), block=(16, 16), **kw)
    assert con.compute.op.hip and type(two.compute).__name__ == "HipCompute"
    buf = torch.empty_like(con.state)
    fns = {"state_copy": lambda: buf.copy_(con.state), "consistent_step": con.step, "two_point_step": two.step}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(_time(fn, reps))
    assert bool(torch.isfinite(con.tiles_view()).all()) and bool(torch.isfinite(two.tiles_view()).all())
    stage = sum(LEAST_BYTES.values())
    rec = {"N": N, "tiles_per_edge": t, "cells": 6 * N * N, "dtype": "float64", "integrator": "ssprk3", "reps": reps,
           "rounds": rounds,
           "least_bytes_per_cell": dict(LEAST_BYTES, stage=stage, step=STAGES * stage, state_copy=16)}
    base = statistics.median(ts["state_copy"])
    for k, v in ts.items():
        med = statistics.median(v)
        rec[k] = {"us": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2),
                  "ratio_to_state_copy": round(med / base, 2)}
    rec["consistent_step"]["launches"] = 2 * STAGES + 1
    rec["consistent_step"]["least_GB_per_s"] = round(STAGES * stage * 6 * N * N / rec["consistent_step"]["us"] * 1e-3, 1)
    rec["consistent_step"]["ratio_to_two_point_step"] = round(rec["consistent_step"]["us"] / rec["two_point_step"]["us"], 2)
    rec["two_point_step"]["launches"] = STAGES
    print(json.dumps(rec), flush=True)


def runs(N, t, nsteps, rounds):
    import tempfile
    import torch
    out = tempfile.mkdtemp(prefix="heat_probe_")
    from stsphere.driver import Solver
    solvers = {}
    for name in ("two_point", "consistent"):
        c = {"parallelization": {"tiles_per_edge": t, "num_devices": 1, "device_type": "gpu"},
             "grid": {"N": N, "halo": 2, "dtype": "float64"},
             "physics": {"model": "diffusion", "case": "harmonic32", "operator": name},
             "time": {"integrator": "ssprk3"}, "io": {"output_dir": os.path.join(out, name)}}
        solvers[name] = Solver(c, verbose=False)
        solvers[name].run(nsteps=nsteps)          # warm: graphs, tables, code objects
    torch.cuda.synchronize()
    rates = {k: [] for k in solvers}
    kinds = {}
    for _ in range(rounds):
        for k, s in solvers.items():
            r = s.run(nsteps=nsteps)
            rates[k].append(r["cell_updates_per_s"])
            kinds[k] = r["runtime"]
    rec = {"part": "run", "N": N, "tiles_per_edge": t, "nsteps": nsteps, "rounds": rounds, "runtime": kinds}
    base = statistics.median(rates["two_point"])
    for k, v in rates.items():
        rec[k] = {"cell_updates_per_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                  "us_per_step": round(6 * N * N / statistics.median(v) * 1e6, 2),
                  "ratio_to_two_point": round(statistics.median(v) / base, 3)}
    for k, s in solvers.items():
        assert s.all_finite(), k
        s.close()
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x2,720x3", help="N x tiles per edge, comma separated")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--run-steps", type=int, default=960)
    ap.add_argument("--no-run", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("heat_probe: needs a GPU (no timing without one)")
    for size in a.sizes.split(","):
        N, t = (int(v) for v in size.split("x"))
        steps(N, t, a.reps, a.rounds)
    if not a.no_run:
        runs(96, 2, a.run_steps, a.rounds)


if __name__ == "__main__":
    main()
