#!/usr/bin/env python
"""Time the scale-selective dissipation (ops/csrc/dissipation_kernel.hip) on one GPU.

Part 1, per size (default C96 and C720, fp64): device-event time of one
application of order 1 (two launches) and order 2 (four), against one
streaming pass over the state (a copy of its four rows: 64 bytes per cell) and,
at C96, against one fused SSP-RK3 step.  The configurations are timed
interleaved (round r times each of them once, ``--reps`` calls per window).

Part 2, C96: ``Solver.run`` cell-updates/s with ``physics.dissipation.interval``
1, 4 and 16 against the same run without dissipation, interleaved the same way.

One JSON line per size and one for part 2.  ``least_bytes_per_cell``: what the
two passes must move per cell and application without a topography (fp64
state): pass 1 reads 4 state values and 12 weights and writes 16 scratch rows
(256 B); pass 2 reads 16 scratch rows, 2 + 6 edge-table values, 1 / A, the
centre (3) and the own state cell (4) and writes 4 (288 B).  The scratch
(256 B) and the weights (96 B) dominate.

    python tools/dissipation_probe.py
    python tools/dissipation_probe.py --sizes 96x2 --no-run
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEAST_BYTES = {"pass1": 8 * (4 + 12 + 16), "pass2": 8 * (16 + 2 + 6 + 1 + 3 + 4 + 4)}


def _time(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernels(N, t, reps, rounds, fused):
    import torch
    from stsphere.engine import Engine
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    e = Engine(ShallowWater("galewsky"), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N), device="cuda",
               backend="hip")
    lam = e.dissipation().lam
    tau = e.dt
    # a quarter of the explicit bound: one sub-step, and the state stays smooth over the timed calls
    ops = {"order1": e.dissipation(1, 0.25 / (2.0 * tau * lam)), "order2": e.dissipation(2, 0.25 / (tau * (2.0 * lam) ** 2))}
    buf = torch.empty_like(e.state)
    fns = {"state_pass": lambda: buf.copy_(e.state)}
    for k, d in ops.items():
        assert d.substeps(tau) == 1
        fns[k] = lambda d=d: d.apply(tau)
    if fused:
        from stsphere.ops.fused import FusedKernel
        e2 = Engine(ShallowWater("galewsky"), TileLayout(N, t, 1, ng=2), grid=e.grid, device="cuda", backend="hip")
        fk = FusedKernel(e2)
        fns["fused_step"] = lambda: fk.launch(0, nsteps=2)
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(_time(fn, reps))
    if fused:
        fk.check()
    assert bool(torch.isfinite(e.tiles_view()).all())
    rec = {"N": N, "tiles_per_edge": t, "cells": 6 * N * N, "dtype": "float64", "reps": reps, "rounds": rounds,
           "least_bytes_per_cell": dict(LEAST_BYTES, application=sum(LEAST_BYTES.values()), state_pass=64)}
    base = statistics.median(ts["state_pass"])
    for k, v in ts.items():
        med = statistics.median(v) / (2 if k == "fused_step" else 1)       # the fused launch covers two steps
        rec[k] = {"us": round(med, 2), "min": round(min(v) / (2 if k == "fused_step" else 1), 2),
                  "max": round(max(v) / (2 if k == "fused_step" else 1), 2), "ratio_to_state_pass": round(med / base, 2)}
    for k, launches in (("order1", 2), ("order2", 4)):
        rec[k]["launches"] = launches
        rec[k]["least_GB_per_s"] = round(launches // 2 * sum(LEAST_BYTES.values()) * 6 * N * N / rec[k]["us"] * 1e-3, 1)
    print(json.dumps(rec), flush=True)


def runs(N, t, nsteps, rounds):
    import tempfile
    import torch
    out = tempfile.mkdtemp(prefix="dissipation_probe_")
    from stsphere.driver import Solver
    solvers = {}
    for name, iv in (("none", 0), ("interval_1", 1), ("interval_4", 4), ("interval_16", 16)):
        c = {"parallelization": {"tiles_per_edge": t, "num_devices": 1, "device_type": "gpu"},
             "grid": {"N": N, "halo": 2, "dtype": "float64"},
             "physics": {"model": "swe", "case": "galewsky", "limiter": "mc"},
             "time": {"integrator": "ssprk3", "dt": 80.0}, "io": {"output_dir": os.path.join(out, name)}}
        if iv:
            c["physics"]["dissipation"] = {"order": 1, "nu": 1.0e5, "interval": iv}
        solvers[name] = Solver(c, verbose=False)
        solvers[name].run(nsteps=nsteps)          # warm: graphs, tables, code objects
    torch.cuda.synchronize()
    rates = {k: [] for k in solvers}
    for _ in range(rounds):
        for k, s in solvers.items():
            rates[k].append(s.run(nsteps=nsteps)["cell_updates_per_s"])
    rec = {"part": "run", "N": N, "tiles_per_edge": t, "nsteps": nsteps, "rounds": rounds,
           "runtime": "fused" if solvers["none"].fused is not None else "native"}
    base = statistics.median(rates["none"])
    for k, v in rates.items():
        rec[k] = {"cell_updates_per_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                  "ratio_to_none": round(statistics.median(v) / base, 3)}
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
        raise SystemExit("dissipation_probe: needs a GPU (no timing without one)")
    for size in a.sizes.split(","):
        N, t = (int(v) for v in size.split("x"))
        kernels(N, t, a.reps, a.rounds, fused=N == 96)
    if not a.no_run:
        runs(96, 2, a.run_steps, a.rounds)


if __name__ == "__main__":
    main()
