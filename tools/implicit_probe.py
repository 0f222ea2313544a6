#!/usr/bin/env python
"""Time the implicit consistent diffusion (ops/csrc/helmholtz_kernel.hip) on one GPU.

Per size (default C96 t = 2 and C720 t = 3, fp64, the ``harmonic`` case): device-event
time of one implicit step at ``--factor`` (default 50) times the explicit bound
1 / (2 kappa lam), backward Euler and Crank-Nicolson, against ``--factor`` explicit
SSP-RK3 steps of the consistent operator at the bound (the same simulated time, on the
kernels of heat_kernel.hip).  The configurations are timed interleaved in one process
(round r times each of them once, from the same initial state), and the medians are
reported with the iterations per solve and the microseconds per iteration (10 launches).
The host reads the 16-byte record once per chunk of 8 iterations; that wait is inside
the implicit step's time.

One JSON line per size.

    python tools/implicit_probe.py
    python tools/implicit_probe.py --sizes 96x2 --rounds 5
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LAUNCHES_PER_ITERATION = 10


def probe(N, t, factor, rounds, tol):
    import torch
    from stsphere.engine import Engine
    from stsphere.models.diffusion import ConsistentDiffusion
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.parallel.layout import TileLayout
    grid = CubedSphereGrid(N)
    ph = ConsistentDiffusion(case="harmonic")
    bound = ph.max_dt(grid, 1.0)
    e = Engine(ph, TileLayout(N, t, 1, ng=2), grid=grid, device="cuda", backend="hip", integrator="ssprk3", dt=bound)
    op = e.heat_operator()
    assert op.hip
    T0 = e.tiles_view().clone()
    its, failed = {}, {}

    def implicit(theta):
        def run():
            try:
                r = op.implicit_step(factor * bound, ph.kappa, theta, tol=tol)
            except RuntimeError as err:      # stagnation or breakdown: reported, not hidden
                r = err.record
                failed[theta] = r
            its.setdefault(theta, []).append(r["iterations"])
        return run
    fns = {"explicit_ssprk3": lambda: e.step(factor), "backward_euler": implicit(1.0), "crank_nicolson": implicit(0.5)}

    def timed(fn):
        e.set_state(T0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3
    for fn in fns.values():              # warm: code objects, the solver's buffers, the pinned record
        timed(fn)
    its.clear()
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn))
    assert bool(torch.isfinite(e.tiles_view()).all())
    rec = {"N": N, "tiles_per_edge": t, "cells": 6 * N * N, "dtype": "float64", "factor": factor, "tol": tol,
           "explicit_bound_s": bound, "rounds": rounds}
    for k, v in ts.items():
        rec[k] = {"us": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    base = rec["explicit_ssprk3"]["us"]
    rec["explicit_ssprk3"]["steps"] = factor
    for k, theta in (("backward_euler", 1.0), ("crank_nicolson", 0.5)):
        n = statistics.median(its[theta])
        rec[k].update(iterations=n, iterations_min=min(its[theta]), iterations_max=max(its[theta]),
                      us_per_iteration=round(rec[k]["us"] / n, 2), launches_per_iteration=LAUNCHES_PER_ITERATION,
                      ratio_to_explicit=round(rec[k]["us"] / base, 3), not_converged=failed.get(theta))
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x2,720x3", help="N x tiles per edge, comma separated")
    ap.add_argument("--factor", type=int, default=50, help="implicit dt over the explicit bound")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tol", type=float, default=1e-10)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("implicit_probe: needs a GPU (no timing without one)")
    for size in a.sizes.split(","):
        N, t = (int(v) for v in size.split("x"))
        probe(N, t, a.factor, a.rounds, a.tol)


if __name__ == "__main__":
    main()
