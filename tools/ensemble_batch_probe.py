#!/usr/bin/env python
"""Batched-ensemble probe (GPU): SWE TC5, SSP-RK3, MC, per grid size and dtype

    streams   ``Ensemble`` mode 'streams' with 2 members (one runner, graph and
              stream per member)
    batched   ``Ensemble`` mode 'batched' with M = 1, 2, 4, 8, 16, 32 members
              (one launch per stage for all members, one graph)
    fused     one run through the fused step (the path of bench.py)
    stage     one run through the launch-per-stage path (NativeStepper)

Every configuration is built and warmed first; then the timed runs are
interleaved in one process order (A B ... A B ..., ``--rounds`` times), each
between two events on the caller's stream.  Per row: us per step (all members
advance one step), us per member step (that over the members), aggregate
cell-updates/s (members x cells x steps / time) and the block shape.

    python tools/ensemble_batch_probe.py [--N 48,96] [--dtype fp64,fp32] [--members 1,2,4,8,16,32]
                                         [--steps 300] [--warmup 30] [--rounds 2] [--out FILE.json]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="48,96")
    ap.add_argument("--dtype", default="fp64,fp32")
    ap.add_argument("--members", default="1,2,4,8,16,32")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--tpe", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine
    from stsphere.ensemble import Ensemble
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.ops.fused import FusedKernel, rank_cus
    from stsphere.ops.native_runtime import NativeStepper
    from stsphere.parallel.layout import TileLayout

    dev = torch.device("cuda:0")
    factory = lambda: ShallowWater("tc5")
    rows = []
    for N in [int(v) for v in a.N.split(",")]:
        grid = CubedSphereGrid(N)
        L = TileLayout(N, a.tpe, 1, ng=2)
        cells = 6 * N * N
        for dname in a.dtype.split(","):
            dtype = {"fp64": torch.float64, "fp32": torch.float32}[dname]
            kw = dict(amplitude=1e-4, grid=grid, dtype=dtype, device=dev, backend="hip", steps_per_graph=a.steps)
            cfgs = []      # (name, members, block, run(nsteps), close)

            ens = Ensemble(factory, L, 2, **kw)
            c = ens.engines[0].compute
            cfgs.append(("streams", 2, (c.bx, c.by), ens, ens.run))
            for M in [int(m) for m in a.members.split(",")]:
                ens = Ensemble(factory, L, M, mode="batched", **kw)
                cfgs.append(("batched", M, ens.block, ens, ens.run))
            e = Engine(factory(), L, grid=grid, dtype=dtype, device=dev, backend="hip")
            fk = FusedKernel(e)
            even = a.steps - a.steps % 2
            spl = max([k for k in range(2, 513, 2) if even and even % k == 0], default=1) \
                if fk.plan.nb <= rank_cus(dev) else 1
            r = NativeStepper(e, use_graph=True, steps_per_graph=a.steps, fused=fk, steps_per_launch=spl, direct=True)
            cfgs.append(("fused", 1, (fk.plan.B, fk.plan.B), r, r.run))
            e = Engine(factory(), L, grid=grid, dtype=dtype, device=dev, backend="hip")
            r = NativeStepper(e, use_graph=True, steps_per_graph=a.steps)
            cfgs.append(("stage", 1, (e.compute.bx, e.compute.by), r, r.run))

            for name, M, blk, obj, run in cfgs:
                obj.prepare(a.steps)
                run(a.warmup)
            torch.cuda.synchronize()
            times = {i: [] for i in range(len(cfgs))}
            for _ in range(a.rounds):
                for i, (name, M, blk, obj, run) in enumerate(cfgs):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    run(a.steps)
                    t1.record()
                    t1.synchronize()
                    times[i].append(t0.elapsed_time(t1) * 1e-3)
            for i, (name, M, blk, obj, run) in enumerate(cfgs):
                best = min(times[i])
                row = {"N": N, "dtype": dname, "config": name, "members": M, "block": list(blk),
                       "us_per_step": 1e6 * best / a.steps,                    # all members advance one step
                       "us_per_member_step": 1e6 * best / a.steps / M,         # the same, per member
                       "aggregate_cell_updates_per_s": M * cells * a.steps / best,
                       "all_us_per_step": [1e6 * t / a.steps for t in times[i]]}
                rows.append(row)
                print(json.dumps(row), flush=True)
                obj.close()
            del cfgs
            torch.cuda.empty_cache()
    res = {"model": "SWE TC5, SSPRK3, MC-PLR", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "tiles_per_edge": a.tpe, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
