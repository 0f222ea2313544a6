#!/usr/bin/env python
"""Event-time the grid transfer (ops/transfer.py::Transfer, one launch of
ops/csrc/transfer_kernel.hip) on one GPU for shallow water: refine C48 -> C96,
refine C96 -> C768 (r = 8) and coarsen C720 -> C360, interleaved with one streaming
copy of the target state in each repetition.  One JSON line per case with the
medians, the least bytes a transfer must move per target cell (the target rows
written once, the source rows read once) and the rate that makes, the wall time of
the twin (models/transfer.py, on the host) and the largest difference against it.

    python tools/transfer_probe.py
    python tools/transfer_probe.py --cases 48:96 --dtype fp32 --no-twin
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def event_us(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="48:96,96:768,720:360", help="comma list of Ns:N")
    ap.add_argument("--dtype", default="fp64", choices=["fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--no-twin", action="store_true")
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.parallel.layout import TileLayout
    if not torch.cuda.is_available():
        raise SystemExit("transfer_probe needs a GPU")
    dtype = torch.float64 if a.dtype == "fp64" else torch.float32
    for Ns, N in (tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")):
        s = Engine(ShallowWater("tc5"), TileLayout(Ns, 1, 1, ng=2), grid=CubedSphereGrid(Ns))
        src = s.tiles_view().double().to("cuda").contiguous()              # one tile per panel: [F, 6, Ns, Ns]
        e = Engine(ShallowWater("tc5"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), dtype=dtype, device="cuda",
                   backend="hip")
        op, buf = e.transfer, torch.empty_like(e.state)
        ts, copy = [], []
        for r in range(a.warm + a.reps):
            t = event_us(lambda: op.apply(src, e.state))
            c = event_us(lambda: buf.copy_(e.state))
            if r >= a.warm:
                ts.append(t)
                copy.append(c)
        cells = 6 * N * N
        least = e.physics.F * (e.state.element_size() + 8.0 * (Ns / N) ** 2)
        med = statistics.median(ts)
        rec = {"Ns": Ns, "N": N, "dtype": a.dtype, "reps": a.reps, "transfer_us_median": med, "transfer_us_min": min(ts),
               "state_copy_us_median": statistics.median(copy), "least_bytes_per_cell": least,
               "rate_GBps_at_least_bytes": least * cells / med * 1e-3}
        if not a.no_twin:
            t0 = time.perf_counter()
            ref = op.twin(src)
            rec["twin_host_s"] = time.perf_counter() - t0
            got = e.tiles_view().double().cpu()
            rec["max_diff_vs_twin"] = float(((got - ref).abs().amax((1, 2, 3)) / ref.abs().amax((1, 2, 3)).clamp_min(1e-300)).max())
        print(json.dumps(rec), flush=True)
        del e, op, buf, s, src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
