#!/usr/bin/env python
"""EOF probe (GPU): the event-timed snapshot decomposition per grid size and
number of snapshots

    kernel   ``ops.eof.Eof.compute`` on contiguous float64 snapshots (four launches
             and the read-back of the error word)
    twin     ``models.eof.eofs`` on the same GPU tensors
    read     one streaming read of the snapshots (``x.sum()``): the kernel reads
             them twice

Everything is built and warmed first; then the timed calls are interleaved in one
process order (kernel twin read kernel twin read ..., ``--rounds`` times), each
between two events on the caller's stream.  Per row: the median and the spread
(min .. max) in microseconds, and for the kernel the GB/s of two reads.

    python tools/eof_probe.py [--N 96,720] [--S 16,64] [--k 8] [--rounds 7] [--out FILE.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="96,720")
    ap.add_argument("--S", default="16,64")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from stsphere.engine import Engine
    from stsphere.models import eof as me
    from stsphere.models.advection import Advection
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.ops.eof import Eof
    from stsphere.parallel.layout import TileLayout

    dev = torch.device("cuda:0")
    rows = []
    for N in [int(v) for v in a.N.split(",")]:
        e = Engine(Advection("cosine_bell"), TileLayout(N, 1, 1, ng=2), grid=CubedSphereGrid(N), device=dev,
                   backend="torch")
        area = torch.as_tensor(e.geo.area, device=dev)
        for S in [int(v) for v in a.S.split(",")]:
            g = torch.Generator(device=dev).manual_seed(S)
            x = 3.0 + torch.randn((S, 6, N, N), generator=g, dtype=torch.float64, device=dev)
            op = Eof(e, S, a.k, padded=False)
            calls = {"kernel": lambda: op.compute(x), "twin": lambda: me.eofs(x, area, a.k), "read": lambda: x.sum()}
            for f in calls.values():
                f()
            torch.cuda.synchronize()
            times = {n: [] for n in calls}
            for _ in range(a.rounds):
                for n, f in calls.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    f()
                    t1.record()
                    t1.synchronize()
                    times[n].append(1e3 * t0.elapsed_time(t1))
            for n, t in times.items():
                row = {"N": N, "S": S, "k": a.k, "what": n, "us_median": statistics.median(t), "us_min": min(t),
                       "us_max": max(t), "rounds": a.rounds}
                if n == "kernel":
                    row["GBps_two_reads"] = 2 * x.numel() * 8 / statistics.median(t) * 1e-3
                rows.append(row)
                print(json.dumps(row), flush=True)
            del x, op
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
