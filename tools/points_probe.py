#!/usr/bin/env python
"""Event-time point sampling and the particle advance (ops/points.py, the
launches of ops/csrc/points_kernel.hip) on one GPU.  One JSON line per size:

1. the sample launch (four prognostic channels at K random points) against the
   lat-lon gather kernel run on host-built tables for the same points (the
   gather without the location: the floor), and against the host
   ``locate_points`` plus that gather (what one had to do before);
2. the fused advance launch, per particle;
3. (``--run``) ``Solver.run`` us/step at C96 with K particles at interval 1, 4
   and 16 against the same run without particles.

    python tools/points_probe.py                       # C96 and C720, K = 1e6
    python tools/points_probe.py --run --K 100000      # the run rate at C96
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


def kernels(a):
    import numpy as np
    import torch
    from stsphere.engine import Engine
    from stsphere.models import latlon as ml
    from stsphere.models import points as mp
    from stsphere.models.geometry import CubedSphereGrid
    from stsphere.models.swe import ShallowWater
    from stsphere.ops import native
    from stsphere.parallel.layout import TileLayout
    for size in a.sizes.split(","):
        N, t = (int(v) for v in size.split("x"))
        e = Engine(ShallowWater("tc5"), TileLayout(N, t, 1, ng=2), grid=CubedSphereGrid(N), device="cuda",
                   backend="hip")
        sm = e.points()
        p = mp.random_points(a.K, 1)
        pd = sm.points(p)
        k = timed(lambda: sm.fields(pd), a.reps, a.warm)
        # the floor: the lat-lon gather kernel on tables built on the host for the same points
        t0 = time.perf_counter()
        src, w, _, _ = ml.locate_points(N, p, sm.tab.mesh)
        host_s = time.perf_counter() - t0
        idx = torch.as_tensor(sm.pad_np[src], device="cuda").contiguous()
        wd = torch.as_tensor(w, device="cuda").contiguous()
        out = torch.empty((4, a.K), dtype=e.dtype, device="cuda")
        lib = native.require_native()

        def gather():
            d = native.LatLonDesc()
            d.K, d.nlat, d.nlon = a.K, 1, a.K
            d.Q, d.idx, d.w, d.partial = native.ptr(e.state), native.ptr(idx), native.ptr(wd), native.ptr(out)
            d.cs, d.C, d.phases = sm.S, 4, 1
            native.check(lib.stsp_latlon_launch(native.dtype_code(e.dtype), d, native.current_stream_handle(e.device)),
                         "lat-lon gather")
        g = timed(gather, a.reps, a.warm)
        diff = float(((sm.fields(pd) - out).abs().amax(1) / out.abs().amax(1).clamp_min(1e-300)).max())
        lat, lon = mp.points_lonlat(p)
        P = e.particles(lat, lon, interval=1)
        P.start()
        f = timed(P.advance, a.reps, a.warm)
        rec = {"N": N, "tiles_per_edge": t, "points": a.K, "reps": a.reps,
               "sample_us_median": statistics.median(k), "sample_us_min": min(k),
               "gather_only_us_median": statistics.median(g), "sample_over_gather": statistics.median(k) / statistics.median(g),
               "host_locate_s": host_s, "host_locate_plus_gather_over_sample": (host_s * 1e6 + statistics.median(g)) / statistics.median(k),
               "max_diff_vs_gather": diff,
               "fused_advance_us_median": statistics.median(f), "fused_advance_ns_per_particle": statistics.median(f) * 1e3 / a.K}
        print(json.dumps(rec), flush=True)
        del e, sm, P
        torch.cuda.empty_cache()


def run_rate(a):
    import tempfile

    import stsphere as S
    for interval in (0, 1, 4, 16):
        with tempfile.TemporaryDirectory() as out:
            io = {"output_dir": out}
            if interval:
                io["particles"] = {"count": a.K, "seed": 1, "interval": interval}
            s = S.Solver({"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": "gpu"},
                          "grid": {"N": 96}, "physics": {"model": "swe", "case": "tc5"}, "io": io}, verbose=False)
            s.initialize()
            s.run(nsteps=a.steps)              # warm: graphs, code objects
            r = s.run(nsteps=a.steps)
            print(json.dumps({"N": 96, "particles": a.K if interval else 0, "interval": interval, "steps": a.steps,
                              "us_per_step": r["wall_s"] / r["steps_run"] * 1e6, "runtime": r["runtime"]}), flush=True)
            s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x2,720x2", help="comma list of NxT")
    ap.add_argument("--K", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--run", action="store_true", help="the Solver.run rate with particles instead of the kernels")
    ap.add_argument("--steps", type=int, default=480)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("points_probe needs a GPU")
    run_rate(a) if a.run else kernels(a)


if __name__ == "__main__":
    main()
