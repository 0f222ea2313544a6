#!/usr/bin/env python
"""Launch-per-stage C96 step of a loopback rank: every ghost goes through the
rank's own xGMI ring (the XG stage kernel fp64 / fp32 and the XG streaming
stage), graph replay of 100 steps, five timings each, us/step.  One JSON line.

    python tools/xg_stage_probe.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stsphere.engine import Engine
from stsphere.models.geometry import CubedSphereGrid
from stsphere.models.swe import ShallowWater
from stsphere.ops.native_runtime import NativeStepper
from stsphere.ops.xgmi import XgmiHalo
from stsphere.parallel.comm import NativeBuffers
from stsphere.parallel.layout import TileLayout

out = {}
for name, dtype, block in (("stage_fp64", torch.float64, None), ("stage_fp32", torch.float32, None),
                           ("march_fp64", torch.float64, (64, 4))):
    N, t, steps = 96, 2, 100
    L = TileLayout(N, t, 1, ng=2, loopback=True)
    kw = {"block": block} if block else {}
    b = Engine(ShallowWater("tc5"), L, grid=CubedSphereGrid(N), device="cuda", backend="hip", dtype=dtype,
               transport=NativeBuffers(L.plan(0), 4, dtype, torch.device("cuda")), **kw)
    xg = XgmiHalo(b, timeout_s=1.0)
    ns = NativeStepper(b, use_graph=True, steps_per_graph=steps, xgmi=xg)
    ns.run(steps)
    torch.cuda.synchronize()
    ts = []
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(5):
        s0.record()
        ns.run(steps)
        s1.record()
        torch.cuda.synchronize()
        ts.append(s0.elapsed_time(s1) * 1e3 / steps)
    ns.check()
    out[name] = [round(x, 3) for x in ts]
    ns.close()
    xg.close()
print(json.dumps(out), flush=True)
