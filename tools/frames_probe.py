#!/usr/bin/env python
"""``Solver.run`` on one GPU with every frame output on: C96 shallow water,
480 steps, history every 48 steps with ``io.latlon``, ``io.spectra`` and 10^5
particles at interval 16 that sample h and u.  One JSON line: cell-updates/s,
us/step and the host time of the history phase of a warm run.  The host side
of the run loop (staging, the frame outputs) is what this measures; compare two
trees by running it on each, interleaved.

    python tools/frames_probe.py                   # this tree
    python tools/frames_probe.py --tree DIR        # the package of another checkout
"""
import argparse
import json
import os
import sys
import tempfile


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this", help="the tree key of the result line")
    ap.add_argument("--pair", type=int, default=None, help="the pair key of the result line (interleaved runs)")
    ap.add_argument("--steps", type=int, default=480)
    ap.add_argument("--K", type=int, default=100000)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import stsphere as S
    with tempfile.TemporaryDirectory() as out:
        io = {"output_dir": out, "history_interval": 48, "latlon": [90, 180], "spectra": 42,
              "particles": {"count": a.K, "seed": 1, "interval": 16, "fields": ["h", "u"]}}
        s = S.Solver({"parallelization": {"tiles_per_edge": 2, "num_devices": 1, "device_type": "gpu"},
                      "grid": {"N": 96}, "physics": {"model": "swe", "case": "tc5"}, "io": io}, verbose=False)
        s.initialize()
        s.run(nsteps=a.steps)              # warm: graphs, code objects, tables
        r = s.run(nsteps=a.steps)
        print(json.dumps({"tree": a.label, "pair": a.pair, "N": 96, "steps": r["steps_run"], "particles": a.K,
                          "cell_updates_per_s": r["cell_updates_per_s"],
                          "us_per_step": r["wall_s"] / r["steps_run"] * 1e6,
                          "history_s": r["phase_s"].get("history", 0.0), "phase_s": r["phase_s"],
                          "runtime": r["runtime"]}), flush=True)
        s.close()


if __name__ == "__main__":
    main()
