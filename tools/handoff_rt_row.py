#!/usr/bin/env python
"""One summary row of tools/handoff_rt_ab.sh: the figures of one (variant, rep)
from its probe and bench outputs.

    python tools/handoff_rt_row.py OUT_DIR VARIANT REP
"""
import json
import sys


def last(path):
    return json.loads(open(path).read().strip().splitlines()[-1])


def main():
    out, v, rep = sys.argv[1:4]
    a = last(f"{out}/probe_C96_{v}_{rep}.json")
    b = last(f"{out}/probe_C36B6_{v}_{rep}.json")
    c = last(f"{out}/bench20_{v}_{rep}.json")
    d = last(f"{out}/bench_{v}_{rep}.json")
    ring = (a.get("multi_wave_ring_cycles") or {}).get("int")
    print(f"{v:6s} {rep} C96 multi20/100 {a['multi20_us_per_step']:.3f}/{a['multi100_us_per_step']:.3f}"
          f" | C36B6 multi100 {b['multi100_us_per_step']:.3f}"
          f" | bench 20/5 {c['ms_per_step'] * 1e3:.3f} us | bench {d['ms_per_step'] * 1e3:.3f} us"
          f" | ring arrival by wave (int) {ring}", flush=True)


if __name__ == "__main__":
    main()
