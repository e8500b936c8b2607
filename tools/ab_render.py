#!/usr/bin/env python3
"""Interleaved A/B of two (or more) builds of libscade_hip.so on the headline render step (tools/probe_render.py: the
step bench.py times): every variant runs as its own process (the library is chosen at load time: SCADE_LIB), in
ALTERNATING order, ``--reps`` times each (at least 7); median and spread of the ms / step.  The render-step
counterpart of tools/ab_step.py.

    SCADE_AB_FLAGS=-DX SCADE_AB_OUT=tools/scratch/ab_X python -m scade_amd.build
    python tools/ab_render.py intree tools/scratch/ab_X/libscade_hip.so [--reps 7] [--steps 40]"""
import argparse
import os
import re
import subprocess
import sys

here = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+", help='"intree" (the in-tree build) or a path to a libscade_hip.so')
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--timeout", type=float, default=300.0, help="seconds per process")
args = ap.parse_args()
if args.reps < 7:
    ap.error("--reps: at least 7 runs per build")
res = {l: [] for l in args.libs}
for _ in range(args.reps):
    for l in args.libs:
        env = dict(os.environ)
        if l != "intree":
            env["SCADE_LIB"] = os.path.abspath(l)
        else:
            env.pop("SCADE_LIB", None)
        cmd = [sys.executable, os.path.join(here, "probe_render.py"), "--steps", str(args.steps)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.timeout)
        m = re.search(r"([0-9.]+) ms / step", r.stdout)
        if r.returncode != 0 or not m:     # a failed run ends the comparison: nothing more is started
            sys.exit(f"{l}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        res[l].append(float(m.group(1)))
for l, v in res.items():
    v = sorted(v)
    print(f"{l:48s} median {v[len(v) // 2]:.4f} ms  min {v[0]:.4f}  max {v[-1]:.4f}  ({len(v)} runs)")
