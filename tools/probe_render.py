#!/usr/bin/env python3
"""The headline step of bench.py on its own: render_rays forward (no_grad, perturb=0, f32) of 1024 synthetic rays x
(64 coarse + 128 fine), the same nets and rays as bench.py's rank 0; 12 set-up + ``--warmup`` steps, then ``--steps``
timed ones ending in a device synchronise.  Prints "<ms> ms / step".  The command behind tools/ab_render.py."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--rays", type=int, default=1024)
args = ap.parse_args()

import bench
import scade_amd as S
from scade_amd.synthetic import synthetic_rays

dev = torch.device("cuda:0")
_, _, coarse, fine = bench.make_nets(dev)
e, _ = S.get_embedder(9, 0)
ed, _ = S.get_embedder(0, 0)
query = S.make_network_query_fn(e, ed, torch.zeros(3, device=dev), torch.tensor(0.2, device=dev))
rays = synthetic_rays(args.rays, seed=1000).to(dev)


def step():
    with torch.no_grad():
        return S.render_rays(rays, True, coarse, query, bench.N_COARSE, N_importance=bench.N_FINE,
                             network_fine=fine, perturb=0., raw_noise_std=0.)


for _ in range(12 + args.warmup):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.steps):
    ret = step()
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / args.steps * 1e3
assert bool(torch.isfinite(ret["rgb_map"]).all())
print(f"render {args.rays} rays: {ms:.4f} ms / step")
