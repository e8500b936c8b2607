#!/usr/bin/env python3
"""Where the exact fp32 inference forward (mlp_fwd_kernel<1,false,2>) spends its cycles, section by section, and when
a SIMD's MFMA pipe has no k-loop to run.  Needs a -DFWD_TRACE variant of the library, which stamps (s_memtime, core
clocks) every section boundary of every wave of every workgroup, and records the CU and SIMD each wave ran on:

    SCADE_AB_FLAGS=-DFWD_TRACE SCADE_AB_OUT=tools/scratch/ab_FT python -m scade_amd.build
    SCADE_LIB=tools/scratch/ab_FT/libscade_hip.so python tools/probe_fwd_trace.py --save trace.npz   # on the GPU
    python tools/probe_fwd_trace.py --analyse trace.npz                                                 # anywhere

One headline render step (bench.py's: 1024 rays x (64 + 128) samples) is traced after warm-up: the coarse launch
(1,024 workgroups, two rounds over 256 CUs x 2) and the fine launch (3,072, six rounds).

Per section: mean cycles per wave.  Pipe idle: on every SIMD, the cycles between the first and the last stamp of the
launch on that CU in which NEITHER resident wave is inside a k-loop, split by what the waves were doing instead (the
section each one was in; "-" = no wave resident).  Stalls inside a k-loop (vmcnt, lgkmcnt, VALU) are not in this
split: the PMC pass (SQ_WAIT_*, SQ_INSTS_*) covers those."""
import argparse
import collections
import ctypes
import os
import sys

import numpy as np

FT_N, FT_WG = 64, 3072
LAYERS = ["l0", "l1", "l2", "l3", "l4", "l5", "l6", "l7", "feat", "views"]
PHASES = ["k-loop", "barrier 1", "epilogue", "copy", "barrier 2"]


def capture(out):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import bench
    import scade_amd as S
    from scade_amd import _lib
    from scade_amd.synthetic import synthetic_rays
    dev = torch.device("cuda:0")
    _, _, coarse, fine = bench.make_nets(dev)
    e, _ = S.get_embedder(9, 0)
    ed, _ = S.get_embedder(0, 0)
    query = S.make_network_query_fn(e, ed, torch.zeros(3, device=dev), torch.tensor(0.2, device=dev))
    rays = synthetic_rays(1024, seed=1000).to(dev)

    def step():
        with torch.no_grad():
            S.render_rays(rays, True, coarse, query, bench.N_COARSE, N_importance=bench.N_FINE, network_fine=fine,
                          perturb=0., raw_noise_std=0.)
    lib = _lib.load()
    if not hasattr(lib, "scade_debug_fwd_trace"):
        sys.exit("this library was not built with -DFWD_TRACE (see the docstring)")
    for _ in range(20):
        step()
    torch.cuda.synchronize()
    assert lib.scade_debug_fwd_trace_clear() == 0
    step()
    torch.cuda.synchronize()
    st = np.zeros(2 * FT_WG * 4 * FT_N, dtype=np.uint64)
    hw = np.zeros(2 * FT_WG * 4 * 2, dtype=np.uint32)
    lib.scade_debug_fwd_trace.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.scade_debug_fwd_trace(st.ctypes.data, hw.ctypes.data) == 0
    np.savez_compressed(out, stamps=st.reshape(2, FT_WG, 4, FT_N), hwid=hw.reshape(2, FT_WG, 4, 2))
    print(f"wrote {out}")


def section_of(t, w, c):
    """name of the section wave row t[w] is in at cycle c (None outside the kernel)"""
    r = t[w]
    if c < r[0] or c >= r[62]:
        return None
    if c < r[1]:
        return "prologue"
    if c < r[2]:
        return "load_bias/l0 lead-in"
    for l in range(10):
        b = 2 + 6 * l
        for i in range(5):
            if c < r[b + i + 1]:
                return f"{PHASES[i]}"
        nxt = r[2 + 6 * (l + 1)] if l < 9 else r[62]
        if c < nxt:
            return {5: "view pad", 7: "alpha head", 9: "rgb head"}.get(l, "between layers")
    return "rgb head"


def analyse(path):
    d = np.load(path)
    stamps, hwid = d["stamps"].astype(np.int64), d["hwid"]
    for cls, (name, nwg) in enumerate((("coarse launch (1,024 workgroups)", 1024), ("fine launch (3,072 workgroups)", 3072))):
        t = stamps[cls, :nwg]
        h = hwid[cls, :nwg]
        if not (t[:, :, 62] > 0).all():
            print(f"{name}: incomplete trace"); continue
        print(f"== {name}")
        dur = t[:, :, 62] - t[:, :, 0]
        print(f"   workgroup life: mean {dur.mean():.0f} cycles (min {dur.min()} max {dur.max()})")
        rows = [("prologue", t[..., 1] - t[..., 0]), ("bias + first loads", t[..., 2] - t[..., 1])]
        for i, ph in enumerate(PHASES):
            rows.append((ph + " (sum of 10 layers)", sum(t[..., 2 + 6 * l + i + 1] - t[..., 2 + 6 * l + i] for l in range(10))))
        rows.append(("view pad (after l5)", t[..., 2 + 36] - t[..., 2 + 35]))
        rows.append(("alpha head (after l7)", t[..., 2 + 48] - t[..., 2 + 47]))
        rows.append(("between other layers", sum(t[..., 2 + 6 * (l + 1)] - t[..., 2 + 6 * l + 5] for l in (0, 1, 2, 3, 4, 6, 8))))
        rows.append(("rgb head", t[..., 62] - t[..., 2 + 59]))
        tot = dur.mean()
        print(f"   {'section':34s} {'cycles/wave':>12s} {'share':>7s}")
        for n, v in rows:
            print(f"   {n:34s} {v.mean():12.0f} {v.mean() / tot:7.3f}")
        kl = t[..., 2 + 6 * np.arange(10)[:, None] + np.array([0, 1])]          # [wg][wave][layer][start,end]
        # per layer: k-loop skew across the four waves of a workgroup at barrier 1 (last arrival - first)
        arr = t[..., 2 + 6 * np.arange(10) + 1]
        print(f"   barrier-1 arrival skew inside a workgroup: mean {(arr.max(1) - arr.min(1)).mean():.0f} cycles per layer")
        # pipe idle per SIMD
        simd = (h[..., 0] >> 4) & 3
        cu = ((h[..., 1] & 15).astype(np.int64) << 16) | (((h[..., 0] >> 13) & 7) << 8) | (((h[..., 0] >> 12) & 1) << 4) | ((h[..., 0] >> 8) & 15)
        groups = collections.defaultdict(list)
        for g in range(nwg):
            for w in range(4):
                groups[(int(cu[g, w]), int(simd[g, w]))].append((g, w))
        idle = collections.Counter()
        span_total = 0
        cu_span = {}
        for (c, s), members in groups.items():
            cu_span.setdefault(c, [])
            cu_span[c] += members
        for (c, s), members in groups.items():
            allm = cu_span[c]
            lo = min(t[g, w, 0] for g, w in allm)
            hi = max(t[g, w, 62] for g, w in allm)
            span_total += hi - lo
            ev = []
            for g, w in members:
                for l in range(10):
                    ev.append((kl[g, w, l, 0], 1)); ev.append((kl[g, w, l, 1], -1))
            bounds = sorted(set([lo, hi] + [e[0] for e in ev] + [t[g, w, k] for g, w in members for k in list(range(62)) + [62]]))
            busy_iv = sorted((kl[g, w, l, 0], kl[g, w, l, 1]) for g, w in members for l in range(10))
            # coverage by k-loops: sweep
            for a, b in zip(bounds[:-1], bounds[1:]):
                if b <= a or a < lo or b > hi:
                    continue
                m = (a + b) / 2
                if any(s0 <= m < s1 for s0, s1 in busy_iv):
                    continue
                labs = sorted(x for x in (section_of(t[g], w, m) for g, w in members) if x is not None)
                idle[" + ".join(labs) if labs else "-"] += b - a
        tot_idle = sum(idle.values())
        print(f"   SIMD-cycles with no wave in a k-loop: {tot_idle / span_total:.4f} of {len(groups)} SIMDs' spans")
        for k, v in idle.most_common(14):
            print(f"      {v / span_total:7.4f}  {k}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--save", metavar="NPZ")
    ap.add_argument("--analyse", metavar="NPZ")
    a = ap.parse_args()
    if a.save:
        capture(a.save)
    if a.analyse:
        analyse(a.analyse)
