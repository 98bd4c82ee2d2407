#!/usr/bin/env python3
"""Timing harness of the surface smoothing step (pa_surfsmooth.hip; smoothMEF3d) on the lines of the other tools/*_bench.py.  The
input is synthetic: an n x n grid patch with a smooth bump in z, two triangles per cell (n = 1024: 1,050,625 nodes and 2,097,152
triangles), 5 node components, the triangles' own areas as weights.  Two element orders: cell by cell (the locality of marching-cubes
output) and a seeded random permutation (none).
Timed with a host clock around pa_surfsmooth_run, which is synchronous (it ends in a stream synchronise): the call with nSmooth = 0 (the
incidence sort, the neighbour lists, the two averagings) and with nSmooth = K; the time per iteration is their difference over K.
One warm-up call of each, then `reps` of each, alternating; median, minimum and maximum are reported.  The bytes an iteration must
move are counted from the neighbour lists of the run and give the bandwidth the time implies.  No gate: nobody
had measured this kernel before.
usage: python tools/surfsmooth_bench.py [n=1024] [K=200] [reps=5] [out=profiles/surfsmooth_bench.json] [kernels]
`kernels`: one call with nSmooth = 20 per order only, for rocprofv3 --kernel-trace --stats -- python3 ...: profiles/surfsmooth_kernel_stats.txt."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (torch first: one HIP runtime)

from peleanalysis_amd import capi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
K = int(sys.argv[2]) if len(sys.argv) > 2 else 200
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
out_json = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "surfsmooth_bench.json")
kernels_only = len(sys.argv) > 5 and sys.argv[5] == "kernels"
NC = 5

jj, ii = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
x, y = ii.ravel() / n, jj.ravel() / n
rng = np.random.default_rng(1)
nodes = np.ascontiguousarray(np.stack([x, y, 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)] + [rng.uniform(-1, 1, len(x)) for _ in range(NC - 3)], axis=1))
j, i = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
p = (j * (n + 1) + i).ravel()
cells = np.stack([np.stack([p, p + 1, p + n + 2], 1), np.stack([p, p + n + 2, p + n + 1], 1)], axis=1).reshape(-1, 3) + 1  # the two triangles of a cell side by side
orders = {"cell by cell": np.ascontiguousarray(cells.astype(np.int32)), "random": np.ascontiguousarray(cells[rng.permutation(len(cells))].astype(np.int32))}
print(f"{n} x {n} grid patch: {len(nodes)} nodes, {len(cells)} triangles, {NC} components")
ctx = capi.Context(0)


def smooth_once(e, nsmooth, read=False):
    with capi.Surf(ctx, nodes, e) as s:
        ctx.sync()
        t0 = time.perf_counter()
        s.smooth(3, -1, nsmooth)
        dt = 1e3 * (time.perf_counter() - t0)
        return dt, s.last_launch(), (s.read()[0][:, 3].copy() if read else None)


res = {"surface": f"{n} x {n} grid patch", "nodes": len(nodes), "triangles": len(cells), "ncomp": NC, "K": K, "reps": reps,
       "timing": "host clock around the synchronous call, ms; median [min, max] of reps after a warm-up call, nSmooth = 0 and K alternating", "runs": []}
fields = []
for label, e in orders.items():
    if kernels_only:
        smooth_once(e, 20)
        continue
    _, rec, f = smooth_once(e, K, True)
    fields.append(f)
    smooth_once(e, 0)
    t0, tk = [], []
    for _ in range(reps):
        t0.append(smooth_once(e, 0)[0])
        tk.append(smooth_once(e, K)[0])
    ne, na = rec["elements"], rec["neighbours"]
    # per element and iteration: the two offsets of its list (4 B streamed: off[e + 1] is the next element's off[e]), its index entries
    # (4 B each), W, w and q of the element itself and the store of q' (8 B each); the gathers of w_nb and q_nb are counted once per
    # element as the streams of w and q above -- every further touch of them is a hit in L2 where the order has locality
    must = ne * (4 + 8 + 8 + 8 + 8) + na * 4
    gathered = na * 16
    per_it = [(b - a) / K for a, b in zip(t0, tk)]
    row = {"order": label, "neighbours": na, "max_neighbours": rec["max_neighbours"], "kernels": rec["kernels"],
           "setup_ms": {"median": statistics.median(t0), "min": min(t0), "max": max(t0), "all": t0},
           "call_K_ms": {"median": statistics.median(tk), "min": min(tk), "max": max(tk), "all": tk},
           "iteration_us": {"median": 1e3 * statistics.median(per_it), "min": 1e3 * min(per_it), "max": 1e3 * max(per_it)},
           "bytes_must_move": must, "bytes_gathered_through_L2": gathered}
    row["implied_GBps_of_must_move"] = must / (1e-3 * statistics.median(per_it)) / 1e9
    res["runs"].append(row)
    print(f"{label}: {na / ne:.2f} neighbours per element; nSmooth = 0 call {row['setup_ms']['median']:.3f} ms; iteration {row['iteration_us']['median']:.1f} us "
          f"[{row['iteration_us']['min']:.1f}, {row['iteration_us']['max']:.1f}]; {must / 1e6:.1f} MB must move -> {row['implied_GBps_of_must_move']:.0f} GB/s; "
          f"{gathered / 1e6:.1f} MB gathered through L2")
ctx.close()
if kernels_only:
    sys.exit(0)
# the two orders smooth the same surface: the node field agrees up to the order of the additions
res["orders_agree_to"] = float(np.abs(fields[0] - fields[1]).max())
os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
with open(out_json, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
