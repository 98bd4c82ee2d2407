#!/usr/bin/env python3
"""Timing harness of the surface-PDF kernels (pa_binmef.hip; the device work of binMEF3d) on three inputs:
  (1) the marching-cubes surface of the flame field at n^3 (iso 1150), binned 64 x 64 on two fields that vary along it;
  (2) the same surface binned on the iso field itself -- every leaf lands in ONE bin (the contention case of DESIGN.md 3.7) -- with the
      combined accumulation and with `uncombined` (one set of global atomics per leaf);
  (3) the coarse lat-long sphere n4 of tests/binmef_ref.py (64 elements) at 128 x 128 bins: O(s^2) fan-out per triangle; with the
      default list and with work_items = 2^15, where most rounds take a slice.
pa_surfbin_add_surface is a SYNCHRONOUS call that uploads the node components and the elements, loops over the rounds (count kernel ->
counts to the host -> offsets to the device -> emit kernel) and returns when the surface has been binned; the time is the host clock
around that call: min / median / max of `reps` calls after 2 warm-up calls.  Rates: input triangles / s and leaves / s (leaves =
NmyTriangles, the in-range leaves the call added).  FLOOR, timed in the same process: one streaming read of the uploaded arrays (the
node components as doubles + the elements as int32) by a torch reduction over a buffer of that many bytes, after a warm-up, device
synchronised.  For (3) the input is 64 triangles: the floor is a launch, and the figure that matters is leaves / s.
usage: python tools/binmef_bench.py [n=256] [reps=7]   (prints a table and one JSON line)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (torch first: one HIP runtime)

import binmef_ref as B  # noqa: E402
from peleanalysis_amd import capi  # noqa: E402
from peleanalysis_amd.hierarchy import mf_layout, nested_hierarchy  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 7
box = min(128, n)
dev = torch.device("cuda:0")
ctx = capi.Context(0)


def flame(x, y, z):
    """peleanalysis_amd.hierarchy.field_flame (m = 0) in torch"""
    xc, yc, zc = x - 0.5, y - 0.5, z - 0.5
    r = torch.sqrt((xc / 0.30) ** 2 + (yc / 0.15) ** 2 + (zc / 0.18) ** 2)
    theta = torch.atan2(yc, xc)
    rho = torch.sqrt(xc * xc + yc * yc + zc * zc) + 1e-30
    phi = torch.acos(torch.clamp(zc / rho, -1.0, 1.0))
    s = r - 0.03 * torch.sin(6 * theta) * torch.sin(5 * phi)
    return 300.0 + 850.0 * (1.0 + torch.tanh((s - 1.0) / 0.08)) + 0.0 * x


def mc_surface():
    """one level of n^3 cells in boxes of 128^3 with one ghost layer: X Y Z, the flame field and two fields that vary along its
    isosurface, made on the device; marching cubes at 1150 -> (nodes [N][6], elts [M][3] 1-based), the FABs' pieces side by side"""
    lv = nested_hierarchy(n, 1, box, is_per=(0, 0, 0)).levels[0]
    dl = capi.DevLevel(ctx, lv)
    off, cs, tot = mf_layout(lv.boxes, 6, 1)
    t = torch.empty(tot, dtype=torch.float64, device=dev)
    for b in range(lv.nboxes):
        lo = lv.boxes[b, :3] - 1
        g = [int(lv.boxes[b, 3 + d] - lv.boxes[b, d] + 3) for d in range(3)]
        xs = [(torch.arange(int(lo[d]), int(lo[d]) + g[d], device=dev, dtype=torch.float64) + 0.5) / n for d in range(3)]
        shp = (g[2], g[1], g[0])
        X, Y, Z = xs[0][None, None, :].expand(shp), xs[1][None, :, None].expand(shp), xs[2][:, None, None].expand(shp)
        f1 = 300.0 + 1700.0 * (0.5 + 0.5 * torch.tanh(6.0 * (Z - 0.5) + 2.8 * (X - 0.5) * (Y - 0.5)))
        f2 = torch.sin(10.0 * X) * torch.cos(6.0 * Y) + 0.4 * (Z - 0.5)
        for c, v in enumerate((X, Y, Z, flame(X, Y, Z), f1, f2)):
            t[int(off[b]) + c * int(cs[b]): int(off[b]) + c * int(cs[b]) + g[0] * g[1] * g[2]] = v.reshape(-1)
    torch.cuda.synchronize()
    st = capi.DevMF(ctx, dl, 6, 1, t.data_ptr())
    loops = np.zeros((lv.nboxes, 6), np.int64)
    for b in range(lv.nboxes):
        loops[b, :3] = np.maximum(lv.boxes[b, :3] - 1, 0)
        loops[b, 3:] = np.minimum(lv.boxes[b, 3:] + 1, n - 1) - 1
    frags = capi.mc_level(ctx, st, None, loops, 3, 1150.0)
    nodes, elts, base = [], [], 0
    for v, k, tri in frags:
        nodes.append(v)
        elts.append(tri.astype(np.int64) + base + 1)
        base += len(v)
    st.close()
    dl.close()
    return np.ascontiguousarray(np.concatenate(nodes)), np.concatenate(elts).astype(np.int32)


def timed(fn, nrep, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(nrep):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return [min(ts) * 1e3, float(np.median(ts)) * 1e3, max(ts) * 1e3]


def floor_ms(nbytes):
    """one streaming read of nbytes on the device (torch.sum over int64 words)"""
    buf = torch.ones(max(nbytes // 8, 1), dtype=torch.int64, device=dev)
    ts = []
    for i in range(2 + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        buf.sum()
        torch.cuda.synchronize()
        if i >= 2:
            ts.append(time.perf_counter() - t0)
    return [min(ts) * 1e3, float(np.median(ts)) * 1e3, max(ts) * 1e3]


def case(name, nodes, elts, bc, mn, mx, nb, uncombined=False, work_items=0):
    with capi.SurfBin(ctx, nb, mn, mx, work_items) as sb:
        amax = sb.max_area(nodes, elts)

        def run():
            sb.begin(amax)
            sb.add_surface(nodes, elts, bc, uncombined=uncombined)
        t = timed(run, reps)
        area, hits, tot, outside, cnt = sb.read()
    nbytes = (3 + len(bc)) * len(nodes) * 8 + elts.size * 4
    fl = floor_ms(nbytes)
    return {"case": name, "elements": int(len(elts)), "nodes": int(len(nodes)), "bins": list(nb), "uncombined": int(uncombined), "leaves": cnt["n_my"],
            "nonempty": int((hits > 0).sum()), "max_hits": int(hits.max()), "rounds": cnt["rounds"], "peak": cnt["peak"], "sliced": cnt["sliced"], "items": cnt["items"],
            "capacity": cnt["capacity"], "ms": t, "uploaded_bytes": nbytes, "floor_ms": fl, "tri_per_s": len(elts) / (t[1] * 1e-3),
            "leaves_per_s": cnt["n_my"] / (t[1] * 1e-3), "over_floor": t[1] / fl[1], "bin_sum": float(area.sum()), "total_area": tot}


nodes, elts = mc_surface()
out = {"n": n, "reps": reps, "cases": []}
mn = (float(nodes[:, 4].min()), float(nodes[:, 5].min()))
mx = (float(nodes[:, 4].max()), float(nodes[:, 5].max()))
out["cases"].append(case("mc_64x64", nodes, elts, (4, 5), mn, mx, (64, 64)))
out["cases"].append(case("mc_iso_onebin", nodes, elts, (3,), (1000.0,), (1300.0,), (3,)))
out["cases"].append(case("mc_iso_onebin", nodes, elts, (3,), (1000.0,), (1300.0,), (3,), uncombined=True))
sn, se = B.latlong_sphere(4)
out["cases"].append(case("n4_128x128", sn, se, (3, 4), (350.0, -0.9), (1950.0, 0.9), (128, 128)))
out["cases"].append(case("n4_128x128", sn, se, (3, 4), (350.0, -0.9), (1950.0, 0.9), (128, 128), work_items=1 << 15))

print(f"binmef_bench: flame isosurface at {n}^3 ({len(elts)} triangles, {len(nodes)} nodes) and the n4 sphere; ms of one pa_surfbin_add_surface call "
      f"(upload + rounds), min/median/max of {reps} calls after 2 warm-up calls; floor = one streaming read of the uploaded bytes")
print(f"{'case':>14s} {'unc':>3s} {'capacity':>8s} {'elements':>8s} {'leaves':>8s} {'bins>0':>6s} {'maxhit':>7s} {'rounds':>6s} {'peak':>7s} {'sliced':>6s} {'ms':>24s} "
      f"{'floor ms':>21s} {'Mtri/s':>8s} {'Mleaf/s':>8s} {'x floor':>8s}")
f3 = lambda t: "/".join(f"{v:.3f}" for v in t)
for c in out["cases"]:
    print(f"{c['case']:>14s} {c['uncombined']:3d} {c['capacity']:8d} {c['elements']:8d} {c['leaves']:8d} {c['nonempty']:6d} {c['max_hits']:7d} {c['rounds']:6d} {c['peak']:7d} {c['sliced']:6d} "
          f"{f3(c['ms']):>24s} {f3(c['floor_ms']):>21s} {c['tri_per_s'] / 1e6:8.3f} {c['leaves_per_s'] / 1e6:8.3f} {c['over_floor']:8.1f}")
print(json.dumps(out))
ctx.close()
