#!/usr/bin/env python3
"""Timing harness of the binned-statistics kernels (pa_stats.hip; the device work of jpdf3d / conditionalMean3d) on the headline
hierarchy: 3 nested levels on an n^3 base (ratio 2, boxes of `box`^3; every level has n^3 cells), fields made on the device.
Per level and launch: jpdf with 2 and with 4 variables at 128 bins, conditionalMean with 4 averaged components at 128 bins, each
for three distributions of the data -- the flame field (most cells burnt or unburnt: a handful of bins), ONE bin (every cell:
all contention) and uniform random (every cell another bin: no run to merge) -- and each with the combined kernel (private runs,
LDS table or LDS cache of hot bins) and the uncombined one (global atomics per cell).  The yardstick is the READ FLOOR: the time of
pa_minmax_comps_level over the same components of the same multifabs, i.e. of streaming them once.  Times: host clock around
synchronous calls, median of `reps` after 2 warm-up calls (the uncombined one-bin case: one call, it takes seconds).
usage: python tools/stats_bench.py [n=512] [box=128] [reps=5]   (prints a table and one JSON line)"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch first: one HIP runtime)

from peleanalysis_amd import capi  # noqa: E402
from peleanalysis_amd.hierarchy import mf_layout, nested_hierarchy  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
box = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
NB = 128
NC = 5  # components per multifab: the bin variable + 4
HBM = 8.0e12

H = nested_hierarchy(n, 3, box, is_per=(0, 0, 0))
dev = torch.device("cuda:0")
ctx = capi.Context(0)


def flame(x, y, z, m):
    """peleanalysis_amd.hierarchy.field_flame in torch"""
    xc, yc, zc = x - 0.5, y - 0.5, z - 0.5
    r = torch.sqrt((xc / 0.30) ** 2 + (yc / 0.15) ** 2 + (zc / 0.18) ** 2)
    theta = torch.atan2(yc, xc)
    rho = torch.sqrt(xc * xc + yc * yc + zc * zc) + 1e-30
    phi = torch.acos(torch.clamp(zc / rho, -1.0, 1.0))
    s = r - 0.03 * torch.sin(6 * theta) * torch.sin(5 * phi)
    return (1.0 + 0.1 * m) * (300.0 + 850.0 * (1.0 + torch.tanh((s - 1.0) / 0.08))) + 3.0 * m * torch.sin(2 * math.pi * (x + 0.37 * m))


def make_level(lv, dist, seed):
    off, cs, total = mf_layout(lv.boxes, NC, 0)
    buf = torch.zeros(total, dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    dx = lv.dx
    for b in range(lv.nboxes):
        lo, hi = lv.boxes[b, :3], lv.boxes[b, 3:]
        nx, ny, nz = (int(hi[d] - lo[d] + 1) for d in range(3))
        for m in range(NC):
            v = buf[int(off[b]) + m * int(cs[b]):int(off[b]) + m * int(cs[b]) + nx * ny * nz].view(nz, ny, nx)
            if dist == "flame":
                x = ((torch.arange(lo[0], hi[0] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[0])[None, None, :]
                y = ((torch.arange(lo[1], hi[1] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[1])[None, :, None]
                z = ((torch.arange(lo[2], hi[2] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[2])[:, None, None]
                v.copy_(flame(x, y, z, m))
            elif dist == "onebin":
                v.copy_(1000.0 + torch.rand((nz, ny, nx), generator=g, device=dev, dtype=torch.float64))
            else:
                v.copy_(300.0 + 1700.0 * torch.rand((nz, ny, nx), generator=g, device=dev, dtype=torch.float64))
    torch.cuda.synchronize()
    return buf


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
    return float(np.median(ts))


dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
vol = [float(np.prod(lv.dx)) for lv in H.levels]
rows, out = [], {"n": n, "box": box, "reps": reps, "cells_per_level": int(H.levels[0].ncells), "cases": []}
for dist in ("flame", "onebin", "random"):
    for l, lv in enumerate(H.levels):
        buf = make_level(lv, dist, 100 + l)
        mf = capi.DevMF(ctx, dls[l], NC, 0, devptr=buf.data_ptr())
        finer = dls[l + 1] if l + 1 < H.nlev else None
        cells = lv.ncells
        lo_ax, hi_ax = (0.0, 4000.0) if dist == "onebin" else (300.0, 2500.0)
        for kname, nread in (("jpdf2", 2), ("jpdf4", 4), ("condmean4", 5)):
            comps = list(range(nread))
            floor = timed(lambda: capi.minmax_comps_level(ctx, mf, comps), reps)
            case = {"dist": dist, "level": l, "kernel": kname, "bytes": cells * nread * 8, "floor_ms": floor * 1e3}
            for unc in (False, True):
                slow = unc and dist != "random"
                if kname.startswith("jpdf"):
                    acc = capi.JpdfAcc(ctx, nread, NB)
                    acc.begin(vol[0], [3000.0] * nread)
                    P = capi.jpdf_params(nread, [lo_ax] * nread, [hi_ax] * nread, uncombined=unc)
                    t = timed(lambda: acc.add_level(mf, finer, 2, vol[l], P), 1 if slow else reps, 0 if slow else 2)
                else:
                    acc = capi.CondMeanAcc(ctx, 4, NB, False)
                    acc.begin(64, [3000.0] * 4)
                    dom = tuple(int(v) for v in lv.domlo) + tuple(int(v) for v in lv.domhi)
                    t = timed(lambda: acc.add_level(mf, finer, 2, dom, 8 ** (H.nlev - 1 - l), lo_ax, hi_ax, uncombined=unc), 1 if slow else reps, 0 if slow else 2)
                acc.read()  # fails loudly on an overflow flag
                acc.close()
                tag = "uncombined" if unc else "combined"
                case[tag + "_ms"] = t * 1e3
                case[tag + "_over_floor"] = t / floor
                case[tag + "_frac_of_8TBs"] = case["bytes"] / t / HBM
            out["cases"].append(case)
            rows.append(case)
        mf.close()
        del buf
        torch.cuda.empty_cache()

print(f"stats_bench: 3 levels x {n}^3 cells, boxes {box}^3, {NB} bins; read floor = pa_minmax_comps_level over the same components")
print(f"{'dist':7s} {'lev':>3s} {'kernel':10s} {'MB read':>8s} {'floor ms':>9s} {'comb ms':>9s} {'x floor':>8s} {'of 8TB/s':>8s} {'uncomb ms':>10s} {'x floor':>9s}")
for c in rows:
    print(f"{c['dist']:7s} {c['level']:3d} {c['kernel']:10s} {c['bytes'] / 1e6:8.0f} {c['floor_ms']:9.3f} {c['combined_ms']:9.3f} {c['combined_over_floor']:8.2f} "
          f"{c['combined_frac_of_8TBs']:8.3f} {c['uncombined_ms']:10.3f} {c['uncombined_over_floor']:9.2f}")
for dist in ("flame", "onebin", "random"):
    for kname in ("jpdf2", "jpdf4", "condmean4"):
        cs_ = [c for c in rows if c["dist"] == dist and c["kernel"] == kname]
        f, a, u = (sum(c[k] for c in cs_) for k in ("floor_ms", "combined_ms", "uncombined_ms"))
        print(f"SUM {dist:7s} {kname:10s} floor {f:9.3f} ms  combined {a:9.3f} ms = {a / f:7.2f} x floor  uncombined {u:10.3f} ms = {u / f:8.2f} x floor")
print(json.dumps(out))
for dl in dls:
    dl.close()
ctx.close()
