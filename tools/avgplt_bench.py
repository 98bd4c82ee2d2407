#!/usr/bin/env python3
"""Timing harness of the resampling kernel (pa_resample.hip; the device work of avgPlotfiles3d): three files of the headline
hierarchy -- 3 nested levels on an n^3 base, ratio 2, boxes of `box`^3, every level n^3 cells -- whose refined regions are
shifted from file to file (file f: level 1 by f * (64, 32, 0) of its cells, level 2 by twice that + f * 64 in x), `nvar`
components, interp_type 1, the flame field made on the device with a per-file phase.  The output levels are what the tool builds:
level 0 as in the files, the union levels as a disjoint cover chopped to `grid` cells.

Per file and level: the time of the ONE launch pa_resample_add_file_level makes (resample + add, fused), the share of the level's
output cells that were interpolated (not held by the file's level), and the ratio to the FLOOR, timed in the same process:
pa_mf_copy of 3 nvar / 2 components between two multifabs on the same output level = exactly the bytes a file-level pass must
move at least -- read the file's value of every output cell once, read and write the running sum.  (The work multifab T_l a
coarser level also writes, and the coarse values an interpolated parent reads, come on top and are not in the floor.)
A last block repeats level 1 and 2 of file 0 on the file's OWN BoxArray: the fully-present path, no cell interpolated.
Times: host clock around a call + synchronise; min / median / max of `reps` calls after 2 warm-up calls.
usage: python tools/avgplt_bench.py [n=512] [box=128] [reps=7] [grid=32] [nvar=4]   (prints a table and one JSON line)"""
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
from peleanalysis_amd.hierarchy import Level, chop_box, disjoint_cover, mf_layout  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 512
box = int(sys.argv[2]) if len(sys.argv) > 2 else 128
reps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 7
grid = int(sys.argv[4]) if len(sys.argv) > 4 else 32
NV = int(sys.argv[5]) if len(sys.argv) > 5 else 4
NF, NLEV, RATIO, INTERP = 3, 3, 2, 1
IS_PER = (1, 1, 0)
assert n % 8 == 0 and NV % 2 == 0

dev = torch.device("cuda:0")
ctx = capi.Context(0)


def level(boxes, l):
    m = n * RATIO ** l
    return Level(boxes, (0, 0, 0), (m - 1,) * 3, IS_PER, np.zeros(3), np.ones(3))


def file_levels(f):
    """level 1 = the central half-width cube shifted by f * (n/8, n/16, 0); level 2 = the central half of level 1 shifted on"""
    s1 = np.array([f * (n // 8), f * (n // 16), 0])
    lo1 = np.full(3, n // 2) + s1
    hi1 = lo1 + n - 1
    lo2 = 2 * lo1 + n // 2 + np.array([f * (n // 8), 0, 0])
    hi2 = lo2 + n - 1
    return [level(chop_box((0, 0, 0), (n - 1,) * 3, box), 0), level(chop_box(lo1, hi1, box), 1), level(chop_box(lo2, hi2, box), 2)]


def flame(x, y, z, m):
    """peleanalysis_amd.hierarchy.field_flame in torch"""
    xc, yc, zc = x - 0.5, y - 0.5, z - 0.5
    r = torch.sqrt((xc / 0.30) ** 2 + (yc / 0.15) ** 2 + (zc / 0.18) ** 2)
    theta = torch.atan2(yc, xc)
    rho = torch.sqrt(xc * xc + yc * yc + zc * zc) + 1e-30
    phi = torch.acos(torch.clamp(zc / rho, -1.0, 1.0))
    s = r - 0.03 * torch.sin(6 * theta) * torch.sin(5 * phi)
    return (1.0 + 0.1 * m) * (300.0 + 850.0 * (1.0 + torch.tanh((s - 1.0) / 0.08))) + 3.0 * m * torch.sin(2 * math.pi * (x + 0.37 * m))


def make_level(lv, phase):
    off, cs, total = mf_layout(lv.boxes, NV, 0)
    buf = torch.zeros(total, dtype=torch.float64, device=dev)
    dx = lv.dx
    for b in range(lv.nboxes):
        lo, hi = lv.boxes[b, :3], lv.boxes[b, 3:]
        nx, ny, nz = (int(hi[d] - lo[d] + 1) for d in range(3))
        x = ((torch.arange(lo[0], hi[0] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[0])[None, None, :]
        y = ((torch.arange(lo[1], hi[1] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[1])[None, :, None]
        z = ((torch.arange(lo[2], hi[2] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[2])[:, None, None]
        for m in range(NV):
            buf[int(off[b]) + m * int(cs[b]):int(off[b]) + m * int(cs[b]) + nx * ny * nz].view(nz, ny, nx).copy_(flame(x, y, z, m + 2 * phase))
    torch.cuda.synchronize()
    return buf


def timed(fn, nrep, warm=2):
    for _ in range(warm):
        fn()
    ctx.sync()
    ts = []
    for _ in range(nrep):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
    return [min(ts) * 1e3, float(np.median(ts)) * 1e3, max(ts) * 1e3]


def overlap_cells(a, b):
    """cells that a box of list a and a box of list b share (both lists disjoint)"""
    a, b = a.astype(np.int64), b.astype(np.int64)
    tot = 0
    for row in a:
        w = np.minimum(row[3:], b[:, 3:]) - np.maximum(row[:3], b[:, :3]) + 1
        tot += int(np.prod(np.maximum(w, 0), axis=1).sum())
    return tot


def run(files, out_levels, tag, only_file=None, out=None):
    """every file and level through pa_resample_add_file_level on the given output levels; one row per (file, level)"""
    dls = [capi.DevLevel(ctx, lv) for lv in out_levels]
    ghosts = [capi.Resample.ghosts(NLEV, l, [RATIO] * (NLEV - 1), INTERP) for l in range(NLEV)]
    runm = [capi.DevMF(ctx, dl, NV, 0) for dl in dls]
    work = [capi.DevMF(ctx, dls[l], NV, ghosts[l]) if l < NLEV - 1 else None for l in range(NLEV)]
    floors = []
    for l in range(NLEV):  # the floor: 3 NV / 2 components copied = 3 NV components of the level moved
        a, b = capi.DevMF(ctx, dls[l], 3 * NV // 2, 0), capi.DevMF(ctx, dls[l], 3 * NV // 2, 0)
        a.setval(1.0)
        floors.append(timed(lambda: ctx.check(ctx.lib.pa_mf_copy(ctx.h, a.h, 0, b.h, 0, 3 * NV // 2, 0)), reps))
        a.close()
        b.close()
    rs = capi.Resample(ctx)
    rs.begin(runm, NV)
    rows = []
    for f, levs in enumerate(files):
        if only_file is not None and f != only_file:
            continue
        for l, flv in enumerate(levs):
            buf = make_level(flv, f)
            fdl = capi.DevLevel(ctx, flv)
            fm = capi.DevMF(ctx, fdl, NV, 0, devptr=buf.data_ptr())
            fn = lambda: rs.add_file_level(l, fm, list(range(NV)), work[l - 1] if l else None, RATIO, INTERP, work[l])
            t = timed(fn, reps)
            cells = out_levels[l].ncells
            held = overlap_cells(out_levels[l].boxes, flv.boxes)
            row = {"tag": tag, "file": f, "level": l, "out_boxes": out_levels[l].nboxes, "out_cells": cells, "interpolated": 1.0 - held / cells,
                   "ghosts": ghosts[l], "ms": t, "floor_ms": floors[l], "over_floor": t[1] / floors[l][1], "floor_bytes": 3 * NV * 8 * cells,
                   "floor_TBs": 3 * NV * 8 * cells / (floors[l][1] * 1e-3) / 1e12}
            rows.append(row)
            fm.close()
            fdl.close()
            del buf
            torch.cuda.empty_cache()
    nosrc = rs.finish(NF)
    rs.close()
    for m in runm + [w for w in work if w is not None]:
        m.close()
    for dl in dls:
        dl.close()
    if out is not None:
        out["nosrc_" + tag] = nosrc
    return rows


files = [file_levels(f) for f in range(NF)]
union = [files[0][0]] + [level(disjoint_cover(np.vstack([fl[l].boxes for fl in files]), grid), l) for l in (1, 2)]
out = {"n": n, "box": box, "reps": reps, "grid": grid, "nvar": NV, "nfiles": NF, "interp_type": INTERP}
rows = run(files, union, "union", out=out)
rows += run(files, files[0], "own", only_file=0, out=out)
out["rows"] = rows

print(f"avgplt_bench: {NF} files x {NLEV} levels x {n}^3 cells, file boxes {box}^3, union levels chopped to {grid}, {NV} components, interp_type {INTERP};"
      f" ms as min/median/max of {reps} calls after 2 warm-up calls")
print("floor = pa_mf_copy of 3 nvar / 2 components on the output level (read the file's cells once + read and write the running sum)")
print(f"{'grids':>5s} {'file':>4s} {'lev':>3s} {'boxes':>6s} {'Mcells':>7s} {'interp':>6s} {'ng':>2s} {'resample+add ms':>21s} {'floor ms':>21s} {'x floor':>7s} {'floor TB/s':>10s}")
f3 = lambda t: "/".join(f"{v:.3f}" for v in t)
for r in rows:
    print(f"{r['tag']:>5s} {r['file']:4d} {r['level']:3d} {r['out_boxes']:6d} {r['out_cells'] / 1e6:7.1f} {r['interpolated']:6.3f} {r['ghosts']:2d} {f3(r['ms']):>21s} "
          f"{f3(r['floor_ms']):>21s} {r['over_floor']:7.2f} {r['floor_TBs']:10.2f}")
print("cells without source data:", {k: v for k, v in out.items() if k.startswith("nosrc_")})
print(json.dumps(out))
ctx.close()
