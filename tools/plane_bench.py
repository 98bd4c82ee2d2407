#!/usr/bin/env python3
"""Timing harness of the plane kernels (pa_plane.hip; the device work of avgToPlane3d and slicePlot3d) on the headline hierarchy as
bench.py builds it: nested_hierarchy(n, 3, box, is_per=(1, 1, 0)) -- 3 nested levels on an n^3 base, ratio 2, every level n^3 cells in
boxes of `box`^3 -- the flame field made on the device.  The sub-box is the finest level's domain ((4 n)^3 fine cells: a plane of
(4 n)^2 pixels), max_grid_size 32.

Per dir and for 1 and 4 components: pa_plane_run timed as `reps` back-to-back calls after one warm-up call, ended by one synchronise
(host clock; per-call time = the window / reps), three windows, min / median / max.  FLOOR = every UNCOVERED cell of the sub-box read
once -- level l's cells minus the cells under level l + 1, 8 bytes per component -- at the rate a streaming read reaches in the same
process (pa_minmax_comps_level over the finest level's components, which reads every cell once) and, beside it, at 8 TB/s (the
figure DESIGN.md 5 states its shares against).  Also timed: the slice per dir (1 component), min / max and pixelize of a plane.
usage: python tools/plane_bench.py [n=512] [box=128] [reps=8]   (prints a table and one JSON line)"""
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
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 8
NV, MGS, WINDOWS = 4, 32, 3

dev = torch.device("cuda:0")
ctx = capi.Context(0)
H = nested_hierarchy(n, 3, box, is_per=(1, 1, 0))


def flame(x, y, z, m):
    """peleanalysis_amd.hierarchy.field_flame in torch"""
    xc, yc, zc = x - 0.5, y - 0.5, z - 0.5
    r = torch.sqrt((xc / 0.30) ** 2 + (yc / 0.15) ** 2 + (zc / 0.18) ** 2)
    theta = torch.atan2(yc, xc)
    rho = torch.sqrt(xc * xc + yc * yc + zc * zc) + 1e-30
    phi = torch.acos(torch.clamp(zc / rho, -1.0, 1.0))
    s = r - 0.03 * torch.sin(6 * theta) * torch.sin(5 * phi)
    return (1.0 + 0.1 * m) * (300.0 + 850.0 * (1.0 + torch.tanh((s - 1.0) / 0.08))) + 3.0 * m * torch.sin(2 * math.pi * (x + 0.37 * m))


def make_level(lv):
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
            buf[int(off[b]) + m * int(cs[b]):int(off[b]) + m * int(cs[b]) + nx * ny * nz].view(nz, ny, nx).copy_(flame(x, y, z, m))
    torch.cuda.synchronize()
    return buf


def timed(fn):
    """per-call ms of `reps` back-to-back calls ended by one synchronise: [min, median, max] over WINDOWS windows"""
    fn()
    ctx.sync()
    ts = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        ts.append((time.perf_counter() - t0) / reps * 1e3)
    return [min(ts), float(np.median(ts)), max(ts)]


bufs = [make_level(lv) for lv in H.levels]
dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
mfs = [capi.DevMF(ctx, dl, NV, 0, devptr=b.data_ptr()) for dl, b in zip(dls, bufs)]
ratios = [H.ref_ratio] * (H.nlev - 1)
fine = H.levels[-1]
dom = tuple(int(v) for v in fine.domlo) + tuple(int(v) for v in fine.domhi)
# uncovered cells: a level's cells minus the coarsened cells of the next finer level
uncovered = sum(lv.ncells for lv in H.levels) - sum(H.levels[l + 1].ncells // H.ref_ratio ** 3 for l in range(H.nlev - 1))

out = {"n": n, "box": box, "reps": reps, "windows": WINDOWS, "max_grid_size": MGS, "levels_cells": [lv.ncells for lv in H.levels], "uncovered_cells": uncovered,
       "plane_pixels": int((dom[3] + 1) * (dom[4] + 1))}
stream = {}
for nc in (1, NV):
    t = timed(lambda: capi.minmax_comps_level(ctx, mfs[-1], list(range(nc))))
    stream[nc] = fine.ncells * 8 * nc / (t[1] * 1e-3) / 1e12
out["stream_TBs"] = {str(k): v for k, v in stream.items()}

rows = []
for dir in (0, 1, 2):
    for nc in (1, NV):
        with capi.Plane(ctx, nc, dir, dom, MGS) as P:
            comps = list(range(nc))
            t = timed(lambda: P.run(mfs, ratios, comps))
            _, nosrc = P.read()
            assert nosrc == 0
            tmm = timed(lambda: P.minmax(0)) if nc == 1 else None
            mn, mx = P.minmax(0)
            tpx = timed(lambda: P.pixelize(0, mn, mx)) if nc == 1 else None
        nbytes = uncovered * 8 * nc
        floor = nbytes / (stream[nc] * 1e12) * 1e3
        rows.append({"kind": "sum", "dir": dir, "ncomp": nc, "ms": t, "floor_bytes": nbytes, "floor_ms": floor, "over_floor": t[1] / floor,
                     "floor_ms_8TBs": nbytes / 8e12 * 1e3, "over_floor_8TBs": t[1] / (nbytes / 8e12 * 1e3), "TBs": nbytes / (t[1] * 1e-3) / 1e12,
                     "minmax_ms": tmm, "pixelize_ms_with_copy": tpx})
    sl = list(dom)
    sl[dir] = sl[3 + dir] = (dom[dir] + dom[3 + dir]) // 2
    with capi.Plane(ctx, 1, dir, sl, 0) as P:
        t = timed(lambda: P.run(mfs, ratios, [0]))
        _, nosrc = P.read()
        assert nosrc == 0
    rows.append({"kind": "slice", "dir": dir, "ncomp": 1, "ms": t})
out["rows"] = rows

f3 = lambda t: "/".join(f"{v:.3f}" for v in t) if t else "-"
print(f"plane_bench: 3 levels x {n}^3 cells in {box}^3 boxes, sub-box = the finest domain ({dom[3] + 1}^3 fine cells, {out['plane_pixels'] / 1e6:.1f} Mpixels), "
      f"max_grid_size {MGS}; per-call ms of {reps} back-to-back pa_plane_run after a warm-up, min/median/max of {WINDOWS} windows")
print(f"floor = the {uncovered / 1e6:.1f} M uncovered cells read once at the streaming rate of pa_minmax_comps_level in this process: "
      + ", ".join(f"{k} comp {v:.2f} TB/s" for k, v in stream.items()))
print(f"{'kind':>5s} {'dir':>3s} {'nc':>2s} {'run ms':>24s} {'floor ms':>8s} {'x floor':>7s} {'x floor@8TB/s':>13s} {'TB/s':>5s} {'minmax ms':>20s} {'pixelize+copy ms':>20s}")
for r in rows:
    if r["kind"] == "sum":
        print(f"{r['kind']:>5s} {r['dir']:3d} {r['ncomp']:2d} {f3(r['ms']):>24s} {r['floor_ms']:8.3f} {r['over_floor']:7.2f} {r['over_floor_8TBs']:13.2f} {r['TBs']:5.2f} "
              f"{f3(r['minmax_ms']):>20s} {f3(r['pixelize_ms_with_copy']):>20s}")
    else:
        print(f"{r['kind']:>5s} {r['dir']:3d} {r['ncomp']:2d} {f3(r['ms']):>24s}")
print(json.dumps(out))
for m in mfs:
    m.close()
for dl in dls:
    dl.close()
ctx.close()
