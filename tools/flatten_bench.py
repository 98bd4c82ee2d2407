#!/usr/bin/env python3
"""Timing harness of pa_flatten_level (pa_flatten.hip; the device work of flattenAMRFile3d): the headline hierarchy -- 3 nested
levels on an n^3 base, ratio 2, file boxes of `box`^3, every level n^3 cells -- flattened at level 2: (4 n)^3 output cells in boxes
of `grid`^3, walked in slabs of `slab` consecutive boxes, `nvar` components, interp_type 1, the flame field made on the device.

Per slab and in total, timed in the same process:
  flatten  : pa_flatten_level of the slab (k_prolong + k_overlay; the coarser work multifab is made once, before);
  resample : the route without this entry point -- the one-file average on the same boxes: the slab's running sum zeroed
             (pa_mf_setval) + pa_resample_add_file_level.  The scale pass of pa_resample_finish (another read and write of the
             slab) is NOT in this figure, so it flatters the resample route;
  floor    : pa_mf_copy of nvar / 2 components on the slab = the output's bytes moved once.
counted_B_per_cell_var: bytes per output cell and variable that pa_flatten_level has to move, COUNTED from the geometry, not measured
(no counter pass): the 8-byte store + every coarse value read once (8 / ratio^3) in boxes that are not skipped as covered, + 16 for a
cell the file holds (read, stored).
`whole` rows: the complete job on all levels -- 3 calls of pa_flatten_level against begin + 3 add_file_level + finish.
Times: host clock around a call + synchronise; min / median / max of `reps` calls after 2 warm-up calls.
tool=<dir>: also runs flattenAMRFile3d.ex on a plotfile of the tn^3-base hierarchy written into <dir>, with stream_write=1 (slabs go
to a writer thread while the next one is computed) and stream_write=0 (one host multifab, written at the end), wall time of each.
usage: python tools/flatten_bench.py [n=256] [box=64] [reps=7] [grid=64] [nvar=4] [slab=1024] [tool=<dir>] [tn=128]
(prints a table and one JSON line)"""
import json
import math
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch first: one HIP runtime)

from peleanalysis_amd import capi  # noqa: E402
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, chop_box, field_flame, fill_analytic, mf_layout  # noqa: E402

kv = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
pos = [a for a in sys.argv[1:] if "=" not in a]
n = int(kv.get("n", pos[0] if len(pos) > 0 else 256))
box = int(kv.get("box", pos[1] if len(pos) > 1 else 64))
reps = max(5, int(kv.get("reps", pos[2] if len(pos) > 2 else 7)))
grid = int(kv.get("grid", pos[3] if len(pos) > 3 else 64))
NV = int(kv.get("nvar", pos[4] if len(pos) > 4 else 4))
slab = int(kv.get("slab", pos[5] if len(pos) > 5 else 1024))
NLEV, RATIO, INTERP = 3, 2, 1
IS_PER = (1, 1, 0)
assert n % 8 == 0 and NV % 2 == 0

dev = torch.device("cuda:0")
ctx = capi.Context(0)


def level(boxes, l, m=None):
    m = (m or n) * RATIO ** l
    return Level(boxes, (0, 0, 0), (m - 1,) * 3, IS_PER, np.zeros(3), np.ones(3))


def file_levels(m=None, bx=None):
    """level 1 = the central half-width cube, level 2 = the central half of level 1: every level m^3 cells"""
    m, bx = m or n, bx or box
    lo1 = np.full(3, m // 2)
    lo2 = 2 * lo1 + m // 2
    return [level(chop_box((0, 0, 0), (m - 1,) * 3, bx), 0, m), level(chop_box(lo1, lo1 + m - 1, bx), 1, m), level(chop_box(lo2, lo2 + m - 1, bx), 2, m)]


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
    a, b = a.astype(np.int64), b.astype(np.int64)
    tot = 0
    for row in a:
        w = np.minimum(row[3:], b[:, 3:]) - np.maximum(row[:3], b[:, :3]) + 1
        tot += int(np.prod(np.maximum(w, 0), axis=1).sum())
    return tot


files = file_levels()
ident = list(range(NV))
ghosts = [capi.Flatten.ghosts(NLEV, l, [RATIO] * (NLEV - 1), INTERP) for l in range(NLEV)]
bufs = [make_level(lv) for lv in files]
fdl = [capi.DevLevel(ctx, lv) for lv in files]
fmf = [capi.DevMF(ctx, fdl[l], NV, 0, devptr=bufs[l].data_ptr()) for l in range(NLEV)]
out_levels = [level(chop_box((0, 0, 0), (n * RATIO ** l - 1,) * 3, grid), l) for l in range(NLEV)]
dls = [capi.DevLevel(ctx, lv) for lv in out_levels[:2]]
work = [capi.DevMF(ctx, dls[l], NV, ghosts[l]) for l in range(2)]
run01 = [capi.DevMF(ctx, dls[l], NV, 0) for l in range(2)]
fl = capi.Flatten(ctx)
lib = ctx.lib
nosrc = capi.C.c_int64(0)


def flat(l, out):
    ctx.check(lib.pa_flatten_level(ctx.h, fmf[l].h, np.asarray(ident, dtype=np.int32).ctypes.data_as(capi.C.POINTER(capi.C.c_int32)),
                                   work[l - 1].h if l else None, RATIO, INTERP, out.h, NV, capi.C.byref(nosrc)))


rows = []
lower = [timed(lambda l=l: flat(l, work[l]), reps) for l in range(2)]  # also leaves the work multifabs filled
ob = out_levels[2].boxes
tot = {"flatten": np.zeros(3), "resample": np.zeros(3), "floor": np.zeros(3)}
launches = []
for s0 in range(0, len(ob), slab):
    sl = level(ob[s0:s0 + slab], 2)
    sdl = capi.DevLevel(ctx, sl)
    out = capi.DevMF(ctx, sdl, NV, 0)
    t_flat = timed(lambda: flat(2, out), reps)
    launches.append(fl.last_launch())
    out.close()
    runs = capi.DevMF(ctx, sdl, NV, 0)
    rs = capi.Resample(ctx)
    rs.begin(run01 + [runs], NV)

    def resample():
        runs.setval(0.0, 0, NV)
        rs.add_file_level(2, fmf[2], ident, work[1], RATIO, INTERP, None)
    t_rs = timed(resample, reps)
    rs.finish(1)
    rs.close()
    runs.close()
    a, b = capi.DevMF(ctx, sdl, NV // 2, 0), capi.DevMF(ctx, sdl, NV // 2, 0)
    a.setval(1.0)
    t_floor = timed(lambda: ctx.check(lib.pa_mf_copy(ctx.h, a.h, 0, b.h, 0, NV // 2, 0)), reps)
    a.close()
    b.close()
    cells = sl.ncells
    held = overlap_cells(sl.boxes, files[2].boxes)
    skipped_cells = sum(int(np.prod(bx[3:].astype(np.int64) - bx[:3] + 1)) for bx in sl.boxes
                        if overlap_cells(bx[None, :], files[2].boxes) == int(np.prod(bx[3:].astype(np.int64) - bx[:3] + 1)))
    rows.append({"slab": s0 // slab, "boxes": sl.nboxes, "cells": cells, "interpolated": 1.0 - held / cells, "flatten_ms": t_flat, "resample_ms": t_rs, "floor_ms": t_floor,
                 "counted_B_per_cell_var": ((cells - skipped_cells) * (8.0 + 8.0 / RATIO ** 3) + 16.0 * held) / cells, "speedup": t_rs[1] / t_flat[1], "flatten_over_floor": t_flat[1] / t_floor[1], "resample_over_floor": t_rs[1] / t_floor[1],
                 "floor_TBs": NV * 8 * cells / (t_floor[1] * 1e-3) / 1e12, "flatten_out_TBs": NV * 8 * cells / (t_flat[1] * 1e-3) / 1e12})
    for k, t in (("flatten", t_flat), ("resample", t_rs), ("floor", t_floor)):
        tot[k] += np.array(t)
    sdl.close()

# the complete job on all levels, output level whole
whole = None
try:
    odl = capi.DevLevel(ctx, out_levels[2])
    out = capi.DevMF(ctx, odl, NV, 0)
    t_flat = timed(lambda: [flat(0, work[0]), flat(1, work[1]), flat(2, out)], reps)
    out.close()
    runs = capi.DevMF(ctx, odl, NV, 0)
    rs = capi.Resample(ctx)

    def average():
        rs.begin(run01 + [runs], NV)
        for l in range(NLEV):
            rs.add_file_level(l, fmf[l], ident, work[l - 1] if l else None, RATIO, INTERP, work[l] if l < 2 else None)
        assert rs.finish(1) == 0
    t_rs = timed(average, reps)
    rs.close()
    runs.close()
    odl.close()
    whole = {"flatten_ms": t_flat, "resample_ms": t_rs, "speedup": t_rs[1] / t_flat[1]}
except capi.PaError as e:  # the whole level does not fit next to the rest
    whole = {"error": str(e)}

res = {"n": n, "box": box, "reps": reps, "grid": grid, "nvar": NV, "slab_boxes": slab, "interp_type": INTERP, "out_cells": int(out_levels[2].ncells),
       "lower_levels_ms": lower, "rows": rows, "total_ms": {k: v.tolist() for k, v in tot.items()}, "launches": launches, "whole": whole, "nosrc": int(nosrc.value)}
res["total_speedup"] = tot["resample"][1] / tot["flatten"][1]
f3 = lambda t: "/".join(f"{v:.3f}" for v in t)
print(f"flatten_bench: {n}^3 base, 3 levels, flattened at level 2 = {4 * n}^3 cells in boxes of {grid}^3, slabs of {slab} boxes, {NV} components, interp_type {INTERP};"
      f" ms as min/median/max of {reps} calls after 2 warm-up calls")
print("resample = pa_mf_setval of the slab's running sum + pa_resample_add_file_level (without the scale pass of finish); floor = pa_mf_copy of the output's bytes")
print(f"{'slab':>5s} {'boxes':>6s} {'Mcells':>7s} {'interp':>6s} {'flatten ms':>24s} {'resample ms':>24s} {'floor ms':>24s} {'rs/fl':>6s} {'fl/floor':>8s} {'rs/floor':>8s} {'out TB/s':>8s} {'B/cell':>6s}")
for r in rows:
    print(f"{r['slab']:5d} {r['boxes']:6d} {r['cells'] / 1e6:7.1f} {r['interpolated']:6.3f} {f3(r['flatten_ms']):>24s} {f3(r['resample_ms']):>24s} {f3(r['floor_ms']):>24s} "
          f"{r['speedup']:6.2f} {r['flatten_over_floor']:8.2f} {r['resample_over_floor']:8.2f} {r['flatten_out_TBs']:8.2f} {r['counted_B_per_cell_var']:6.2f}")
print(f"{'total':>5s} {len(ob):6d} {out_levels[2].ncells / 1e6:7.1f} {'':6s} {f3(tot['flatten']):>24s} {f3(tot['resample']):>24s} {f3(tot['floor']):>24s} {res['total_speedup']:6.2f}")
print("levels 0 and 1 (ghosted work multifabs, general route), ms:", [f3(t) for t in lower])
print("whole job, all levels (flatten x 3 | begin + add x 3 + finish):", whole)
print("launch records (wide, general, skipped, rectangles) per slab:", launches)

if "tool" in kv:  # the tool end to end: stream_write=1 against stream_write=0
    tn = int(kv.get("tn", 128))
    d = kv["tool"]
    os.makedirs(d, exist_ok=True)
    tl = file_levels(tn, min(box, tn // 2))
    mfs = []
    for lv in tl:
        m = MultiFab(lv, NV, 0)
        for c in range(NV):
            fill_analytic(m, c, lambda x, y, z, c=c: field_flame(x, y, z, c))
        mfs.append(m)
    from peleanalysis_amd.plotfile import write_plotfile  # noqa: E402
    src = os.path.join(d, "plt_bench")
    write_plotfile(src, Hierarchy(tl, RATIO), mfs, [f"v{c}" for c in range(NV)], time=1.0)
    exe = os.path.join(ROOT, "tools", "bin", "flattenAMRFile3d.ex")
    res["tool"] = {"base": tn, "out_cells": (4 * tn) ** 3, "nvar": NV}
    for tag, extra in (("stream_write=1", []), ("stream_write=0", ["stream_write=0"]), ("stream_write=1 slab_boxes=64", ["slab_boxes=64"])):
        ts = []
        for rep in range(2):
            o = os.path.join(d, "flat_out")
            shutil.rmtree(o, ignore_errors=True)
            t0 = time.perf_counter()
            r = subprocess.run([exe, "infile=" + src, "output_file=" + o, "output_level=2", "output_max_grid_size=%d" % grid, "is_per=1 1 0"] + extra, capture_output=True, text=True, timeout=600)
            ts.append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr[-2000:]
        res["tool"][tag] = ts
        print(f"flattenAMRFile3d.ex {tn}^3 base -> {4 * tn}^3 cells x {NV} variables, {tag}: wall s (two runs) {ts}")
    shutil.rmtree(d, ignore_errors=True)
print(json.dumps(res))
ctx.close()
