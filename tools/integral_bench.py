#!/usr/bin/env python3
"""Timing harness of the composite-integral kernels (pa_integral.hip; the device work of integral3d / rmsVel3d) on the headline
hierarchy of tools/stats_bench.py: 3 nested levels on an n^3 base (ratio 2, boxes of `box`^3; every level has n^3 cells), the flame
field made on the device.  Per level and launch: every kind and direction (kind 1 and 2: dir = x, y, z; kind 3) for 1, 4 and 8
variables, without and with a condition window on the last variable, with the combined kernel (private runs, integer wave reduction,
LDS table) and the uncombined one (global atomics per cell).  Two yardsticks of the parent commit are timed in the same process on the
same multifab:
  (a) the READ FLOOR: pa_minmax_comps_level over the same components, i.e. streaming them once;
  (b) pa_condmean_add_level, combined, 128 bins, over the same number of components (the bin variable + nvars - 1 averaged ones;
      2 components for nvars = 1).
Times: host clock around synchronous calls; min / median / max of `reps` calls after 2 warm-up calls.  The uncombined kernel puts
every cell's atomics on a handful of addresses and takes seconds per launch: it is timed ONCE, without warm-up, and only for the cases
`unc` selects (some: 4 variables without a condition; all; none).
usage: python tools/integral_bench.py [n=512] [box=128] [reps=5] [unc=some]   (prints a table and one JSON line)"""
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
reps = max(5, int(sys.argv[3])) if len(sys.argv) > 3 else 5
unc_sel = sys.argv[4] if len(sys.argv) > 4 else "some"
NC = 8
NB = 128
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


def make_level(lv):
    off, cs, total = mf_layout(lv.boxes, NC, 0)
    buf = torch.zeros(total, dtype=torch.float64, device=dev)
    dx = lv.dx
    for b in range(lv.nboxes):
        lo, hi = lv.boxes[b, :3], lv.boxes[b, 3:]
        nx, ny, nz = (int(hi[d] - lo[d] + 1) for d in range(3))
        x = ((torch.arange(lo[0], hi[0] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[0])[None, None, :]
        y = ((torch.arange(lo[1], hi[1] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[1])[None, :, None]
        z = ((torch.arange(lo[2], hi[2] + 1, device=dev, dtype=torch.float64) + 0.5) * dx[2])[:, None, None]
        for m in range(NC):
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


def weight(lv, kind, d):
    dx = lv.dx
    return float(dx[0] * dx[1] * dx[2]) if kind == 3 else (float(dx[(d + 1) % 3] * dx[(d + 2) % 3]) if kind == 2 else float(dx[d]))


KIND_DIR = [(3, 0), (2, 0), (2, 1), (2, 2), (1, 0), (1, 1), (1, 2)]
fl = H.nlev - 1
dom = tuple(int(v) for v in H.levels[fl].domlo) + tuple(int(v) for v in H.levels[fl].domhi)
dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
out = {"n": n, "box": box, "reps": reps, "unc": unc_sel, "cells_per_level": int(H.levels[0].ncells), "cases": []}
for l, lv in enumerate(H.levels):
    buf = make_level(lv)
    mf = capi.DevMF(ctx, dls[l], NC, 0, devptr=buf.data_ptr())
    finer = dls[l + 1] if l < fl else None
    Rl = 2 ** (fl - l)
    ldom = tuple(int(v) for v in lv.domlo) + tuple(int(v) for v in lv.domhi)
    for nv in (1, 4, 8):
        comps = list(range(nv))
        floor = timed(lambda: capi.minmax_comps_level(ctx, mf, comps), reps)
        navg = max(nv - 1, 1)
        cm = capi.CondMeanAcc(ctx, navg, NB, False)
        cm.begin(64, [3000.0] * navg)
        cond = timed(lambda: cm.add_level(mf, finer, 2, ldom, 8 ** (fl - l), 300.0, 2500.0), reps)
        cm.read()
        cm.close()
        for kind, d in KIND_DIR:
            for window in (False, True):
                case = {"level": l, "nvars": nv, "kind": kind, "dir": d, "cond": int(window), "bytes": lv.ncells * nv * 8, "floor_ms": floor, "condmean_ms": cond}
                kw = dict(ccomp=nv - 1, cmin=400.0 * (1.0 + 0.1 * (nv - 1)), cmax=1900.0 * (1.0 + 0.1 * (nv - 1))) if window else {}
                for unc in (False, True):
                    if unc and not (unc_sel == "all" or (unc_sel == "some" and nv == 4 and not window)):
                        continue
                    acc = capi.IntegralAcc(ctx, nv, kind, d, dom)
                    acc.begin(weight(H.levels[0], kind, d), [3000.0] * nv)
                    fn = lambda: acc.add_level(mf, finer, 2, Rl, weight(lv, kind, d), uncombined=unc, **kw)
                    t = timed(fn, 1, 0) if unc else timed(fn, reps)
                    acc.read()  # fails loudly on an overflow flag
                    acc.close()
                    case["uncombined_ms" if unc else "combined_ms"] = t
                case["over_floor"] = case["combined_ms"][1] / floor[1]
                case["over_condmean"] = case["combined_ms"][1] / cond[1]
                case["frac_of_8TBs"] = case["bytes"] / (case["combined_ms"][1] * 1e-3) / HBM
                out["cases"].append(case)
    mf.close()
    del buf
    torch.cuda.empty_cache()

print(f"integral_bench: 3 levels x {n}^3 cells, boxes {box}^3, flame field; ms as min/median/max of {reps} calls after 2 warm-up calls")
print("(a) floor = pa_minmax_comps_level over the same components; (b) condmean = pa_condmean_add_level combined, 128 bins, same number of components")
print("uncombined: ONE call without warm-up")
print(f"{'lev':>3s} {'nv':>2s} {'kind':>4s} {'dir':>3s} {'cond':>4s} {'MB':>6s} {'(a) floor ms':>21s} {'(b) condmean ms':>21s} {'combined ms':>21s} {'x(a)':>6s} {'x(b)':>6s} {'of 8TB/s':>8s} {'uncomb ms':>10s}")
f3 = lambda t: "/".join(f"{v:.3f}" for v in t)
for c in out["cases"]:
    u = f"{c['uncombined_ms'][1]:10.1f}" if "uncombined_ms" in c else f"{'-':>10s}"
    print(f"{c['level']:3d} {c['nvars']:2d} {c['kind']:4d} {c['dir']:3d} {c['cond']:4d} {c['bytes'] / 1e6:6.0f} {f3(c['floor_ms']):>21s} {f3(c['condmean_ms']):>21s} "
          f"{f3(c['combined_ms']):>21s} {c['over_floor']:6.2f} {c['over_condmean']:6.2f} {c['frac_of_8TBs']:8.3f} {u}")
for nv in (1, 4, 8):
    for kind, d in KIND_DIR:
        for window in (0, 1):
            cs_ = [c for c in out["cases"] if c["nvars"] == nv and c["kind"] == kind and c["dir"] == d and c["cond"] == window]
            a, b, t = (sum(c[k][1] for c in cs_) for k in ("floor_ms", "condmean_ms", "combined_ms"))
            worst = max(c["combined_ms"][2] for c in cs_)
            print(f"SUM nv={nv} kind={kind} dir={d} cond={window}: (a) {a:8.3f} ms  (b) {b:8.3f} ms  combined {t:8.3f} ms = {t / a:6.2f} x (a) = {t / b:6.2f} x (b)   slowest call {worst:.3f} ms")
print(json.dumps(out))
for dl in dls:
    dl.close()
ctx.close()
