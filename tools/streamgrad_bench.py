#!/usr/bin/env python3
"""Timing harness of the gradient streamlines (pa_streamgrad.hip; the stream3d tool's device work) on a 3-level nested
hierarchy (base n^3 per level, ratio 2, boxes of `box`^3) of the flame field, seeded on the isosurface temp = 1150: the
crossings of every x-edge of every level's valid cells not covered by the next level (a third of the MEF's nodes).
Times (host clock around synchronous calls, after a warm-up): pa_streamgrad_prepare of the hierarchy, pa_streamgrad_trace
(one launch, the gradient formed on the fly), and for comparison the per-box path pa_vtrace_fab (the gradient materialised
over each box's FAB grown by nGrow-1, as the reference does) over the same seeds.  Run it under rocprofv3 --kernel-trace
--stats for kernel times.  usage: python tools/streamgrad_bench.py [n=256] [box=64] [nRKsteps=51] [reps=3]   (prints one JSON)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (torch first: one HIP runtime)

import streamgrad_ref as R  # noqa: E402
from peleanalysis_amd import capi  # noqa: E402
from peleanalysis_amd.hierarchy import MultiFab, cell_centers, field_flame, nested_hierarchy  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
box = int(sys.argv[2]) if len(sys.argv) > 2 else 64
nRKsteps = int(sys.argv[3]) if len(sys.argv) > 3 else 51
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
ISO = 1150.0
nRKh = (nRKsteps - 1) // 2
hRK0 = 0.1
ng = int(hRK0 * nRKh) + 2

H = nested_hierarchy(n, 3, box, is_per=(0, 0, 0))
t0 = time.time()
raw, seeds = [], []
for l, lv in enumerate(H.levels):
    m = MultiFab(lv, 1, ng)
    for b in range(lv.nboxes):
        x, y, z = cell_centers(lv, b, 0)
        m.valid(b)[0] = field_flame(x, y, z, 0)
    raw.append(m)
    fin = H.levels[l + 1] if l + 1 < H.nlev else None
    dx = R.level_dx(lv)
    for b in range(lv.nboxes):
        v = m.valid(b)[0]
        a, c = v[:, :, :-1] - ISO, v[:, :, 1:] - ISO
        kk, jj, ii = np.nonzero((a < 0) != (c < 0))
        if len(ii) == 0:
            continue
        t = a[kk, jj, ii] / (a[kk, jj, ii] - c[kk, jj, ii])
        lo = lv.boxes[b, :3]
        p = np.stack([(lo[0] + ii + 0.5 + t) * dx[0], (lo[1] + jj + 0.5) * dx[1], (lo[2] + kk + 0.5) * dx[2]])
        if fin is not None:  # covered by the next level: its own crossings stand there
            cov = np.zeros(p.shape[1], dtype=bool)
            for f in fin.boxes:
                flo, fhi = f[:3] * 0.5 * dx, (f[3:] + 1) * 0.5 * dx
                cov |= np.all((p >= flo[:, None]) & (p < fhi[:, None]), axis=0)
            p = p[:, ~cov]
        seeds.append(p)
nodes = np.ascontiguousarray(np.concatenate(seeds, axis=1))
setup_s = time.time() - t0
fin = H.levels[-1]
R.push_nodes_inside(nodes, fin.prob_lo, fin.prob_hi, R.EPS_PUSH * R.level_dx(fin)[0])
ins = R.inside_nodes(H.levels, nodes)
hRK = hRK0 * R.level_dx(fin)[0]

ctx = capi.Context(0)
dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
dms = [capi.DevMF(ctx, dl, 1, ng) for dl in dls]
out = {"hierarchy": f"3 levels of {n}^3 cells, boxes of {box}^3, ratio 2, nGrow {ng}", "nRKsteps": nRKsteps, "seeds": int(nodes.shape[1])}


def timed(fn):
    fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ctx.sync()
        ts.append(time.perf_counter() - t)
    return min(ts)


def prep():
    for d, m in zip(dms, raw):
        d.upload(m)
    capi.streamgrad_prepare(ctx, dms)


t = time.perf_counter()
prep()
ctx.sync()
out["upload_and_prepare_ms_first"] = 1e3 * (time.perf_counter() - t)
out["prepare_ms"] = 1e3 * timed(lambda: capi.streamgrad_prepare(ctx, dms))
res = {}
out["trace_ms"] = 1e3 * timed(lambda: res.setdefault("otf", capi.streamgrad_trace(ctx, dms, nodes, ins, nRKsteps, hRK)))
out["lines_per_s"] = 2 * out["seeds"] / (out["trace_ms"] * 1e-3)

# the per-box path: vtrace with the gradient materialised over every box that holds seeds (pa_vtrace_fab, one call per box)
nb = capi.DevBuf.from_numpy(ctx, nodes)
per_box = []
for l, lv in enumerate(H.levels):
    for b in range(lv.nboxes):
        ids = ins[l][b]
        if len(ids) == 0:
            continue
        T = dms[l].fab(b)
        g = capi.PaFab()
        shape = [T.hi[d] - T.lo[d] - 1 for d in range(3)]
        cnt = int(np.prod(shape))
        gb = capi.DevBuf(ctx, 8 * 3 * cnt)
        g.p, g.ncomp, g.nstride = gb.ptr, 3, cnt
        for d in range(3):
            g.lo[d], g.hi[d] = T.lo[d] + 1, T.hi[d] - 1
        sb = capi.DevBuf(ctx, 8 * 4 * nRKsteps * len(ids))
        s = capi.PaFab()
        s.p, s.ncomp, s.nstride = sb.ptr, 4, nRKsteps * len(ids)
        s.lo[0], s.lo[1], s.lo[2], s.hi[0], s.hi[1], s.hi[2] = 0, -nRKh, 0, len(ids) - 1, nRKsteps - 1 - nRKh, 0
        ib = capi.DevBuf.from_numpy(ctx, np.asarray(ids, np.int32))
        per_box.append((l, b, T, g, gb, s, sb, ib, len(ids)))


def fab_path():
    e = C.c_int32(0)
    for l, b, T, g, gb, s, sb, ib, k in per_box:
        ctx.check(ctx.lib.pa_vtrace_fab(ctx.h, C.byref(T), 1, C.c_void_p(nb.ptr), nodes.shape[1], C.c_void_p(ib.ptr), k, C.byref(g), 1, C.byref(s), 4,
                                        capi._d3(R.level_dx(H.levels[l])), capi._d3(fin.prob_lo), capi._d3(fin.prob_hi), hRK, C.byref(e)))


out["per_box_materialised_ms"] = 1e3 * timed(fab_path)
out["boxes_with_seeds"] = len(per_box)
# the two paths give the same lines (the gradient is one subtraction either way)
lines, _ = res["otf"]
same = True
for l, b, T, g, gb, s, sb, ib, k in per_box:
    same = same and np.array_equal(sb.to_numpy(np.float64, (4, nRKsteps, k)).view(np.int64), lines[l][b].view(np.int64))
out["paths_bit_identical"] = bool(same)
out["host_setup_s"] = setup_s
print(json.dumps(out))
