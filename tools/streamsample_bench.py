#!/usr/bin/env python3
"""Timing harness of the sampling along streamlines (pa_streamsample.hip; the sampleStreamlines3d tool's device work) on the
hierarchy of tools/streamgrad_bench.py: 3 nested levels (base n^3 per level, ratio 2, boxes of `box`^3) of the flame field, lines
traced by pa_streamgrad_trace from the isosurface temp = 1150 (nRKsteps points per line).  K = 1, 8 and 32 components are then
sampled at every point.  Times (host clock around synchronous calls, after a warm-up): pa_streamsample_run (one launch of
k_ss_sample; X / Y / Z and the distances are a separate small launch, run once), and the per-box path pa_interpstream_fab over
the same points (one call per Str box, each box's data FAB grown by nGrow standing in for the staged FAB).  Write bytes of the
launch: 8 * K * points.  Run it under rocprofv3 --kernel-trace --stats for kernel times.
usage: python tools/streamsample_bench.py [n=256] [box=64] [nRKsteps=51] [reps=5]   (prints one JSON)"""
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
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
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
for d, m in zip(dms, raw):
    d.upload(m)
capi.streamgrad_prepare(ctx, dms)
lines, _ = capi.streamgrad_trace(ctx, dms, nodes, ins, nRKsteps, hRK)
for d in dms:
    d.close()

# the streamFile's Str boxes: one per file box, (0,-nRKh,0)..(n-1,nRKsteps-1-nRKh,0) or the null box
NG = 4  # sampleStreamlines' default nGrow
fdx = [R.level_dx(lv) for lv in H.levels]
plo = H.levels[0].prob_lo
sboxes, has, bbox, xyz = [], [], [], []
for l, lv in enumerate(H.levels):
    sb, hl, bb, xs = [], [], [], []
    for b in range(lv.nboxes):
        st = lines[l][b]
        if st is None:
            sb.append((0, 0, 0, 0, 0, 0)); hl.append(0); bb.append((0,) * 6); xs.append(np.zeros((3, 1, 1)))
            continue
        k = st.shape[2]
        sb.append((0, -nRKh, 0, k - 1, nRKsteps - 1 - nRKh, 0)); hl.append(1)
        seeds = st[:3, nRKh]
        lo = [int(np.trunc((seeds[d].min() - plo[d]) / fdx[l][d])) - NG for d in range(3)]
        hi = [int(np.trunc((seeds[d].max() - plo[d]) / fdx[l][d])) + NG for d in range(3)]
        bb.append(tuple(lo + hi))
        xs.append(np.ascontiguousarray(st[:3]))
    sboxes.append(sb); has.append(hl); bbox.append(bb); xyz.append(xs)
npts = sum(int(x[0].size) for per, hl in zip(xyz, has) for x, h in zip(per, hl) if h)
out = {"hierarchy": f"3 levels of {n}^3 cells, boxes of {box}^3, ratio 2", "nRKsteps": nRKsteps, "lines": int(nodes.shape[1]), "points": npts}


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


xb = None
for K in (1, 8, 32):
    data = []
    for l, lv in enumerate(H.levels):
        m = MultiFab(lv, K, 0)
        for b in range(lv.nboxes):
            v = raw[l].valid(b)[0]
            for c in range(K):
                m.valid(b)[c] = v * (1.0 + 0.01 * c)
        data.append(capi.DevMF.from_host(ctx, dls[l], m))
    ncout = 4 + K
    ob, _, st = capi.streamsample_run(ctx, data, K, fdx, plo, (0, 0, 0), sboxes, has, bbox, xyz, ncout)
    assert not any(s for per in st for s in per)
    # the same call on prepared host arrays, so that only the launch (and its small copies) is timed
    nbox = np.array([len(b) for b in sboxes], np.int32)
    sbx = np.ascontiguousarray(np.array([b for per in sboxes for b in per], np.int32))
    hl = np.ascontiguousarray(np.array([h for per in has for h in per], np.int32))
    bbx = np.ascontiguousarray(np.array([b for per in bbox for b in per], np.int32))
    xs = np.concatenate([np.asarray(x).reshape(3, -1).ravel() for per in xyz for x in per])
    xb = capi.DevBuf.from_numpy(ctx, xs)
    fd = np.ascontiguousarray(np.array(fdx, np.float64))
    fail = np.zeros(len(hl), np.int32)
    hnd = capi._handles(data)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))

    def launch(xyzd=0):
        ctx.check(ctx.lib.pa_streamsample_run(ctx.h, len(data), hnd, K, fd.ctypes.data_as(C.POINTER(C.c_double)), capi._d3(plo), capi._i3((0, 0, 0)), P(nbox),
                                              P(sbx), P(hl), P(bbx), C.c_void_p(xb.ptr), C.c_void_p(ob.ptr), ncout, 4, xyzd, P(fail)))

    ms = 1e3 * timed(launch)
    # per-box path: pa_interpstream_fab on each box's FAB grown by nGrow (K components), one call per Str box
    stage = [capi.DevMF(ctx, dls[l], K, NG) for l in range(H.nlev)]
    items, g = [], 0
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            if has[l][b]:
                x = xyz[l][b]
                lb = capi.DevBuf.from_numpy(ctx, x)
                loc = capi._dev_fab(lb, (0, -nRKh, 0), (1,) + x.shape[1:], 3)
                sb = capi.DevBuf(ctx, 8 * K * x[0].size)
                so = capi._dev_fab(sb, (0, -nRKh, 0), (1,) + x.shape[1:], K)
                items.append((l, stage[l].fab(b), lb, loc, sb, so))
    stt = C.c_int32(0)

    def per_box():
        for l, F, lb, loc, sb, so in items:
            ctx.check(ctx.lib.pa_interpstream_fab(ctx.h, C.byref(loc), 3, C.byref(F), K, C.byref(so), capi._d3(fdx[l]), capi._d3(plo), C.byref(stt)))

    pb = 1e3 * timed(per_box)
    wb = 8.0 * K * npts
    out[f"K{K}"] = {"launch_ms": ms, "per_box_ms": pb, "boxes": len(items), "point_comps_per_s": K * npts / (ms * 1e-3), "write_bytes": wb,
                    "write_frac_of_8TBps": wb / (ms * 1e-3) / 8e12}
    for s in stage:
        s.close()
    for d in data:
        d.close()
print(json.dumps(out))
