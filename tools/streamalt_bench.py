#!/usr/bin/env python3
"""Timing harness of the alternate-surface kernel (pa_streamalt.hip; stream3d's buildAltSurf) on the lines of
tools/tubestats_bench.py: 3 nested levels (base n^3 per level, ratio 2, boxes of `box`^3) of the flame field, lines traced by
pa_streamgrad_trace from the crossings of temp = 1150 (nRKsteps points per line; n = 256: 2.14 M line points, X Y Z temp per point).
Timed, warm, with device events around `reps` back-to-back calls of pa_streamalt_run (a synchronous entry point: each call uploads
the box table, checks the node ids in a launch of their own, reads one flag back and ends in a stream synchronise, so a short kernel
sits under that overhead; the kernel's own time comes from rocprofv3 --kernel-trace --stats on this script):
  alt            the search for temp = ALT on every line, position, temp and distance there
  alt + angle    the same with the angle's cosine
  all            alt, the thermal thickness between two further values of temp, the "cold strain" (temp read where temp crosses a
                 fourth value) and the angle: four queries on one distinct component
Next to each the READ FLOOR: the unique Str bytes the kernel must touch -- X Y Z and every distinct query component of every point
-- read once at 8 TB/s (the first march reads the query components, the second X Y Z: no point is read twice).  Also timed: the
device-to-host copy of the whole line buffer, which the tool performs anyway to write streamFile / outFile.
usage: python tools/streamalt_bench.py [n=256] [box=64] [nRKsteps=51] [reps=20]   (prints a table and one JSON line)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (torch first: one HIP runtime)

import streamgrad_ref as R  # noqa: E402
from peleanalysis_amd import capi  # noqa: E402
from peleanalysis_amd.hierarchy import MultiFab, cell_centers, field_flame, nested_hierarchy  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 256
box = int(sys.argv[2]) if len(sys.argv) > 2 else 64
nRKsteps = int(sys.argv[3]) if len(sys.argv) > 3 else 51
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
ISO, ALT, HBM = 1150.0, 1300.0, 8.0e12
nRKh = (nRKsteps - 1) // 2
ng = int(0.1 * nRKh) + 2

# ---- the lines, as tools/tubestats_bench.py makes them
H = nested_hierarchy(n, 3, box, is_per=(0, 0, 0))
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
        if fin is not None:
            cov = np.zeros(p.shape[1], dtype=bool)
            for f in fin.boxes:
                flo, fhi = f[:3] * 0.5 * dx, (f[3:] + 1) * 0.5 * dx
                cov |= np.all((p >= flo[:, None]) & (p < fhi[:, None]), axis=0)
            p = p[:, ~cov]
        seeds.append(p)
nodes = np.ascontiguousarray(np.concatenate(seeds, axis=1))
fin = H.levels[-1]
R.push_nodes_inside(nodes, fin.prob_lo, fin.prob_hi, R.EPS_PUSH * R.level_dx(fin)[0])
ins = R.inside_nodes(H.levels, nodes)
hRK = 0.1 * R.level_dx(fin)[0]

stream = torch.cuda.Stream()  # the library on a stream of torch's: torch's events time its launches
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)
dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
dms = [capi.DevMF(ctx, dl, 1, ng) for dl in dls]
for d, m in zip(dms, raw):
    d.upload(m)
capi.streamgrad_prepare(ctx, dms)
lines, _ = capi.streamgrad_trace(ctx, dms, nodes, ins, nRKsteps, hRK)
for d in dms:
    d.close()
del raw

# ---- the trace's buffer back on the device, as the tool holds it between the trace and the download
N, ncs = nodes.shape[1], 4
counts = [len(i) for per in ins for i in per]
start = np.zeros(len(counts) + 1, dtype=np.int64)
start[1:] = np.cumsum(counts)
assert int(start[-1]) == N
flat = np.concatenate([x.ravel() for per in lines for x in per if x is not None])
npts = N * nRKsteps
assert flat.size == ncs * npts
strm = capi.DevBuf.from_numpy(ctx, flat)
ids = capi.DevBuf.from_numpy(ctx, np.concatenate([np.asarray(i, np.int32) for per in ins for i in per]))
out = capi.DevBuf(ctx, 8 * 16 * N)
host = np.empty_like(flat)


def params(thick, strain, angle):
    P = capi.PaStreamAltParams()
    P.isoComp, P.altVal, P.ncarry = 3, ALT, 1
    P.carry[0] = 3
    P.thickComp, P.thickLo, P.thickHi = (3 if thick else -1), 800.0, 1500.0
    P.TComp, P.strainComp, P.TVal = (3 if strain else -1), 3, 600.0
    P.addAngle = int(angle)
    return P


def timed(fn, nrep=reps):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(nrep):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / nrep


vp = C.c_void_p
rows = []
for name, P, ncomp_read in (("alt", params(0, 0, 0), 4), ("alt + angle", params(0, 0, 1), 4), ("all (4 queries on temp, angle)", params(1, 1, 1), 4)):
    ms = timed(lambda: ctx.check(ctx.lib.pa_streamalt_run(ctx.h, len(counts), start.ctypes.data_as(C.POINTER(C.c_int64)), vp(ids.ptr), vp(strm.ptr), ncs, nRKsteps, N,
                                                          C.byref(P), vp(out.ptr), None)))
    rows.append((name, ms, 8.0 * ncomp_read * npts))


def d2h():
    ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, host.ctypes.data_as(vp), vp(strm.ptr), host.nbytes))


d2h()
t0 = time.perf_counter()
for _ in range(3):
    d2h()
d2h_ms = 1e3 * (time.perf_counter() - t0) / 3

res = {"hierarchy": f"3 levels of {n}^3 cells, boxes of {box}^3, ratio 2", "nRKsteps": nRKsteps, "lines": N, "points": npts, "ncs": ncs, "reps": reps,
       "strm_bytes": int(host.nbytes), "d2h_ms": d2h_ms, "rows": []}
print(f"{N} lines, {npts} line points, {ncs} components, {host.nbytes / 1e6:.1f} MB of lines; device-to-host copy of them {d2h_ms:.3f} ms")
print(f"{'call':34s} {'ms':>9s} {'unique MB':>10s} {'floor ms':>9s} {'ratio':>7s}")
for name, ms, u in rows:
    fl = 1e3 * u / HBM
    print(f"{name:34s} {ms:9.4f} {u / 1e6:10.1f} {fl:9.4f} {ms / fl:7.1f}")
    res["rows"].append({"call": name, "ms": ms, "unique_bytes": u, "floor_ms": fl, "ratio": ms / fl})
print(json.dumps(res))
