#!/usr/bin/env python3
"""Timing harness of the stream-tube kernels (pa_tubestats.hip; the streamTubeStats3d tool's device work) on the lines of
tools/streamsample_bench.py: 3 nested levels (base n^3 per level, ratio 2, boxes of `box`^3) of the flame field, lines traced by
pa_streamgrad_trace from the crossings of temp = 1150 (nRKsteps points per line; n = 256: 2.14 M line points).  The crossings carry no
connectivity, so two triangles per node join neighbours in node order -- (q, q+1, q+2) and (q, q+2, q+3), the valence of a real
surface -- and the K = 1, 8, 32 "sampled" components are analytic functions of the line points made on the device (their values do
not change the work; staging 32 components of the hierarchy on the host would take 12 GB).
Timed, each warm, with device events around `reps` back-to-back calls (every call ends in a stream synchronise, so a call of a few
tens of microseconds is dominated by that): the wedge kernel for K = 1, 8, 32, the line kernels (max_grad, peak_val), the
neighbour build on a fresh tube (its allocations and one 8-byte read-back included; the tube's own creation subtracted) and one
smoothing pass (21 passes minus 11, over 10).  Next to each: the READ FLOOR -- the unique bytes of Str data touched, read once at 8 TB/s -- and for the wedges also the
GATHERED bytes (three nodes per triangle and a re-read of the coordinates per sweep of 8 components) at the same rate: which of the
two a time sits near tells whether the L2 serves the reuse.
usage: python tools/tubestats_bench.py [n=256] [box=64] [nRKsteps=51] [reps=20]   (prints a table and one JSON line)"""
import ctypes as C
import json
import os
import sys

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
ISO, HBM = 1150.0, 8.0e12
nRKh = (nRKsteps - 1) // 2
ng = int(0.1 * nRKh) + 2

# ---- the lines, as tools/streamsample_bench.py makes them
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

# ---- the tables: one Str box per file box with lines, a placeholder elsewhere
N = nodes.shape[1]
box_desc, node_table, xs, off = [], np.zeros((N, 2), np.int32), [], 0
for l, lv in enumerate(H.levels):
    for b in range(lv.nboxes):
        st = lines[l][b]
        if st is None:
            box_desc.append((1, 1, 0, off)); xs.append(np.zeros((3, 1, 1))); off += 1
            continue
        k = st.shape[2]
        ids = np.asarray(ins[l][b]) - 1
        node_table[ids, 0], node_table[ids, 1] = len(box_desc), np.arange(k)
        box_desc.append((k, nRKsteps, -nRKh, off)); xs.append(np.ascontiguousarray(st[:3])); off += k * nRKsteps
q = np.arange(N - 3)
face = np.concatenate([np.stack([q, q + 1, q + 2], 1), np.stack([q, q + 2, q + 3], 1)]).astype(np.int32) + 1
E, npts = len(face), N * nRKsteps
tube = capi.Tube(ctx, box_desc, node_table, face)
xyz_h = capi.Tube.flat(xs)
xyz = capi.DevBuf.from_numpy(ctx, xyz_h)


def components(K):
    """box g at K * off_g, component-major: c-th component = T-like(x, y, z) * (1 + 0.01 c), made with torch on the device"""
    parts = []
    for (ni, nj, _, _), x in zip(box_desc, xs):
        t = torch.from_numpy(x.reshape(3, -1)).cuda()
        base = 300.0 + 850.0 * (1.0 + torch.tanh((torch.sqrt(((t - 0.5) ** 2).sum(0)) - 0.25) / 0.05))
        parts.append((base[None, :] * (1.0 + 0.01 * torch.arange(K, device="cuda", dtype=torch.float64))[:, None]).reshape(-1))
    return torch.cat(parts)


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
out = {"hierarchy": f"3 levels of {n}^3 cells, boxes of {box}^3, ratio 2", "nRKsteps": nRKsteps, "lines": N, "points": npts, "elements": E, "reps": reps, "rows": []}
geo = [capi.DevBuf(ctx, 8 * E) for _ in range(3)]
rows = []
for K in (1, 8, 32):
    d = components(K)
    raw_b, per_b = capi.DevBuf(ctx, 8 * K * E), capi.DevBuf(ctx, 8 * K * E)
    ms = timed(lambda: ctx.check(ctx.lib.pa_tube_wedges(ctx.h, tube.h, vp(xyz.ptr), vp(d.data_ptr()), K, -nRKh, nRKsteps, 1, vp(geo[0].ptr), vp(geo[1].ptr), vp(geo[2].ptr),
                                                        vp(raw_b.ptr), vp(per_b.ptr))))
    sweeps = (K + 7) // 8
    unique = 8.0 * (3 + K) * npts
    gathered = 8.0 * 3 * E * nRKsteps * (3 * sweeps + K)
    rows.append((f"wedges K={K}", ms, unique, gathered))
    if K == 8:
        gm, ok = capi.DevBuf(ctx, 8 * N), capi.DevBuf(ctx, 4 * N)
        sc = (C.c_int32 * 1)(0)
        for eps in (0, 1):
            ms = timed(lambda: ctx.check(ctx.lib.pa_tube_lines(ctx.h, tube.h, vp(xyz.ptr), vp(d.data_ptr()), K, 3, eps, vp(gm.ptr))))
            rows.append((f"lines max_grad use_eps={eps}", ms, 8.0 * 4 * npts, None))  # X, Y, Z (twice, the second pass from cache or not) and one component
        ms = timed(lambda: ctx.check(ctx.lib.pa_tube_peaks(ctx.h, tube.h, vp(d.data_ptr()), K, 3, 1, sc, vp(gm.ptr), vp(ok.ptr))))
        rows.append(("lines peak_val", ms, 8.0 * npts, None))
    del d, raw_b, per_b


def csr_build():
    t = capi.Tube(ctx, box_desc, node_table, face)
    nnz = C.c_int64(0)
    ctx.check(ctx.lib.pa_tube_neighbors(ctx.h, t.h, C.byref(nnz), None, None))
    t.close()
    return nnz.value


def create_only():
    capi.Tube(ctx, box_desc, node_table, face).close()


nnz = csr_build()
ms_build = timed(csr_build, 5) - timed(create_only, 5)
rows.append(("neighbour build (CSR)", ms_build, 4.0 * 3 * E * 4 + 4.0 * nnz, None))  # the connectivity four times, the columns once
vals, area, sm = capi.DevBuf.from_numpy(ctx, np.random.default_rng(0).random(E)), capi.DevBuf.from_numpy(ctx, np.random.default_rng(1).random(E) + 0.1), capi.DevBuf(ctx, 8 * E)
tube.neighbors()
t21 = timed(lambda: ctx.check(ctx.lib.pa_tube_smooth(ctx.h, tube.h, vp(vals.ptr), vp(area.ptr), 21, vp(sm.ptr))), 5)
t11 = timed(lambda: ctx.check(ctx.lib.pa_tube_smooth(ctx.h, tube.h, vp(vals.ptr), vp(area.ptr), 11, vp(sm.ptr))), 5)
rows.append(("smoothing, one pass", (t21 - t11) / 10.0, 8.0 * 3 * E + 8.0 * (E + 1) + 4.0 * nnz, None))  # vals, area, out, row pointers, columns

print(f"{N} lines, {npts} line points, {E} triangles, {nnz} neighbour entries")
print(f"{'kernel':32s} {'ms':>9s} {'unique MB':>10s} {'floor ms':>9s} {'gathered MB':>12s} {'floor ms':>9s}")
for name, ms, u, g in rows:
    line = f"{name:32s} {ms:9.4f} {u / 1e6:10.1f} {1e3 * u / HBM:9.4f}"
    if g is not None:
        line += f" {g / 1e6:12.1f} {1e3 * g / HBM:9.4f}"
    print(line)
    out["rows"].append({"kernel": name, "ms": ms, "unique_bytes": u, "unique_floor_ms": 1e3 * u / HBM, "gathered_bytes": g, "gathered_floor_ms": None if g is None else 1e3 * g / HBM})
print(json.dumps(out))
