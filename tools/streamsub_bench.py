#!/usr/bin/env python3
"""Timing harness of the subsetting of streamSub3d (pa_streamsub.hip: pa_ssub_select_seedbox, pa_ssub_plan, pa_ssub_gather) on a synthetic
stream directory in device memory: `nboxes` Str boxes of `lines` lines with `points` points and `ncomp` components, uniform values in
[0, 1) made on the device; node ids in storage order; element e on nodes e/2, e/2+1, e/2+2; the seed x of a line of box g lies in
[g, g+1) / nboxes, so the seed box x <= 0.25 keeps the elements of a quarter of the boxes.  Timed warm, with device events around `reps`
passes of each call (each ends in a stream synchronise; a plan is built and destroyed every pass, its allocations included).  Beside each
the bytes it must move, at 8 TB/s:
  select  the element table once, and per node the table entry and three seed coordinates
  plan    the selected connectivity read and written, the node table read and the new numbers written
  gather  the kept points of every component, read and written
and the same work on ONE host thread: tools/bench/streamsub_host.cpp, compiled here with g++ -O2, best of 3.
usage: python tools/streamsub_bench.py [nboxes=16] [lines=65536] [points=64] [ncomp=4] [nelts=2097152] [reps=10]   (a table and one JSON line)"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch first: one HIP runtime)

from peleanalysis_amd import capi  # noqa: E402

arg = lambda k, d: int(sys.argv[k]) if len(sys.argv) > k else d
nb, ni, nj, ncomp, nelts, reps = arg(1, 16), arg(2, 65536), arg(3, 64), arg(4, 4), arg(5, 2097152), arg(6, 10)
FRAC, HBM, NPE = 0.25, 8.0e12, 3
N = nb * ni

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "streamsub_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "bench", "streamsub_host.cpp"), "-o", exe])
    host = subprocess.run([exe, str(nb), str(ni), str(nj), str(ncomp), str(nelts), repr(FRAC), "3"], check=True, capture_output=True, text=True).stdout.split()
host_ms, host_counts = [float(v) for v in host[:3]], [int(v) for v in host[3:6]]

stream = torch.cuda.Stream()  # the library on a stream of torch's: torch's events time its launches
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)
box_desc = [(ni, nj, -(nj // 2), g * ni * nj) for g in range(nb)]
node_table = np.stack([np.repeat(np.arange(nb, dtype=np.int32), ni), np.tile(np.arange(ni, dtype=np.int32), nb)], 1)
sel = capi.StreamSel(ctx, box_desc, node_table)
gen = torch.Generator(device="cuda").manual_seed(1)
data = torch.rand((nb, ncomp, nj, ni), device="cuda", dtype=torch.float64, generator=gen)
data[:, 0, nj // 2, :] = (torch.arange(nb, device="cuda", dtype=torch.float64)[:, None] + data[:, 0, nj // 2, :]) / nb
e = torch.arange(nelts, device="cuda", dtype=torch.int64)
face = (((e // 2)[:, None] + torch.arange(NPE, device="cuda")) % N + 1).to(torch.int32).contiguous()
elts = torch.full((nelts,), -1, device="cuda", dtype=torch.int32)
out = torch.empty(ncomp * N * nj // 2, device="cuda", dtype=torch.float64)  # room for half of the boxes
torch.cuda.synchronize()
vp, nsel = C.c_void_p, C.c_int64(0)
lo, hi = (C.c_double * 3)(0.0, 0.0, 0.0), (C.c_double * 3)(FRAC, 1.0, 1.0)
comps = (C.c_int32 * ncomp)(*range(ncomp))
state = {"plan": None}


def select():
    ctx.check(ctx.lib.pa_ssub_select_seedbox(ctx.h, sel.h, vp(data.data_ptr()), ncomp, nelts, NPE, vp(face.data_ptr()), lo, hi, vp(elts.data_ptr()), C.byref(nsel), None))


def plan():
    if state["plan"]:
        ctx.lib.pa_ssub_destroy(state["plan"])
    state["plan"] = ctx.lib.pa_ssub_plan(ctx.h, sel.h, nelts, NPE, vp(face.data_ptr()), nsel.value, vp(elts.data_ptr()))
    if not state["plan"]:
        raise capi.PaError(ctx.lib.pa_last_error(ctx.h).decode())


def gather():
    ctx.check(ctx.lib.pa_ssub_gather(ctx.h, state["plan"], vp(data.data_ptr()), ncomp, ncomp, comps, vp(out.data_ptr()), ncomp, 0))


def whole():
    select()
    plan()
    gather()


def timed(fn):
    fn()
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


t_sel = timed(select)
t_plan = timed(plan)
counts = (C.c_int64 * 3)()
ctx.lib.pa_ssub_counts(state["plan"], counts)
if counts[2] * ncomp > out.numel():
    raise SystemExit("the selection keeps more than half of the boxes")
t_gat = timed(gather)
t_all = timed(whole)
b_sel = 4.0 * nelts * NPE + N * (8.0 + 24.0)
b_plan = 2 * 4.0 * nsel.value * NPE + N * (8.0 + 4.0)
b_gat = 2 * 8.0 * ncomp * counts[2]
rows = [("select by seed box", t_sel, b_sel, host_ms[0]), ("plan", t_plan, b_plan, host_ms[1]), ("gather", t_gat, b_gat, host_ms[2]),
        ("the three calls", t_all, b_sel + b_plan + b_gat, sum(host_ms))]
print(f"{N} lines of {nj} points in {nb} boxes, {ncomp} components, {nelts} elements; kept on the device: {nsel.value} elements, {counts[0]} boxes, {counts[2]} points; "
      f"in the host run: {host_counts[0]} elements, {host_counts[1]} boxes, {host_counts[2]} points")
print(f"{'call':22s} {'ms':>9s} {'MB to move':>11s} {'floor ms':>9s} {'one host thread ms':>19s}")
for name, ms, b, h in rows:
    print(f"{name:22s} {ms:9.4f} {b / 1e6:11.1f} {1e3 * b / HBM:9.4f} {h:19.2f}")
print(json.dumps({"lines": N, "points": nj, "boxes": nb, "ncomp": ncomp, "elements": nelts, "reps": reps, "kept_elements": nsel.value, "kept_boxes": counts[0], "kept_points": counts[2],
                  "host_kept": host_counts, "rows": [{"call": n, "ms": ms, "floor_ms": 1e3 * b / HBM, "host_one_thread_ms": h} for n, ms, b, h in rows]}))
ctx.lib.pa_ssub_destroy(state["plan"])
sel.close()
