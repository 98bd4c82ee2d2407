#!/usr/bin/env python3
"""Timing harness of the peak-and-gather pass of streamScatter3d (pa_streamsel.hip: pa_ssel_peaks, the counting call of
pa_ssel_scatter, pa_ssel_scatter) on synthetic lines in device memory: `nboxes` Str boxes of `lines` lines with `points` points, the
conditioning component and `nvars` variables, uniform values in [0, 1) made on the device; node ids in storage order.  The range
[0.98, 0.99) keeps about a quarter of the lines of 64 points.  Timed warm, with device events around `reps` passes of the three
calls (each ends in a stream synchronise).  Beside it the same loop on ONE host thread: tools/bench/streamsel_host.cpp, compiled
here with g++ -O2, over data of the same shape and distribution (its own generator: the kept lines differ, their share does not).
The READ FLOOR is the conditioning component read once at 8 TB/s.
usage: python tools/streamsel_bench.py [nboxes=16] [lines=65536] [points=64] [nvars=3] [reps=10]   (prints a table and one JSON line)"""
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

nb = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ni = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
nj = int(sys.argv[3]) if len(sys.argv) > 3 else 64
nv = int(sys.argv[4]) if len(sys.argv) > 4 else 3
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 10
MORE, LESS, HBM = 0.98, 0.99, 8.0e12
N, ncomp = nb * ni, 1 + nv

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "streamsel_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "bench", "streamsel_host.cpp"), "-o", exe])
    host = subprocess.run([exe, str(nb), str(ni), str(nj), str(nv), repr(MORE), repr(LESS), "3"], check=True, capture_output=True, text=True).stdout.split()
host_ms, host_kept = float(host[0]), int(host[1])

stream = torch.cuda.Stream()  # the library on a stream of torch's: torch's events time its launches
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)
box_desc = [(ni, nj, -(nj // 2), g * ni * nj) for g in range(nb)]
node_table = np.stack([np.repeat(np.arange(nb, dtype=np.int32), ni), np.tile(np.arange(ni, dtype=np.int32), nb)], 1)
sel = capi.StreamSel(ctx, box_desc, node_table)
data = torch.rand(nb * ncomp * ni * nj, device="cuda", dtype=torch.float64, generator=torch.Generator(device="cuda").manual_seed(1))
jpeak, hival = capi.DevBuf(ctx, 4 * N), capi.DevBuf(ctx, 8 * N)
out = capi.DevBuf(ctx, 8 * N * max(nv, 1))
comps = (C.c_int32 * max(nv, 1))(*range(1, 1 + nv))
vp, kept = C.c_void_p, C.c_int64(0)


def peaks():
    ctx.check(ctx.lib.pa_ssel_peaks(ctx.h, sel.h, vp(data.data_ptr()), ncomp, 0, vp(jpeak.ptr), vp(hival.ptr)))


def count():
    ctx.check(ctx.lib.pa_ssel_scatter(ctx.h, sel.h, None, ncomp, 0, None, None, vp(hival.ptr), MORE, LESS, 0, 0, None, C.byref(kept)))


def gather():
    ctx.check(ctx.lib.pa_ssel_scatter(ctx.h, sel.h, vp(data.data_ptr()), ncomp, nv, comps, vp(jpeak.ptr), vp(hival.ptr), MORE, LESS, nv, 0, vp(out.ptr), C.byref(kept)))


def whole():
    peaks()
    count()
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


rows = [("peak of every line", timed(peaks), 8.0 * N * nj), ("count of the kept lines", timed(count), 8.0 * N), ("ordered gather", timed(gather), 8.0 * N),
        ("the three calls", timed(whole), 8.0 * N * nj)]
print(f"{N} lines of {nj} points, {nv} variables; {kept.value} lines kept on the device, {host_kept} in the host run")
print(f"{'call':28s} {'ms':>9s} {'MB read at least':>17s} {'floor ms':>9s}")
for name, ms, b in rows:
    print(f"{name:28s} {ms:9.4f} {b / 1e6:17.1f} {1e3 * b / HBM:9.4f}")
print(f"{'one host thread (g++ -O2)':28s} {host_ms:9.2f}")
print(json.dumps({"lines": N, "points": nj, "nvars": nv, "reps": reps, "kept_device": kept.value, "kept_host": host_kept, "host_one_thread_ms": host_ms,
                  "rows": [{"call": n, "ms": ms, "floor_ms": 1e3 * b / HBM} for n, ms, b in rows]}))
sel.close()
