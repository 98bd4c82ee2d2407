#!/usr/bin/env python3
"""Timing harness of the surface merge (pa_surfjoin.hip; mergeMEF3d) on the lines of the other tools/*_bench.py.  The input is
synthetic: the two halves of an n x n grid patch with a smooth bump in z, cut at the middle column, each half with its own copy of the
seam column (n = 448: 101,025 nodes and 200,704 triangles per half, 449 coincident nodes), 5 node components.  remDupNodes = 1.
Timed, at eps = 1e-8 and at eps = 10 x the node spacing (the dense-cell regime: hundreds of nodes per cell, thousands of duplicates):
  grid, brute    pa_surfjoin_merge with method = 1 and method = 2: a host clock around the call, which is synchronous (it ends in a stream
                 synchronise); the upload of the two handles is outside the window, the re-layout of M into its new allocation inside
  baseline       the reference's double loop (mergeMEF.cpp:186-208) restated in tools/bench/merge_loop_baseline.cpp, compiled here with
                 g++ -O2, serial as the reference: what a user of the reference waits for.  Never the code under test.
Before anything is timed the three results are checked equal: the two device surfaces byte for byte, and the baseline's node ids
against the device's appended elements.  Two warm-up merges per path, then `reps` timed ones (a fresh M each: the merge replaces it),
alternating the paths; median, minimum and maximum are reported.  The gate: every grid time below every brute-force time.
usage: python tools/surfjoin_bench.py [n=448] [reps=7] [out=profiles/surfjoin_bench.json] [kernels]
`kernels`: one merge per path and eps only, for rocprofv3 --kernel-trace --stats -- python3 ...: profiles/surfjoin_kernel_stats.txt."""
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (torch first: one HIP runtime)

from peleanalysis_amd import capi  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 448
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
out_json = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "surfjoin_bench.json")
kernels_only = len(sys.argv) > 4 and sys.argv[4] == "kernels"
NC = 5
assert n % 2 == 0 and reps >= 5


def half(i0, i1, seed):
    """columns i0 .. i1 of the (n + 1) x (n + 1) node grid, two triangles per quad"""
    w = i1 - i0 + 1
    jj, ii = np.meshgrid(np.arange(n + 1), np.arange(i0, i1 + 1), indexing="ij")
    x, y = ii.ravel() / n, jj.ravel() / n
    z = 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)
    rng = np.random.default_rng(seed)
    nodes = np.ascontiguousarray(np.stack([x, y, z] + [rng.uniform(-1, 1, len(x)) for _ in range(NC - 3)], axis=1))
    j, i = np.meshgrid(np.arange(n), np.arange(w - 1), indexing="ij")
    p = (j * w + i).ravel()
    e = np.concatenate([np.stack([p, p + 1, p + w + 1], 1), np.stack([p, p + w + 1, p + w], 1)]) + 1
    return nodes, np.ascontiguousarray(e.astype(np.int32))


(a, ea), (b, eb) = half(0, n // 2, 1), half(n // 2, n, 2)
print(f"two halves of the {n} x {n} patch: {len(a)} + {len(b)} nodes, {len(ea)} + {len(eb)} triangles, {NC} components, {n + 1} seam nodes")
ctx = capi.Context(0)


def merge_once(eps, method, read=False):
    with capi.Surf(ctx, a, ea) as m, capi.Surf(ctx, b, eb) as s:
        ctx.sync()
        t0 = time.perf_counter()
        m.merge(s, eps, True, method)
        dt = 1e3 * (time.perf_counter() - t0)
        return dt, m.last_launch(), (m.read() if read else None)


res = {"surface": f"halves of the {n} x {n} grid patch", "nodes": [len(a), len(b)], "triangles": [len(ea), len(eb)], "ncomp": NC, "spacing": 1.0 / n, "reps": reps,
       "timing": "host clock around the synchronous call, ms; median [min, max] of reps after 2 warm-up calls, paths alternating", "runs": []}
tmp = tempfile.mkdtemp(prefix="surfjoin_bench_")
try:
    base = os.path.join(tmp, "merge_loop_baseline")
    if not kernels_only:
        subprocess.check_call(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "bench", "merge_loop_baseline.cpp"), "-o", base])
        for tag, x in (("M", a), ("S", b)):
            with open(os.path.join(tmp, tag + ".bin"), "wb") as fh:
                fh.write(np.int64(len(x)).tobytes() + np.ascontiguousarray(x[:, :3].T).tobytes())
    for label, eps in (("eps = 1e-8", 1.0e-8), ("eps = 10 x spacing", 10.0 / n)):
        (_, rg, g), (_, rb, br) = merge_once(eps, 1, True), merge_once(eps, 2, True)
        assert rg["path"] == "grid" and rb["path"] == "brute", (rg, rb)
        assert g[0].tobytes() == br[0].tobytes() and g[1].tobytes() == br[1].tobytes(), "the two device paths differ"
        row = {"eps": eps, "label": label, "duplicates": rg["duplicates"], "nodes_appended": rg["nodes_appended"], "table": rg["table"], "results_equal": True}
        if kernels_only:
            res["runs"].append(row)
            continue
        r = subprocess.run([base, os.path.join(tmp, "M.bin"), os.path.join(tmp, "S.bin"), repr(eps), "5", os.path.join(tmp, "new.bin")],
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
        tb = [float(v) for v in r.stdout.split()]
        new_nodes = np.fromfile(os.path.join(tmp, "new.bin"), dtype=np.int32)
        assert np.array_equal(g[1][len(ea):], new_nodes[eb - 1] + 1) and len(g[0]) == len(a) + int((new_nodes >= len(a)).sum()), "the baseline differs from the device"
        merge_once(eps, 1), merge_once(eps, 2)
        tg, tbr = [], []
        for _ in range(reps):
            tg.append(merge_once(eps, 1)[0])
            tbr.append(merge_once(eps, 2)[0])
        for key, t in (("grid_ms", tg), ("brute_ms", tbr), ("baseline_ms", tb)):
            row[key] = {"median": statistics.median(t), "min": min(t), "max": max(t), "all": t}
        row["grid_faster_than_brute"] = max(tg) < min(tbr)
        row["kernels"] = {"grid": rg["kernels"], "brute": rb["kernels"]}
        res["runs"].append(row)
        print(f"{label}: {row['duplicates']} duplicates; grid {row['grid_ms']['median']:.3f} ms [{min(tg):.3f}, {max(tg):.3f}], brute force {row['brute_ms']['median']:.3f} ms "
              f"[{min(tbr):.3f}, {max(tbr):.3f}], host loop {row['baseline_ms']['median']:.1f} ms [{min(tb):.1f}, {max(tb):.1f}]; gate {'met' if row['grid_faster_than_brute'] else 'MISSED'}")
finally:
    shutil.rmtree(tmp, ignore_errors=True)
ctx.close()
if kernels_only:
    sys.exit(0)
res["gate"] = all(r["grid_faster_than_brute"] for r in res["runs"])
os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
with open(out_json, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
sys.exit(0 if res["gate"] else 3)
