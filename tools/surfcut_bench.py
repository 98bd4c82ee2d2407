#!/usr/bin/env python3
"""Timing harness of the surface cutting and trimming path (pa_surfcut.hip; sliceMEF3d, trimMEFgen3d) on the lines of the other
tools/*_bench.py.  The surface is synthetic: an icosphere subdivided `level` times (level 9: 5.24 M triangles, 2.62 M nodes) with 8 node
components: x, y, z, a smooth wavy field sin(40 x) sin(40 y) sin(40 z) (component 3: many long contour lines), and four random ones.
Timed:
  slice          pa_surf_slice, warm, `reps` back-to-back calls between device events on the context's stream, for three cuts: the
                 plane z = 0.1 (a few thousand segments), the wavy field at 0 (some 10^5 segments) and a random field at 0 (about
                 half of all elements cut: the most requests the sorts can see).  The call is synchronous -- two counts are read back
                 on the way -- so the figure is the kernel chain with those two round trips, not the sum of the kernel times.
  trim           one pa_surf_trim (z < 0 removed), wall clock: flags, three scans, gathers, two allocations
  area           one pa_surf_area, wall clock
  tools          sliceMEF3d.ex (dir=2 locs=0.1) and trimMEFgen3d.ex (comps=2 signs=lt vals=0) end to end, wall clock: HIP start-up, reading
                 the MEF, the upload and writing the results are in these figures
  host assembly  tools/src/contourCheck.cpp `time`: the first phase of tools/common/pa_contour.h by the CSR (its host-side build
                 included) against the plain list scan (the reference's FindMySeg loop), and the join phase both share, on the
                 segments of the plane cut (whole) and of the wavy cut.  The list scan is quadratic: on the wavy cut it is given the
                 first `scan_segs` segments only (the JSON says how many), the CSR walk the same prefix and the whole set.
Next to each slice the bytes the chain must move at least at 8 TB/s.
usage: python tools/surfcut_bench.py [level=9] [reps=10] [scan_segs=50000] [out=profiles/surfcut_bench.json] [kernels]
`kernels`: the device part only, with the random cut alone (the most requests), for rocprofv3 --kernel-trace --stats -- python3 ...: the
kernel times of profiles/surfcut_kernel_stats.txt."""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (torch first: one HIP runtime)

import decimate_cases as DC  # noqa: E402
import surfcut_ref as R  # noqa: E402
from peleanalysis_amd import capi  # noqa: E402

level = int(sys.argv[1]) if len(sys.argv) > 1 else 9
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
scan_segs = int(sys.argv[3]) if len(sys.argv) > 3 else 50000
out_json = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "surfcut_bench.json")
kernels_only = len(sys.argv) > 5 and sys.argv[5] == "kernels"  # under rocprofv3 --kernel-trace --stats: the random cut, area and trim only
HBM, NC = 8.0e12, 8


def icosphere(lv):
    """DC.icosphere's subdivision in numpy (the same midpoints; the node order differs)"""
    x, e = DC.icosphere(0)
    v, f = x.copy(), (e - 1).astype(np.int64)
    for _ in range(lv):
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        p = np.concatenate([a, b, c])
        q = np.concatenate([b, c, a])
        n = len(v)
        uk, inv = np.unique(np.minimum(p, q) * n + np.maximum(p, q), return_inverse=True)
        mid = v[uk // n] + v[uk % n]
        mid /= np.linalg.norm(mid, axis=1)[:, None]
        ids = n + inv
        m = len(f)
        ab, bc, ca = ids[:m], ids[m:2 * m], ids[2 * m:]
        f = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1), np.stack([ab, bc, ca], 1)])
        v = np.vstack([v, mid])
    return v, (f + 1).astype(np.int32)


xyz, elts = icosphere(level)
rng = np.random.default_rng(1)
nodes = np.hstack([xyz, (np.sin(40 * xyz[:, 0]) * np.sin(40 * xyz[:, 1]) * np.sin(40 * xyz[:, 2]))[:, None], rng.uniform(-1, 1, size=(len(xyz), NC - 4))])
nodes = np.ascontiguousarray(nodes)
nN, nE = len(nodes), len(elts)
print(f"icosphere level {level}: {nN} nodes, {nE} triangles, {NC} components ({nodes.nbytes / 1e6:.0f} MB of nodes, {elts.nbytes / 1e6:.0f} MB of elements)")

stream = torch.cuda.Stream()  # the library on a stream of torch's: torch's events time its launches
torch.cuda.set_stream(stream)
ctx = capi.Context(0, stream.cuda_stream)


def timed(fn, nrep):
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


res = {"surface": f"icosphere level {level}", "nodes": nN, "triangles": nE, "ncomp": NC, "reps": reps, "slices": [], "host_assembly": []}
t0 = time.perf_counter()
S = capi.Surf(ctx, nodes, elts)
res["create_upload_ms"] = 1e3 * (time.perf_counter() - t0)
cuts = {}
print(f"{'slice':26s} {'segments':>9s} {'vertices':>9s} {'ms':>9s} {'floor MB':>9s} {'floor ms':>9s} {'ratio':>7s}")
CUTS = (("plane z = 0.1", 2, 0.1), ("wavy field = 0", 3, 0.0), ("random field = 0", 5, 0.0))
for name, comp, loc in (CUTS[2:] if kernels_only else CUTS):
    nv, ns = S.slice(comp, loc)
    ms = timed(lambda: S.slice(comp, loc), reps)
    # least traffic: the triples and one value per corner (20 B / element); per request a key, a pair and an index written, read by the
    # sort and written again (2 * 20 B), the id scattered back and the CSR entry (8 B); per vertex 2 nodes x ncomp read, ncomp written
    floor = 20.0 * nE + 2 * ns * (2 * 20.0 + 8.0) + nv * 3 * 8.0 * NC
    fl = 1e3 * floor / HBM
    print(f"{name:26s} {ns:9d} {nv:9d} {ms:9.4f} {floor / 1e6:9.1f} {fl:9.4f} {ms / fl:7.1f}")
    res["slices"].append({"cut": name, "comp": comp, "loc": loc, "segments": ns, "vertices": nv, "ms": ms, "floor_bytes": floor, "floor_ms": fl, "ratio": ms / fl})
    if comp != 5:
        cuts[name] = (nv, S.slice_read()[2])
t0 = time.perf_counter()
S.area()
res["area_ms"] = 1e3 * (time.perf_counter() - t0)
t0 = time.perf_counter()
S.area()
res["area_warm_ms"] = 1e3 * (time.perf_counter() - t0)
t0 = time.perf_counter()
unused = S.trim([(2, "lt", 0.0)])
res["trim_ms"] = 1e3 * (time.perf_counter() - t0)
res["trim_out"] = dict(zip(("nodes", "triangles", "ncomp"), S.counts()))
res["trim_floor_ms"] = 1e3 * (8.0 * nN + 12.0 * nE + 8.0 * NC * (nN + S.counts()[0]) + 12.0 * (nE + S.counts()[1])) / HBM
print(f"area {res['area_ms']:.3f} ms (warm {res['area_warm_ms']:.3f}); trim z < 0: {res['trim_ms']:.3f} ms -> {res['trim_out']} ({unused} unused nodes), floor {res['trim_floor_ms']:.4f} ms")
S.close()
ctx.close()
if kernels_only:
    sys.exit(0)

# ---- the tools end to end, and the host line assembly
tmp = tempfile.mkdtemp(prefix="surfcut_bench_")
try:
    names = ["X", "Y", "Z", "wavy"] + ["f%d" % c for c in range(4, NC)]
    with open(os.path.join(tmp, "sphere.mef"), "wb") as fh:
        fh.write(R.mef_bytes(nodes, elts, "0.125", names))
    BIN = os.path.join(ROOT, "tools", "bin")
    res["tools"] = {}
    for exe, args in (("sliceMEF3d.ex", ["infile=sphere.mef", "dir=2", "locs=0.1"]), ("trimMEFgen3d.ex", ["infile=sphere.mef", "outfile=trimmed.mef", "comps=2", "signs=lt", "vals=0"])):
        best = None
        for _ in range(2):
            t0 = time.perf_counter()
            r = subprocess.run([os.path.join(BIN, exe)] + args, cwd=tmp, capture_output=True, text=True, timeout=600)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr
            best = dt if best is None else min(best, dt)
        res["tools"][exe] = {"args": " ".join(args), "seconds": best, "input_MB": os.path.getsize(os.path.join(tmp, "sphere.mef")) / 1e6}
        print(f"{exe} {' '.join(args)}: {best:.3f} s end to end (best of 2)")
    cc = os.path.join(tmp, "contourCheck")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + ROOT, os.path.join(ROOT, "tools", "src", "contourCheck.cpp"), "-o", cc])

    def assemble(tag, nv, segs, scan):
        text = "%d %d\n" % (nv, len(segs)) + "".join("%d %d\n" % (l, r) for l, r in segs.tolist())
        r = subprocess.run([cc, "time"] + ([] if scan else ["noscan"]), input=text, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr
        w = r.stdout.split()
        row = {"segments_of": tag, "segments": len(segs), "csr_walk_ms": float(w[1]), "list_scan_walk_ms": float(w[3]) if scan else None, "join_ms": float(w[5]),
               "fragments": int(w[7]), "lines": int(w[9])}
        res["host_assembly"].append(row)
        print(f"host assembly, {tag}: {len(segs)} segments, {row['fragments']} fragments, {row['lines']} lines: CSR build + walk {row['csr_walk_ms']:.3f} ms, list-scan walk "
              + (f"{row['list_scan_walk_ms']:.3f} ms" if scan else "not run (quadratic)") + f", join (shared) {row['join_ms']:.3f} ms")

    nv, segs = cuts["plane z = 0.1"]
    assemble("plane z = 0.1 (whole)", nv, segs, True)
    nv, segs = cuts["wavy field = 0"]
    assemble("wavy field = 0, first %d segments" % min(scan_segs, len(segs)), nv, segs[:scan_segs], True)
    assemble("wavy field = 0 (whole)", nv, segs, False)
    res["host_assembly_note"] = ("the list-scan walk is quadratic: on the wavy cut it ran on the first %d of %d segments only; "
                                 "a prefix is a soup of many fragments, so its join time is not the whole cut's" % (min(scan_segs, len(segs)), len(segs)))
finally:
    shutil.rmtree(tmp, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(out_json)), exist_ok=True)
with open(out_json, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
print(json.dumps(res))
