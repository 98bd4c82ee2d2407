#!/usr/bin/env python3
"""Timing harness of the hex-element mesh kernels (pa_amrtofe.hip; the device work of amrToFE3d) on a 3-level nested_hierarchy at base
n^3 (every level n^3 cells in boxes of 64^3, the central half of each level refined, non-periodic), two components gathered.
The stages are timed with HIP events inside the library (pa_fe_stage_times): number (count pass, scan of the block sums, id pass), tag,
cubes (count pass, scan, the host's read of the count, emit pass), order (node keys, node sort,
ranks, four key-gather + radix-sort passes over the cubes, first-occurrence count, scan, emit) and gather.  Each figure is the minimum
of `reps` builds after one warm-up build (the first build grows the context's two scratch buffers; later builds allocate only their results).
BYTES MODEL (what each stage has to move if every array is touched once per pass; cells V, grown cells G, nodes N, cubes M, elements E,
b = ceil(bits / 8) radix passes of a sort over `bits` key bits):
  number  4 V (id map) + 20 N (node table); the count pass reads only the owner maps
  tag     4 G (tags) + 4 G (gathered ids)
  cubes   2 * 4 G (the tags, once per pass; the other seven reads of a cube hit lines a neighbour loaded) + 32 M (cube list)
  order   nodes: 12 N (keys, ids) + b_n * 2 * 12 N + 8 N (ranks); per cube pass (4 of them): 4 M (order) + 8 M (two ids) + 8 M (two
          gathered ranks) + 8 M (key) + b_c * 2 * 12 M; unique: 2 * (4 + 32) M (two passes; the predecessor's row is the neighbour's)
          + 32 E
  gather  20 N (node table) + 8 nc N (gathered values) + 8 (3 + nc) N (block-ordered output)
and is compared with 8 TB/s.
usage: python tools/amrtofe_bench.py [n=128] [reps=3]   (prints a table and one JSON line)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (torch first: one HIP runtime)

from peleanalysis_amd import capi  # noqa: E402
from peleanalysis_amd.hierarchy import nested_hierarchy  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 128
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
NC = 2
ctx = capi.Context(0)
H = nested_hierarchy(n, 3, min(64, n), is_per=(0, 0, 0))
dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
mfs = [capi.DevMF(ctx, dl, NC, 0) for dl in dls]
for m in mfs:
    m.setval(1.0)
V = sum(lv.ncells for lv in H.levels)
G = sum(int(((lv.boxes[:, 3:].astype("int64") - lv.boxes[:, :3] + 3).prod(axis=1)).sum()) for lv in H.levels)

best, sizes = None, None
for rep in range(1 + reps):
    with capi.FeMesh(ctx, dls, [2, 2]) as fe:
        buf = fe.gather(mfs, list(range(NC)), download=False)
        ms, cubes = fe.stage_times()
        sizes = (fe.nnodes, cubes, fe.nelts)
        del buf
    if rep:
        best = ms if best is None else {k: min(best[k], ms[k]) for k in ms}
N, M, E = sizes
bits = lambda x: max(1, (x - 1).bit_length())
bn = -(-(3 * bits(4 * n) + bits(3)) // 8)
bc = -(-(2 * bits(N)) // 8)
model = {"number": 4 * V + 20 * N,
         "tag": 8 * G,
         "cubes": 8 * G + 32 * M,
         "order": 12 * N + bn * 24 * N + 8 * N + 4 * (28 * M + bc * 24 * M) + 72 * M + 32 * E,
         "gather": 20 * N + 8 * NC * N + 8 * (3 + NC) * N}
total = sum(best.values())
out = {"n": n, "reps": reps, "cells": V, "grown_cells": G, "nodes": N, "cubes": M, "elements": E, "ms": best, "bytes": model, "total_ms": total,
       "nodes_per_s": N / (total * 1e-3), "elements_per_s": E / (total * 1e-3)}
print(f"amrtofe_bench: 3 levels of {n}^3 cells: {V} cells, {G} grown cells, {N} nodes, {M} cubes before duplicate removal, {E} elements; min of {reps} builds")
print(f"{'stage':>8s} {'ms':>9s} {'share':>6s} {'model MB':>10s} {'GB/s':>8s} {'of 8 TB/s':>9s}")
for k in capi.FeMesh.STAGES:
    gbs = model[k] / (best[k] * 1e-3) / 1e9 if best[k] > 0 else 0.0
    print(f"{k:>8s} {best[k]:9.3f} {100 * best[k] / total:5.1f}% {model[k] / 1e6:10.1f} {gbs:8.1f} {100 * gbs / 8000:8.2f}%")
print(f"{'total':>8s} {total:9.3f}   {N / (total * 1e-3) / 1e6:.1f} Mnodes/s   {E / (total * 1e-3) / 1e6:.1f} Melements/s")
print(json.dumps(out))
for m in mfs:
    m.close()
for dl in dls:
    dl.close()
ctx.close()
