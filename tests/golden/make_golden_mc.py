#!/usr/bin/env python3
"""Golden vectors for marching cubes, marching squares and the surface merge, produced by the REFERENCE's own code: the part
of Src/isosurface.cpp from Edge through Element, cut out and compiled in place into oracle/_ref/libiso_ref3.so / libiso_ref2.so
by `make -C oracle ref`.  Only runs where those libraries exist; the .npz holds data only -- per case the inputs (arrays where
small, a SHA-256 of their bytes otherwise) and the reference's per-FAB vertices, edge keys and elements, and for the hierarchy
cases the merged nodes and elements.  The file is written with fixed zip time stamps: a second run reproduces it byte for byte.
    python tests/golden/make_golden_mc.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from oracle import oracle as O  # noqa: E402
import mc_cases as M  # noqa: E402

MAX_BYTES = 567471  # the largest fixture the tree held before this one (gradcurv_amr3.npz)


def small_int(a):
    a = np.asarray(a)
    for dt in (np.int8, np.int16, np.int32):
        if a.size == 0 or (a.min() >= np.iinfo(dt).min and a.max() <= np.iinfo(dt).max):
            return a.astype(dt)
    raise ValueError("index beyond 32 bits")


def write_npz(path, d):
    """an .npz that numpy.load reads, with fixed time stamps; LZMA members (a quarter smaller than deflate on these arrays), integer
    tables column by column (the .npy header records the order: they load as they were)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_LZMA) as z:
        for k in sorted(d):
            a = np.asanyarray(d[k])
            if a.ndim == 2 and a.dtype.kind == "i":
                a = np.asfortranarray(a)
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_LZMA
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def record(c):
    dim, nc, k = c["dim"], c["nc"], c["name"]
    fab_ref = O.mc_fab_ref if dim == 3 else O.msq_fab_ref
    per_fab = []
    for fb in c["fabs"]:
        if np.any(fb["llo"] > fb["lhi"]):  # an empty loop box is skipped (no Polygonise call)
            per_fab.append((np.zeros((0, nc)), np.zeros((0, 2 * dim), np.int32), np.zeros((0, dim), np.int32)))
        else:
            per_fab.append(fab_ref(fb["state"], fb["mask"], fb["lo"], fb["hi"], c["isocomp"], c["iso"], fb["llo"], fb["lhi"]))
    d = {k + "_dim": np.int32(dim), k + "_nc": np.int32(nc), k + "_iso": np.float64(c["iso"]), k + "_sha": np.array(M.input_digest(c)),
         k + "_nv": small_int([len(v) for v, _, _ in per_fab]), k + "_ne": small_int([len(t) for _, _, t in per_fab]),
         k + "_V": np.concatenate([v for v, _, _ in per_fab]), k + "_K": small_int(np.concatenate([q for _, q, _ in per_fab])),
         k + "_T": small_int(np.concatenate([t for _, _, t in per_fab]))}
    uniq, imap = M.unique_inputs(M.input_arrays(c))
    if sum(a.size for a in uniq) <= M.SMALL_INPUT:
        d[k + "_nin"], d[k + "_inmap"] = np.int32(len(uniq)), small_int(imap)
        for q, a in enumerate(uniq):
            d[f"{k}_in{q}"] = a if a.dtype == np.float64 else small_int(a)
    else:
        d[k + "_nin"], d[k + "_inmap"] = np.int32(0), np.zeros(0, np.int8)
    note = ""
    if c["merge"]:
        fr = M.fragments(per_fab)
        res = O.iso_merge_ref(fr, nc, dim)
        if isinstance(res, str):
            raise SystemExit(f"{k}: the merge of this case is {res} (Node::operator< is no strict weak ordering on it): no such case may be in the matrix")
        nodes, elts = res
        fv = np.concatenate([v for v, _ in fr])
        # every node is a copy of one fragment vertex: keep its index, the first vertex with those bits
        first = {}
        for q, row in enumerate(fv.view(np.int64)):
            first.setdefault(row.tobytes(), q)
        src = np.array([first[row.tobytes()] for row in np.ascontiguousarray(nodes).view(np.int64)], dtype=np.int64)
        assert np.array_equal(fv[src].view(np.int64), np.ascontiguousarray(nodes).view(np.int64))
        d[k + "_msrc"], d[k + "_melts"] = small_int(src), small_int(elts)
        note = f", merge: {len(fv)} vertices -> {len(nodes)} nodes, {len(elts)} elements"
    print(f"{k}: {len(per_fab)} FABs, {sum(len(v) for v, _, _ in per_fab)} vertices, {sum(len(t) for _, _, t in per_fab)} elements{note}")
    return d


def main():
    O.build()
    if O.iso_ref_lib(3) is None or O.iso_ref_lib(2) is None:
        raise SystemExit("oracle/_ref/libiso_ref3.so / libiso_ref2.so are missing and /root/reference is not available")
    d, names = {}, []
    for c in M.cases(O):
        names.append(c["name"])
        d.update(record(c))
    d["names"] = np.array(names)
    out = M.golden_path()
    write_npz(out, d)
    size = os.path.getsize(out)
    print("wrote", out, size, "bytes")
    if size > MAX_BYTES:
        raise SystemExit(f"{size} bytes: larger than the largest fixture so far ({MAX_BYTES})")


if __name__ == "__main__":
    main()
