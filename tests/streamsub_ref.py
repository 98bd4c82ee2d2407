"""CPU restatement (plain Python: literal loops, a set per level, a dict for the renumbering) of the subsetting of a stream directory by
surface elements, Src/streamSub.cpp of the reference, as streamSub3d builds it: the reference's evident INTENT where its text is
defective, its literal text where that is defined.  Shares no code with pa_streamsub.hip, tools/common/pa_streamsub.h or the driver.
Not a test module: test_streamsub_ref.py (CPU) and test_gpu_streamsub.py (GPU, exactly / byte for byte) import it.

The semantics, restated from the issue that asked for the tool (streamSub3d):
  1. the element list E (0-based file indices): eltIDs in the given order, duplicates repeating the element; or sElt .. sElt + nElt - 1
     (defaults 0, 1); or -- new keys -- the elements whose every node has its seed point (components 0, 1, 2 at j = 0 of the node's line)
     inside seedLo .. seedHi, literal <= on both sides, ascending.  An id outside 0 .. nElts-1 and an empty list abort.
  2. faceSel[j * npe + i] = fileFace[E[j] * npe + i]                      (the intent of :337-343)
  3. a box is needed iff it lists a node of faceSel; needed boxes are kept whole, ascending within a level   (:375-395)
  4. new node numbers: 1-based, consecutive over the kept boxes, level -> box -> position                    (:417-425)
  5. faceSel through the new numbers (:439-441); the box indices of Elements are the compacted ones          (:427-437, :495-505)
  6. comps: the file components whose name is listed, in the FILE's order; the Header lists them in that order
  7. outfile: infile split at '.', the last token dropped if there are several, rejoined, + "_new"            (:88-93)
  8. a level without a needed box gets the format's placeholder: one null box (0,0,0)..(0,0,0) of zeros that lists no id, as stream.cpp
     writes for a box without lines (every reader of the family knows it; streamTubeStats3d refuses a level 0 without any box)
`literal_needed` restates the reference's TEXT of :337-343 and :380-388 and raises where that text indexes out of bounds.

Two files of the result are not taken from streamsel_ref.write_files: Elements (write_files fixes three nodes per element) and the Str_H
of every level (its minima / maxima are numpy's, a NaN poisons them; the project's writer folds with literal < from +-1e300 in four
interleaved lanes, restated in `fold_min_max`; the matrix holds NaN, -0.0 next to +0.0 and infinities).  test_streamsub_ref.py holds the
two writers to each other where they must agree."""
from __future__ import annotations

import numpy as np

import streamsample_ref as S
import streamsel_ref as R

PLANTS = ("zero_based", "first_use_order", "referenced_only", "user_order_names", "last_wins", "old_box_ids", "sorted_elements")


class SubAbort(RuntimeError):
    pass


class LiteralOutOfBounds(RuntimeError):
    """the reference's text indexes outside an array here"""


# ------------------------------------------------------------------------------------------------ the keys
def default_outfile(infile):
    """:88-93"""
    tokens = infile.split(".")
    outfile = tokens[0]
    for i in range(1, len(tokens) - 1):
        outfile += "." + tokens[i]
    return outfile + "_new"


def element_list(nElts, eltIDs=None, sElt=None, nElt=None, seedLo=None, seedHi=None):
    """:103-118 and the seed keys -> ("seed", lo, hi) or ("list", E)"""
    if seedLo is not None or seedHi is not None:
        if seedLo is None or seedHi is None:
            raise SubAbort("seedLo and seedHi must come together")
        if eltIDs is not None or sElt is not None or nElt is not None:
            raise SubAbort("seedLo / seedHi exclude eltIDs, sElt and nElt")
        if len(seedLo) != 3 or len(seedHi) != 3:
            raise SubAbort("seedLo and seedHi take three values each")
        return ("seed", [float(v) for v in seedLo], [float(v) for v in seedHi])
    E = []
    if eltIDs is not None and len(eltIDs) > 0:
        for e in eltIDs:
            E.append(int(e))
    else:
        s = 0 if sElt is None else int(sElt)
        n = 1 if nElt is None else int(nElt)
        if n <= 0:
            raise SubAbort("nElt = %d: no element is selected" % n)
        for i in range(n):
            E.append(s + i)
    for e in E if eltIDs else sorted(E):  # the range is refused at its first id outside, the list at the first in its own order
        if e < 0 or e >= nElts:
            raise SubAbort("element id %d outside 0 .. %d" % (e, nElts - 1))
    return ("list", E)


def select_comps(names, comps=()):
    """:121-147 -> file component indices in the file's order; a name the file holds twice selects both"""
    comps = list(comps)
    if not comps:
        return list(range(len(names)))
    for j, n in enumerate(comps):
        if n in comps[:j]:
            raise SubAbort("Component given twice: " + n)
        if n not in names:
            raise SubAbort("Component not found: " + n)
    out = []
    for i, fn in enumerate(names):
        for n in comps:
            if fn == n:
                out.append(i)
    return out


# ------------------------------------------------------------------------------------------------ the tables
def check_tables(path, by_seed):
    """build_nodeMap (:228-250) with the sister tools' checks, the element table, and what the seed keys need -> nodeMap"""
    if sum(len(lev) for lev in path["levels"]) == 0:
        raise SubAbort("the stream file has no Str box")
    try:
        node_map = R.build_node_map(path)
    except R.SelAbort as e:
        raise SubAbort(str(e))
    for v in path["face"]:
        if int(v) < 1 or int(v) > len(node_map):
            raise SubAbort("Elements names node id %d outside 1 .. %d" % (int(v), len(node_map)))
    if by_seed:
        if len(path["names"]) < 3:
            raise SubAbort("seedLo / seedHi need the coordinates: the stream file has %d components" % len(path["names"]))
        for l, lev in enumerate(path["levels"]):
            for b, (lo, hi, _) in enumerate(lev):
                if len(path["ins"][l][b]) > 0 and (lo[1] > 0 or hi[1] < 0):
                    raise SubAbort("Str box %d of level %d (j = %d .. %d) has lines but no seed point j = 0" % (b, l, lo[1], hi[1]))
    return node_map


def seed_elements(path, node_map, lo, hi):
    """the elements whose every node's seed point lies in lo .. hi, ascending"""
    npe, face = path["npe"], path["face"]
    E = []
    for e in range(path["nElts"]):
        keep = True
        for i in range(npe):
            L, B, Pt = node_map[int(face[e * npe + i]) - 1]
            blo, _, a = path["levels"][L][B]
            for d in range(3):
                x = float(a[d, 0 - blo[1], Pt])
                if not (lo[d] <= x and x <= hi[d]):
                    keep = False
        if keep:
            E.append(e)
    return E


# ------------------------------------------------------------------------------------------------ the subset
def intent_needed(path, node_map, E, plant=None):
    """the intent of :337-343 and :380-388 -> (faceSel in file numbers, per level the needed boxes in the order of their first use)"""
    npe, fileFace = path["npe"], path["face"]
    if plant == "sorted_elements":
        E = sorted(set(E))
    faceSel = [0] * (len(E) * npe)
    for j in range(len(E)):
        for i in range(npe):
            faceSel[(0 if plant == "last_wins" else j * npe) + i] = int(fileFace[E[j] * npe + i])
    if plant == "last_wins":
        faceSel = faceSel[:npe]
    needed = [[] for _ in path["levels"]]
    for v in faceSel:
        lev, box, _ = node_map[v - 1]
        if box not in needed[lev]:
            needed[lev].append(box)
    return faceSel, needed


def literal_needed(path, node_map, eltIDs):
    """the reference's text of :337-343 and :380-388, index for index -> (faceData, needed); raises where it leaves an array"""
    npe, fileFaceData = path["npe"], path["face"]
    nElts = len(eltIDs)
    faceData = [0] * (nElts * npe)
    for j in range(nElts):
        for i in range(npe):
            if not 0 <= eltIDs[j] * npe + i < len(fileFaceData):
                raise LiteralOutOfBounds("fileFaceData[%d]" % (eltIDs[j] * npe + i))
            faceData[i] = int(fileFaceData[eltIDs[j] * npe + i])
    needed = [[] for _ in path["levels"]]
    for k in range(len(eltIDs)):
        eltID = eltIDs[k]
        offset = eltID * npe
        for i in range(npe):
            if not 0 <= offset + i < len(faceData):
                raise LiteralOutOfBounds("faceData[%d] of %d" % (offset + i, len(faceData)))
            n = faceData[offset + i] - 1
            if not 0 <= n < len(node_map):
                raise LiteralOutOfBounds("nodeMap[%d]" % n)
            lev, box, _ = node_map[n]
            if box not in needed[lev]:
                needed[lev].append(box)
    return faceData, needed


def finish(path, faceData, needed, comp_idx, plant=None):
    """:389-441 -> dict(face, kept [(lev, box)], newNum {old id: new}, inside [lev][new box], levels [lev][new box] = (lo, hi, a))"""
    nlev = len(path["levels"])
    boxIDs = []
    for lev in range(nlev):
        s = set(needed[lev])
        boxIDs.append(list(needed[lev]) if plant == "first_use_order" else sorted(s))  # the iteration of a std::set ascends
    file_inside = [[[int(v) for v in ids] for ids in per] for per in path["ins"]]
    used = set(faceData)
    newNum = {}
    cnt = 0 if plant == "zero_based" else 1
    for lev in range(nlev):
        for b in boxIDs[lev]:
            for v in file_inside[lev][b]:
                if plant == "referenced_only" and v not in used:
                    continue
                newNum[v] = cnt
                cnt += 1
    inside, levels, kept = [], [], []
    for lev in range(nlev):
        per, fabs = [], []
        for b in boxIDs[lev]:
            lo, hi, a = path["levels"][lev][b]
            ids = file_inside[lev][b]
            if plant == "referenced_only":
                cols = [k for k, v in enumerate(ids) if v in used]
                ids = [ids[k] for k in cols]
                a = a[:, :, cols]
                hi = (len(cols) - 1, hi[1], hi[2])
            per.append([newNum[v] for v in ids])
            fabs.append((tuple(lo), tuple(hi), np.ascontiguousarray(a[comp_idx])))
            kept.append((lev, b))
        inside.append(per)
        levels.append(fabs)
    return dict(face=[newNum[v] for v in faceData], kept=kept, newNum=newNum, inside=inside, levels=levels, boxIDs=boxIDs)


def subset(path, E, comp_idx=None, plant=None):
    """semantics 2 - 5 for the element list E"""
    if len(E) == 0:
        raise SubAbort("no element is selected")
    for e in E:
        if e < 0 or e >= path["nElts"]:
            raise SubAbort("element id %d outside 0 .. %d" % (e, path["nElts"] - 1))
    node_map = check_tables(path, False)
    faceSel, needed = intent_needed(path, node_map, E, plant)
    if comp_idx is None:
        comp_idx = list(range(len(path["names"])))
    out = finish(path, faceSel, needed, comp_idx, plant)
    out["faceSel_file"] = faceSel
    return out


# ------------------------------------------------------------------------------------------------ the files
def fold_min_max(values):
    """the minimum and maximum of a component as the project's VisMF writer folds them: from +1e300 / -1e300, literal <, four interleaved
    lanes (the tail in lane 0), the lanes combined in order.  A NaN never wins; of -0.0 and +0.0 the first seen in its lane stays"""
    n = len(values)
    a = [1e300] * 4
    b = [-1e300] * 4
    i = 0
    while i + 4 <= n:
        for q in range(4):
            v = values[i + q]
            a[q] = v if v < a[q] else a[q]
            b[q] = v if b[q] < v else b[q]
        i += 4
    while i < n:
        v = values[i]
        a[0] = v if v < a[0] else a[0]
        b[0] = v if b[0] < v else b[0]
        i += 1
    mn, mx = 1e300, -1e300
    for q in range(4):
        mn = a[q] if a[q] < mn else mn
        mx = b[q] if mx < b[q] else mx
    return mn, mx


def str_header(fabs, ncomp, fname="Str_D_00000"):
    """the Str_H of one level (VisMF, one data file, no ghost cells)"""
    offs, at = [], 0
    for lo, hi, a in fabs:
        offs.append(at)
        at += len("FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))" + R.G._box_str(lo, hi) + " %d\n" % ncomp) + 8 * a.size
    nb = len(fabs)
    h = "1\n1\n%d\n0\n(%d 0\n" % (ncomp, nb)
    for lo, hi, _ in fabs:
        h += R.G._box_str(lo, hi) + "\n"
    h += ")\n%d\n" % nb
    for o in offs:
        h += "FabOnDisk: %s %d\n" % (fname, o)
    folds = [[fold_min_max([float(v) for v in a[c].ravel()]) for c in range(ncomp)] for _, _, a in fabs]
    for which in (0, 1):
        h += "\n%d,%d\n" % (nb, ncomp)
        for f in folds:
            h += "".join("%.17g," % f[c][which] for c in range(ncomp)) + "\n"
    return h.encode()


def elements_text(face, nElts, inside):
    """:473-507"""
    nodesPerElt = len(face) // nElts
    e = "%d\n%d\n" % (nElts, nodesPerElt)
    for v in face:
        e += "%d " % v
    e += "\n"
    for per in inside:
        e += "%d\n" % sum(1 for ids in per if len(ids) > 0)
        for j, ids in enumerate(per):
            if len(ids) > 0:
                e += "%d %d" % (j, len(ids)) + "".join(" %d" % v for v in ids) + "\n"
    return e.encode()


def dir_files(names, levels, ins, face, nElts):
    """{relative path: bytes} of a stream directory with any number of nodes per element"""
    files = R.write_files(names, levels, ins)
    files["Elements"] = elements_text([int(v) for v in face], nElts, ins)
    for l, fabs in enumerate(levels):
        files["Level_%d/Str_H" % l] = str_header(fabs, len(names))
    return files


def placeholder_bytes(ncomp):
    """the data file of a level that holds the placeholder alone"""
    return b"FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))((0,0,0) (0,0,0) (0,0,0)) %d\n" % ncomp + bytes(8 * ncomp)


def with_placeholders(levels, inside, ncomp):
    """semantics 8: a level that kept no box holds the null box of zeros, which lists no id"""
    levels = [fabs if fabs else [((0, 0, 0), (0, 0, 0), np.zeros((ncomp, 1, 1)))] for fabs in levels]
    return levels, [per if per else [[]] for per in inside]


def run(files, infile="in", outfile=None, comps=(), verbose=0, ngpus=1, plant=None, **keys):
    """main of streamSub.cpp as streamSub3d runs it -> dict(files, outfile, stdout, stderr, sub, E, comp_idx)"""
    if ngpus > 1:
        raise SubAbort("ngpus")
    if outfile is None:
        outfile = default_outfile(infile)
    path = S.read_stream_dir(files)
    names = path["names"]
    comp_idx = select_comps(names, comps)
    if path["npe"] < 1:
        raise SubAbort("Elements: %d nodes per element" % path["npe"])
    how = element_list(path["nElts"], **keys)
    node_map = check_tables(path, how[0] == "seed")
    err = ""
    if verbose:
        err += "Reading components: " + "".join("%d " % c for c in comp_idx) + " from stream file ...\n"
    for lev in range(len(path["levels"])):
        err += "Possibly reading mf level %d\n" % lev
    if how[0] == "seed":
        E = seed_elements(path, node_map, how[1], how[2])
        if not E:
            raise SubAbort("no element has all its seed points inside seedLo .. seedHi")
    else:
        E = how[1]
    sub = subset(path, E, comp_idx, plant)
    if verbose:
        err += "...finished reading stream file \n"
    sel_names = [names[c] for c in comp_idx]
    if plant == "user_order_names" and comps:
        sel_names = list(comps)
    levels, inside = with_placeholders(sub["levels"], sub["inside"], len(comp_idx))
    nSel = len(sub["face"]) // path["npe"]
    out = dir_files(sel_names, levels, inside, sub["face"], nSel)
    if plant == "old_box_ids":
        old = []
        for lev, per in enumerate(sub["inside"]):
            full = [[] for _ in range(max(sub["boxIDs"][lev]) + 1)] if sub["boxIDs"][lev] else []
            for b, ids in zip(sub["boxIDs"][lev], per):
                full[b] = ids
            old.append(full)
        out["Elements"] = elements_text(sub["face"], nSel, old)
    return dict(files=out, outfile=outfile, stdout="", stderr=err, sub=sub, E=E, comp_idx=comp_idx)
