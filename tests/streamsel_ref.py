"""CPU restatement (plain Python loops over numpy arrays) of the reference's Src/streamScatter.cpp and Src/stream2plt.cpp: the keys
of the two mains, build_nodeMap, the peak scanned from the middle of the line, the range test and the printing of streamScatter;
downsampleStreamData, the dense array of the selected lines, the filters, the signed arc length and write_tec_ascii of stream2plt.
Written from the reference sources line by line -- per condition, per line, per point, on Python floats (IEEE doubles, one rounding
per operation, comparisons as written) -- and sharing no code with pa_streamsel.hip or the tool drivers.  Not a test module:
test_streamsel_ref.py (CPU) and test_gpu_streamsel.py (GPU, bit for bit / byte for byte) import it.

Where it does not follow the reference text, on purpose (streamScatter3d / stream2plt3d):
  - amrex::Random() is RECALLED (AMReX is not in the reference tree) as libstdc++'s std::uniform_real_distribution<double>(0, 1) over a
    std::mt19937 seeded with 987654321: two 32-bit outputs a, b -> (double(a) + double(b) * 2^32) / 2^64.  Restated here over the raw
    outputs of numpy.random.RandomState(987654321); test_streamsel_ref.py pins the two against each other.
  - what the reference leaves undefined raises SelAbort: no conditioning component, node ids out of range or listed by no box,
    nLines <= 0, finestLevel other than the file's, distComp with no_filter, condition arrays of different counts, components out of
    range, a selected box that does not span the directory's j range.
"""
from __future__ import annotations

import math

import numpy as np

import streamgrad_ref as G
import streamsample_ref as S

NLINESMAX = 32700
SEED = 987654321


class SelAbort(RuntimeError):
    pass


def write_files(names, levels, ins, face=(1, 1, 1)):
    """{relative path: bytes} of a stream directory, written the way streamgrad_ref writes one: levels[l] = [(lo, hi, a [ncomp][nj][ni])],
    ins[l][b] = 1-based node ids ([] for a box without lines)"""
    face = np.asarray(face, np.int32).ravel()
    per = [[np.asarray(i, np.int32) for i in p] for p in ins]
    files = G.stream_file_bytes(names, face, len(face) // 3, per, [[None] * len(p) for p in levels], 1)
    for l, fabs in enumerate(levels):
        hb, db = G.vismf_bytes([(lo, hi, a) for lo, hi, a in fabs])
        files["Level_%d/Str_H" % l] = hb
        files["Level_%d/Str_D_00000" % l] = db
    return files


def trunc_mid(lo, hi):
    """int ptOnStr = 0.5 * (lo + hi): the conversion of a double to int truncates toward zero"""
    return int(math.trunc(0.5 * (lo + hi)))


def fmt(v):
    """operator<<(double) with the default precision"""
    return "%g" % v


# ------------------------------------------------------------------------------------------------ streamScatter.cpp
def build_node_map(path):
    """:212-237 -> [(lev, box, pt)] by node id - 1"""
    num = sum(len(ids) for per in path["ins"] for ids in per)
    node_map = [None] * num
    for l, per in enumerate(path["ins"]):
        for b, ids in enumerate(per):
            lo, hi, _ = path["levels"][l][b]
            if len(ids) > hi[0] - lo[0] + 1:
                raise SelAbort("more inside_nodes than lines")
            for k, v in enumerate(ids):
                v = int(v)
                if v < 1 or v > num:
                    raise SelAbort("inside_nodes id %d outside 1 .. %d" % (v, num))
                node_map[v - 1] = (l, b, k)
    for n, m in enumerate(node_map):
        if m is None:
            raise SelAbort("node %d has no inside_nodes entry" % (n + 1))
    return node_map


def peaks(path, condComp):
    """:119-143 for every node -> (ptOnStr list, hiVal list)"""
    jp, hv = [], []
    for (L, B, Pt) in build_node_map(path):
        lo, hi, fab = path["levels"][L][B]
        loPt, hiPt = lo[1], hi[1]
        ptOnStr = trunc_mid(loPt, hiPt)
        hiVal = float(fab[condComp, ptOnStr - loPt, Pt])
        for j in range(loPt, hiPt + 1):
            val = float(fab[condComp, j - loPt, Pt])
            if val > hiVal:
                hiVal = val
                ptOnStr = j
        jp.append(ptOnStr)
        hv.append(hiVal)
    return jp, hv


def scatter_rows(path, comps, condComp, moreThan, lessThan):
    """:119-155 -> the rows of the kept nodes, in node order"""
    jp, hv = peaks(path, condComp)
    rows = []
    for (L, B, Pt), j, hiVal in zip(build_node_map(path), jp, hv):
        lo, hi, fab = path["levels"][L][B]
        if (hiVal >= moreThan) and (hiVal < lessThan):
            rows.append([float(fab[c, j - lo[1], Pt]) for c in comps])
    return rows


def run_scatter(files, vars=(), condVar="", condComp=-1, condValMoreThan=0.0, condValLessThan=0.0, ngpus=1):
    """main of streamScatter.cpp -> stdout text"""
    if ngpus > 1:
        raise SelAbort("ngpus")
    path = S.read_stream_dir(files)
    names = path["names"]
    if len(vars) == 0:
        raise SelAbort("ParmParse::getarr(): vars not found in table")  # :88
    comps = []
    for v in vars:
        if v not in names:
            raise SelAbort("Variable not found: " + v)
        comps.append(names.index(v))  # the first with the name (:90-94)
    if condVar != "":
        for j, n in enumerate(names):
            if n == condVar:
                condComp = j  # the last with the name (:106-110)
        if condComp < 0:
            raise SelAbort("Conditioning variable not found: " + condVar)
    if condComp < 0:
        raise SelAbort("no conditioning component")
    if condComp >= len(names):
        raise SelAbort("condComp out of range")
    rows = scatter_rows(path, comps, condComp, float(condValMoreThan), float(condValLessThan))
    return "".join("".join(fmt(v) + " " for v in r) + "\n" for r in rows)


# ------------------------------------------------------------------------------------------------ stream2plt.cpp
def random_draws(n):
    """the first n values of amrex::Random() as recalled (module docstring)"""
    raw = np.random.RandomState(SEED).randint(0, 2 ** 32, size=2 * n, dtype=np.uint32)
    out = []
    for k in range(n):
        a, b = float(raw[2 * k]), float(raw[2 * k + 1])
        r = (a + b * 4294967296.0) / 18446744073709551616.0
        out.append(r if r < 1.0 else math.nextafter(1.0, 0.0))
    return out


def do_test(thisVal, sgn, critVal):
    """:732-751"""
    if sgn == "ge":
        return thisVal >= critVal
    if sgn == "gt":
        return thisVal > critVal
    if sgn == "lt":
        return thisVal < critVal
    if sgn == "le":
        return thisVal <= critVal
    if sgn == "eq":
        return thisVal == critVal
    if sgn == "ne":
        return thisVal != critVal
    return False


def std_max(a, b):
    return b if a < b else a


def std_min(a, b):
    return b if b < a else a


def stream_extent(path):
    """StreamData.cpp:207-217, :263-284 -> (slo, shi, NLines)"""
    ext = None
    for fabs in path["levels"]:
        for lo, hi, _ in fabs:
            if ext is None and not (tuple(lo) == (0, 0, 0) and tuple(hi) == (0, 0, 0)):
                ext = (lo[1], hi[1])
    NLines = sum(len(ids) for per in path["ins"] for ids in per)
    if ext is None or NLines < 1:
        raise SelAbort("no lines")
    return ext[0], ext[1], NLines


def downsample(path, num_lines, NLines, verbose=False):
    """:31-126 -> (sel = [(lev, box, line)] in the order of their new index, boxes kept per level, the verbose text)"""
    rval = float(num_lines) / float(NLines)
    rnd = iter(random_draws(NLines))
    sel, nbox, text = [], [], []
    for lev, per in enumerate(path["ins"]):
        grids = []
        for box_id, ids in enumerate(per):
            pairs = []
            for i in range(len(ids)):
                doit = next(rnd)
                if doit < rval:
                    pairs.append((len(sel), i))
                    sel.append((lev, box_id, i))
            if pairs:
                grids.append((box_id, pairs))
        nbox.append(len(grids))
        if verbose:
            for k, (box_id, pairs) in enumerate(grids):
                lo, hi, _ = path["levels"][lev][box_id]
                text.append("%d (%d): " % (k, len(pairs)) + "".join(" ( %d from %d ) " % p for p in pairs) + " src data has %d particles\n" % (hi[0] - lo[0] + 1))
    return sel, nbox, "".join(text)


def final_array(path, sel, comps, slo, shi, extra=0):
    """:498-547 -> fab [len(comps) + extra][shi - slo + 1][nLines]; the extra components are zero"""
    fab = np.zeros((len(comps) + extra, shi - slo + 1, len(sel)))
    for new, (lev, box, line) in enumerate(sel):
        lo, hi, a = path["levels"][lev][box]
        if lo[1] != slo or hi[1] != shi:
            raise SelAbort("Str box (j = %d .. %d) does not span the directory's j = %d .. %d" % (lo[1], hi[1], slo, shi))
        for n, c in enumerate(comps):
            for j in range(shi - slo + 1):
                fab[n, j, new] = a[c, j, line]
    return fab


def first_crossing(fab, i, nvals, loc_comp, loc_val):
    """:634-641 / :681-688 -> (j, alpha) of the first strictly bracketing segment, or None"""
    for j in range(nvals - 1):
        loc_val_lo, loc_val_hi = float(fab[loc_comp, j, i]), float(fab[loc_comp, j + 1, i])
        if ((loc_val_lo > loc_val) and (loc_val_hi < loc_val)) or ((loc_val_lo < loc_val) and (loc_val_hi > loc_val)):
            return j, (loc_val - loc_val_lo) / (loc_val_hi - loc_val_lo)
    return None


def filter_lines(fab, slo, shi, maxc=(), minc=(), RXY=-1.0, RXYsgn="", atc=()):
    """:556-651.  maxc / minc: (comp, sgn, val); atc: (atComp, compAt as read -- a real --, atSgn, valAt, atVal) -> write_lines"""
    nLines, nvals = fab.shape[2], shi - slo + 1
    write_lines = [1] * nLines
    for nc, sgn, crit in maxc:
        for i in range(nLines):
            maxVal = float(fab[nc, 0, 0])  # fab(se, nc): line 0
            for j in range(nvals):
                maxVal = std_max(float(fab[nc, j, i]), maxVal)
            if not do_test(maxVal, sgn, crit):
                write_lines[i] = 0
    for nc, sgn, crit in minc:
        for i in range(nLines):
            minVal = float(fab[nc, 0, 0])
            for j in range(nvals):
                minVal = std_min(float(fab[nc, j, i]), minVal)
            if not do_test(minVal, sgn, crit):
                write_lines[i] = 0
    if RXY > 0:
        jm = trunc_mid(slo, shi) - slo
        for i in range(nLines):
            radius = 0.0
            for n in range(2):
                val = float(fab[n, jm, i])
                radius += val * val
            radius = math.sqrt(radius)
            if not do_test(radius, RXYsgn, RXY):
                write_lines[i] = 0
    for loc_comp, compAt, sgn, test_val, loc_val in atc:
        test_comp = int(math.trunc(compAt))
        for i in range(nLines):
            hit = first_crossing(fab, i, nvals, loc_comp, loc_val)
            if hit is not None:
                j, alpha = hit
                val_lo, val_hi = float(fab[test_comp, j, i]), float(fab[test_comp, j + 1, i])
                val_test = val_lo + alpha * (val_hi - val_lo)
                write_lines[i] = 1 if do_test(val_test, sgn, test_val) else 0
    return write_lines


def segment_lengths(fab, i):
    """:671-676 for every segment of line i"""
    out = []
    for j in range(1, fab.shape[1]):
        ds = 0.0
        for n in range(3):
            dx = float(fab[n, j, i]) - float(fab[n, j - 1, i])
            ds += dx * dx
        out.append(math.sqrt(ds))
    return out


def arc_length(fab, nDist, distComp, distVal):
    """:654-713, in place on component nDist"""
    nLines, nvals = fab.shape[2], fab.shape[1]
    for i in range(nLines):
        fab[nDist, 0, i] = 0.0
        for j, ds in enumerate(segment_lengths(fab, i), start=1):
            fab[nDist, j, i] = float(fab[nDist, j - 1, i]) + ds
        hit = first_crossing(fab, i, nvals, distComp, distVal)
        if hit is not None:
            j, alpha = hit
            val_lo, val_hi = float(fab[nDist, j, i]), float(fab[nDist, j + 1, i])
            loc_offset = val_lo + alpha * (val_hi - val_lo)
            for jj in range(nvals):
                fab[nDist, jj, i] = float(fab[nDist, jj, i]) - loc_offset
        else:
            err_val = float(fab[nDist, nvals - 1, i]) * 2
            for j in range(nvals):
                fab[nDist, j, i] = err_val


def tec_bytes(fab, names, write_lines):
    """write_tec_ascii (:269-318)"""
    s = ["VARIABLES = " + "".join(n + " " for n in names) + "\n"]
    for i in range(fab.shape[2]):
        if write_lines[i] > 0:
            s.append("ZONE T=id%d I=%d F=POINT\n" % (i, fab.shape[1]))
            for j in range(fab.shape[1]):
                s.append("".join(fmt(fab[n, j, i]) + " " for n in range(fab.shape[0])) + "\n")
    return "".join(s).encode()


def _same_count(first, n, **arrs):
    for k, v in arrs.items():
        if len(v) != n:
            raise SelAbort("%s has %d values, %s has %d" % (k, len(v), first, n))


def run_stream2plt(files, nLines=0, comps=None, sComp=0, nComp=None, no_filter=0, maxComps=(), maxVals=(), maxSgns=(), minComps=(), minVals=(), minSgns=(),
                   atComps=(), compAt=(), valAt=(), atVal=(), atSgns=(), RXY=-1.0, RXYsgn="", distComp=-1, distVal=None, finestLevel=None, verbose=0, ngpus=1):
    """main of stream2plt.cpp -> dict(stdout, dat, write_lines, fab, sel)"""
    if ngpus > 1:
        raise SelAbort("ngpus")
    path = S.read_stream_dir(files)
    names = path["names"]
    nlev = len(path["levels"])
    if finestLevel is not None and finestLevel != nlev - 1:
        raise SelAbort("finestLevel")
    slo, shi, NLines = stream_extent(path)
    if comps is None:
        comps = [sComp + i for i in range(len(names) if nComp is None else nComp)]
    comps = list(comps)
    if not comps or any(c < 0 or c >= len(names) for c in comps):
        raise SelAbort("component out of range")
    sel_names = [names[c] for c in comps]

    def sel_ok(c):
        if c < 0 or c >= len(comps):
            raise SelAbort("component %d out of range (%d components are selected)" % (c, len(comps)))
    if distComp >= 0:
        if distVal is None:
            raise SelAbort("distVal not found")
        sel_ok(distComp)
        if len(comps) < 3:
            raise SelAbort("distComp needs three coordinates")
        sel_names.append("distance_from_" + names[comps[distComp]] + "_eq_" + fmt(distVal))
    if distComp >= 0 and no_filter:
        raise SelAbort("distComp with no_filter")
    nLines = min(int(nLines), NLINESMAX)
    if nLines <= 0:
        raise SelAbort("nLines")
    if RXY > 0 and len(comps) < 2:
        raise SelAbort("RXY needs two components")
    _same_count("maxComps", len(maxComps), maxVals=maxVals, maxSgns=maxSgns)
    _same_count("minComps", len(minComps), minVals=minVals, minSgns=minSgns)
    _same_count("atComps", len(atComps), compAt=compAt, valAt=valAt, atVal=atVal, atSgns=atSgns)
    for c in list(maxComps) + list(minComps) + list(atComps) + [int(math.trunc(c)) for c in compAt]:
        sel_ok(c)
    out = []
    condStr = ""
    if verbose:
        out.append("Preparing to extract/write the following components (i,idx,name): \n")
        out.append("".join("(%d,%d,%s) " % (i, c, names[c]) for i, c in enumerate(comps)) + "\n")
        if len(sel_names) > len(comps):
            out.append("....appending the following component(s): " + "".join(n + "\n" for n in sel_names[len(comps):]))
        for c, s, v in zip(maxComps, maxSgns, maxVals):
            condStr += "Max(" + names[comps[c]] + ") " + s + " " + fmt(v) + "; "
        for c, s, v in zip(minComps, minSgns, minVals):
            condStr += "Min(" + names[comps[c]] + ") " + s + " " + fmt(v) + "; "
        for ac, ca, s, va, av in zip(atComps, compAt, atSgns, valAt, atVal):
            condStr += names[comps[int(math.trunc(ca))]] + "(" + names[comps[ac]] + " = " + fmt(av) + ") " + s + " " + fmt(va) + "; "
        if RXY > 0:
            condStr += "radiusXY " + RXYsgn + " " + fmt(RXY) + " "
        if condStr != "":
            out.append(" ...subject to: " + condStr + "\n")
    sel, nbox, vtext = downsample(path, nLines, NLines, verbose)
    out.append(vtext)
    out.append("Reduced dataset has %d lines \n" % len(sel))
    if not sel:
        raise SelAbort("no line was selected")
    if verbose:
        for l in range(nlev):
            out.append("Reduced  dataset has %d boxes (original has %d) at level = %d\n" % (nbox[l], len(path["levels"][l]), l))
    fab = final_array(path, sel, comps, slo, shi, extra=len(sel_names) - len(comps))
    write_lines = [1] * len(sel)
    if not no_filter:
        write_lines = filter_lines(fab, slo, shi, list(zip(maxComps, maxSgns, maxVals)), list(zip(minComps, minSgns, minVals)), RXY, RXYsgn,
                                   list(zip(atComps, compAt, atSgns, valAt, atVal)))
        if distComp >= 0:
            arc_length(fab, len(comps), distComp, float(distVal))
    return dict(stdout="".join(out), dat=tec_bytes(fab, sel_names, write_lines), write_lines=write_lines, fab=fab, sel=sel, slo=slo, shi=shi)
