"""Plain-Python restatement of the reference's sliceMEF.cpp and trimMEFgen.cpp, line by line: what peleanalysis_amd/csrc/pa_surfcut.hip,
tools/common/pa_contour.h and the two tools are held to.  Python floats only (IEEE double, one operation at a time, no fused
multiply-add); the vertex cache is a dict with the reference's forward-then-reverse lookup; the numbering sorts the directed keys (the
reference's std::map<std::pair<int,int>, ...> orders by std::pair's <); the lines are assembled by a list scan.  The one value that is
not the reference's: the area TOTAL is the exactly rounded sum the 192-bit fixed-point accumulator returns (tests/fixed192_ref.py);
the reference adds serially.

`mistake=` plants one wrong reading of the reference, for tests/test_surfcut_ref.py: every one of them must change a named case."""
import math

import numpy as np

import fixed192_ref as FX

EPS = 1.0e-8  # epsilon_DEF
FAB_DESC = "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))"
SIGNS = ("lt", "le", "gt", "ge", "eq")
MISTAKES = ("minmax_numbering", "lower_id_direction", "le_classify", "eps_order", "walk_last", "elt_any", "keep_unused")


# ---------------------------------------------------------------------------------------------------- slice
def vi_doit(val, comp, pts, p1, p2, mistake=None):
    """VI_doIt, sliceMEF.cpp:581-605"""
    pt1, pt2 = pts[p1], pts[p2]
    v1, v2 = pt1[comp], pt2[comp]
    if mistake == "eps_order":
        if abs(val - v2) < EPS:
            return list(pt2)
        if abs(val - v1) < EPS:
            return list(pt1)
    else:
        if abs(val - v1) < EPS:
            return list(pt1)
        if abs(val - v2) < EPS:
            return list(pt2)
    if abs(v1 - v2) < EPS:
        return list(pt1)
    mu = (val - v1) / (v2 - v1)
    return [a + mu * (b - a) for a, b in zip(pt1, pt2)]


def slice_surface(nodes, elts1, comp, val, mistake=None):
    """sliceMEF.cpp:239-268 with Segmentise :637-681 and VertexInterp :607-630.  -> dict(verts [nv][nc], pairs [nv][2], segs [ns][2],
    src [ns], csr_off [nv + 1], csr_adj [2 ns]); ids 0-based"""
    pts = np.asarray(nodes, dtype=np.float64).tolist()
    nc = np.asarray(nodes).shape[1]
    val = float(val)
    cache = {}  # directed pair of the first request -> point
    raw, src = [], []

    def below(p):
        return pts[p][comp] <= val if mistake == "le_classify" else pts[p][comp] < val

    def vertex(p1, p2):
        if mistake == "lower_id_direction":
            p1, p2 = min(p1, p2), max(p1, p2)
        if (p1, p2) in cache:
            return (p1, p2)
        if (p2, p1) in cache:
            return (p2, p1)
        cache[(p1, p2)] = vi_doit(val, comp, pts, p1, p2, mistake)
        return (p1, p2)

    for i, e in enumerate(np.asarray(elts1).reshape(-1, 3).tolist()):
        p0, p1, p2 = e[0] - 1, e[1] - 1, e[2] - 1
        case = (1 if below(p0) else 0) | (2 if below(p1) else 0) | (4 if below(p2) else 0)
        if case in (0, 7):
            continue
        if case in (1, 6):
            a, b = vertex(p0, p1), vertex(p0, p2)
        elif case in (2, 5):
            a, b = vertex(p1, p0), vertex(p1, p2)
        else:
            a, b = vertex(p2, p0), vertex(p2, p1)
        raw.append((a, b))
        src.append(i)
    keys = sorted(cache, key=(lambda k: (min(k), max(k))) if mistake == "minmax_numbering" else None)
    vid = {k: j for j, k in enumerate(keys)}
    segs = [(vid[a], vid[b]) for a, b in raw]
    rows = [[] for _ in keys]
    for s, (l, r) in enumerate(segs):  # the requests in order: first end, second end
        rows[l].append(s)
        rows[r].append(s)
    off = np.zeros(len(keys) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(r) for r in rows], dtype=np.int64)
    return dict(verts=np.array([cache[k] for k in keys], dtype=np.float64).reshape(len(keys), nc),
                pairs=np.array(keys, dtype=np.int32).reshape(len(keys), 2), segs=np.array(segs, dtype=np.int32).reshape(len(segs), 2),
                src=np.array(src, dtype=np.int32), csr_off=off, csr_adj=np.array([s for r in rows for s in r], dtype=np.int32))


def join_fragments(lines):
    """sliceMEF.cpp:311-360: lines = list of lists of (l, r)"""
    changed = True
    while changed:
        changed = False
        for it in lines:
            if not it:
                continue
            idx_l, idx_r = it[0][0], it[-1][1]  # read once per outer fragment: stale after a splice
            for jt in lines:
                if not jt or it[0] == jt[0]:
                    continue
                if idx_r == jt[0][0]:
                    it.extend(jt)
                    del jt[:]
                    changed = True
                elif idx_r == jt[-1][1]:
                    it.extend((r, l) for l, r in reversed(jt))
                    del jt[:]
                    changed = True
                elif idx_l == jt[0][0]:
                    it[0:0] = [(r, l) for l, r in reversed(jt)]
                    del jt[:]
                    changed = True
    return [ln for ln in lines if ln]


def contour_lines(segs, mistake=None):
    """sliceMEF.cpp:270-360 by a scan of the list of remaining segments (FindMySeg :537-546).  -> list of lists of (l, r)"""
    rest = [tuple(int(x) for x in s) for s in np.asarray(segs).reshape(-1, 2).tolist()]
    lines = []
    if rest:
        idx = rest[0][0]
        lines.append([])
        while rest:
            order = range(len(rest) - 1, -1, -1) if mistake == "walk_last" else range(len(rest))
            hit = next((i for i in order if rest[i][0] == idx or rest[i][1] == idx), None)
            if hit is not None:
                s = rest.pop(hit)
                if s[0] == idx:
                    lines[-1].append(s)
                    idx = s[1]
                else:
                    lines[-1].append((s[1], s[0]))
                    idx = s[0]
            else:
                lines.append([])
                idx = rest[0][0]
    return join_fragments(lines)


def is_closed(line):
    return line[0][0] == line[-1][1]


def root_name(infile):
    """rootName, sliceMEF.cpp:98-111 (Tokenize drops empty tokens)"""
    res = [t for t in infile.split("/") if t]
    res = [t for t in res[-1].split(".") if t]
    return ".".join(res[:-1]) if len(res) > 1 else res[0]


def out_root(infile, name, loc):
    """sliceMEF.cpp:362-367"""
    return "%s_%s_%s%s" % (root_name(infile), name, "n" if loc < 0 else ("p" if loc > 0 else ""), "%g" % abs(loc))


def dat_text(infile, names, d, loc, verts, lines):
    """sliceMEF.cpp:376-409; the default stream format of a double is %g"""
    out = ["VARIABLES = " + "".join('"%s" ' % n for n in names) + "\n"]
    pts = np.asarray(verts).tolist()
    for k, ln in enumerate(lines):
        out.append('ZONE T="%s_%s_%s_%d", I=%d\n' % (root_name(infile), names[d], "%g" % loc, k, len(ln) + 1))
        for v in [ln[0][0]] + [s[1] for s in ln]:
            out.append("".join("%g " % x for x in pts[v]) + "\n")
    return "".join(out)


def mef_bytes(nodes, elts1, title, names, nodes_per_elt=3):
    """write_iso (sliceMEF.cpp:449-491, trimMEFgen.cpp:533-575)"""
    nodes = np.ascontiguousarray(nodes, dtype="<f8").reshape(-1, len(names))
    elts1 = np.ascontiguousarray(elts1, dtype="<i4").reshape(-1, nodes_per_elt)
    head = "%s\n%s\n%d %d\n" % (title, " ".join(names), len(elts1), nodes_per_elt)
    head += FAB_DESC + "((0,0,0) (%d,0,0) (0,0,0)) %d\n" % (len(nodes) - 1, nodes.shape[1])
    return head.encode() + nodes.tobytes() + elts1.tobytes()


def run_slice_tool(infile, nodes, elts1, title, names, d=0, locs=(0.0,), write_tec=True, write_mef=True):
    """what sliceMEF3d.ex leaves behind: -> ({file name: text or bytes}, stderr lines)"""
    files, err = {}, []
    for loc in locs:
        loc = float(loc)
        s = slice_surface(nodes, elts1, d, loc)
        err.append("%s=%s slice computed." % (names[d], "%g" % loc))
        lines = contour_lines(s["segs"])
        root = out_root(infile, names[d], loc)
        if write_tec:
            err.append("Writing contour (%d nodes, %d segments, %d lines) to %s.dat" % (len(s["verts"]), len(s["segs"]), len(lines), root))
            files[root + ".dat"] = dat_text(infile, names, d, loc, s["verts"], lines)
        if write_mef:
            if len(s["segs"]) == 0:  # deviation: the reference divides by nElts == 0
                err.append("sliceMEF3d: %s=%s cuts nothing: %s.mef is not written" % (names[d], "%g" % loc, root))
            else:
                files[root + ".mef"] = mef_bytes(s["verts"], s["segs"] + 1, title, names, 2)
    return files, err


# ---------------------------------------------------------------------------------------------------- trim
def _holds(d, sign, v):
    if sign == "lt":
        return d < v
    if sign == "le":
        return d <= v
    if sign == "gt":
        return d > v
    if sign == "ge":
        return d >= v
    if sign == "eq":
        return d == v
    raise ValueError("Bad signs data. Use one of [lt,le,gt,ge,eq]")


def _compact(pts, elts, remove):
    """the second half of trim_surface / trim_surface_RXY (trimMEFgen.cpp:139-191): nodes and elements keep their order"""
    idx, n = [], 0
    for r in remove:
        idx.append(-1 if r else n)
        n += 0 if r else 1
    new_pts = [p for p, r in zip(pts, remove) if not r]
    new_elts = []
    for e in elts:
        if all(idx[q - 1] >= 0 for q in e):
            new_elts.append([idx[q - 1] + 1 for q in e])
    return new_pts, new_elts


def trim_surface(nodes, elts1, conds=(), rxy=-1.0, sign_rxy="lt", mistake=None):
    """trim_surface (trimMEFgen.cpp:90-192), then trim_surface_RXY (:195-294), then remove_unused_nodes (:297-372), as main calls them
    (:433-458, :524).  -> (nodes [N'][nc], elts [M'][3] int32 1-based, nodes removed as unused)"""
    nc = np.asarray(nodes).shape[1]
    pts = np.asarray(nodes, dtype=np.float64).tolist()
    elts = np.asarray(elts1).reshape(-1, 3).tolist()
    if mistake == "elt_any":  # an element is kept if ANY node survives: its removed nodes have to stay
        rem = [any(_holds(p[c], s, float(v)) for c, s, v in conds) for p in pts]
        if rxy >= 0:
            rem = [r or _holds(math.sqrt(p[0] * p[0] + p[1] * p[1]), sign_rxy, float(rxy)) for r, p in zip(rem, pts)]
        keep_e = [e for e in elts if not all(rem[q - 1] for q in e)]
        used = set(q - 1 for e in keep_e for q in e)
        pts, elts = _compact(pts, keep_e, [i not in used for i in range(len(pts))])
        return np.array(pts, dtype=np.float64).reshape(len(pts), nc), np.array(elts, dtype=np.int32).reshape(len(elts), 3), 0
    if len(conds) > 0:
        remove = []
        for p in pts:
            r = False
            for c, s, v in conds:
                r = r or _holds(p[c], s, float(v))
            remove.append(r)
        pts, elts = _compact(pts, elts, remove)
    if rxy >= 0:
        remove = [_holds(math.sqrt(p[0] * p[0] + p[1] * p[1]), sign_rxy, float(rxy)) for p in pts]
        pts, elts = _compact(pts, elts, remove)
    unused = [True] * len(pts)
    for e in elts:
        for q in e:
            unused[q - 1] = False
    n_unused = sum(unused)
    if mistake != "keep_unused":
        pts, elts = _compact(pts, elts, unused)
    return np.array(pts, dtype=np.float64).reshape(len(pts), nc), np.array(elts, dtype=np.int32).reshape(len(elts), 3), n_unused


def triangle_areas(nodes, elts1):
    """the written expression of surface_area (trimMEFgen.cpp:76-84); pow(x, 2) is x * x exactly"""
    pts = np.asarray(nodes, dtype=np.float64).tolist()
    out = []
    for a, b, c in np.asarray(elts1).reshape(-1, 3).tolist():
        p0, p1, p2 = pts[a - 1], pts[b - 1], pts[c - 1]
        t0 = (p1[1] - p0[1]) * (p2[2] - p0[2]) - (p1[2] - p0[2]) * (p2[1] - p0[1])
        t1 = (p1[2] - p0[2]) * (p2[0] - p0[0]) - (p1[0] - p0[0]) * (p2[2] - p0[2])
        t2 = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0])
        out.append(0.5 * math.sqrt(t0 * t0 + t1 * t1 + t2 * t2))
    return out


def area(nodes, elts1):
    """-> (total, min, max): the total is the exactly rounded fixed-point sum, scaled from the largest area; all 0 without elements"""
    a = triangle_areas(nodes, elts1)
    if not a:
        return 0.0, 0.0, 0.0
    s = FX.scale_of(max(a))
    tot, flag = FX.sum_terms(a, s)
    assert flag == 0
    return FX.read(tot, s), min(a), max(a)


def run_trim_tool(nodes, elts1, title, names, conds=(), rxy=-1.0, sign_rxy="lt", rem_comps=(), do_area_stats=False):
    """what trimMEFgen3d.ex does: -> (mef bytes, stdout lines)"""
    out = ["Surface area before: %g" % area(nodes, elts1)[0]]
    n2, e2, unused = trim_surface(nodes, elts1, conds, rxy, sign_rxy)
    tot, lo, hi = area(n2, e2)
    out.append("Surface area after: %g" % tot)
    if do_area_stats:
        out.append("  Triangle area min, max: %g , %g" % (lo, hi))
    if unused > 0:
        out.append("Removed %d unusued nodes" % unused)
    keep = [c for c in range(len(names)) if c not in rem_comps]
    return mef_bytes(n2[:, keep], e2, title, [names[c] for c in keep]), out
