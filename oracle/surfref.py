"""ctypes bindings of the REFERENCE's own surface-tool arithmetic, compiled by `make -C oracle ref` into oracle/_ref/ (recipe: Makefile;
wrappers: ref/*_ref_wrap.cpp; shim: ref/surf_shim.h): binMEF.cpp, sliceMEF.cpp, trimMEFgen.cpp, mergeMEF.cpp, streamTubeStats.cpp.
Test infrastructure only.  Every function returns None where the library does not exist (no reference tree, nothing prebuilt)."""
import ctypes as C

import numpy as np

from . import oracle as O

SIGNS = ("lt", "le", "gt", "ge", "eq")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f8(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i4(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def lib(tool):
    """tool in binmef, slicemef, trimmef, mergemef"""
    src = {"binmef": "Src/binMEF.cpp", "slicemef": "Src/sliceMEF.cpp", "trimmef": "Src/trimMEFgen.cpp", "mergemef": "Src/mergeMEF.cpp"}[tool]
    return O._ref_lib("lib%s_ref.so" % tool, src)


class RefAssertion(ArithmeticError):
    """the reference's AMREX_ALWAYS_ASSERT on the split fractions fired (binMEF.cpp:121, :159)"""


def binmef(nodes, elts, bin_comps, bin_min, bin_max, nbins, cond=None, area_eps=1.0e-20):
    """binMEF.cpp's element loop.  cond = (condComp, condVal, condSgn) or None.  -> dict(bins [L][nc] int32 and areas [L] of the leaves
    in visiting order, n_my, outside (areaOutsideCondition), total (the serial sum of the element areas)), or None"""
    R = lib("binmef")
    if R is None:
        return None
    nodes, elts = _f8(nodes), _i4(elts).reshape(-1, 3)
    nc = len(bin_comps)
    bc, mn, mx, nb = _i4(bin_comps), _f8(bin_min), _f8(bin_max), _i4(nbins)
    counts, sums = np.zeros(2, dtype=np.int64), np.zeros(2)
    R.ref_binmef_run.restype = C.c_int
    rc = R.ref_binmef_run(C.c_int64(len(nodes)), C.c_int(nodes.shape[1]), _p(nodes), C.c_int64(len(elts)), _p(elts), C.c_int(nc), _p(bc), _p(mn), _p(mx), _p(nb),
                          C.c_double(area_eps), C.c_int(1 if cond else 0), C.c_int(cond[0] if cond else 0), C.c_double(cond[1] if cond else 0.0),
                          C.c_int(cond[2] if cond else 0), _p(counts), _p(sums))
    if rc == 1:
        raise RefAssertion("split fraction outside [0, 1]")
    assert rc == 0
    L = int(counts[0])
    bins, areas = np.zeros((L, nc), dtype=np.int32), np.zeros(L)
    R.ref_binmef_leaves(C.c_int(nc), _p(bins), _p(areas))
    return dict(bins=bins, areas=areas, n_my=int(counts[1]), outside=float(sums[0]), total=float(sums[1]))


def binmef_triangle_area(p0, p1, p2):
    R = lib("binmef")
    if R is None:
        return None
    R.ref_binmef_triangle_area.restype = C.c_double
    a, b, c = _f8(p0)[:3].copy(), _f8(p1)[:3].copy(), _f8(p2)[:3].copy()
    return float(R.ref_binmef_triangle_area(_p(a), _p(b), _p(c)))


def slicemef(nodes, elts, comp, loc):
    """sliceMEF.cpp at one location.  -> dict(verts [nv][nc], pairs [nv][2], segs [ns][2], lines = list of [n][2] int32), or None"""
    R = lib("slicemef")
    if R is None:
        return None
    nodes, elts = _f8(nodes), _i4(elts).reshape(-1, 3)
    counts = np.zeros(4, dtype=np.int64)
    R.ref_slicemef_run.restype = C.c_int
    rc = R.ref_slicemef_run(C.c_int64(len(nodes)), C.c_int(nodes.shape[1]), _p(nodes), C.c_int64(len(elts)), _p(elts), C.c_int(int(comp)), C.c_double(float(loc)),
                            _p(counts))
    assert rc == 0
    nv, ns, nl, nls = (int(v) for v in counts)
    verts, pairs, segs = np.zeros((nv, nodes.shape[1])), np.zeros((nv, 2), dtype=np.int32), np.zeros((ns, 2), dtype=np.int32)
    lines, off = np.zeros((nls, 2), dtype=np.int32), np.zeros(nl + 1, dtype=np.int32)
    R.ref_slicemef_get(_p(verts), _p(pairs), _p(segs), _p(lines), _p(off))
    return dict(verts=verts, pairs=pairs, segs=segs, lines=[lines[off[q]:off[q + 1]] for q in range(nl)])


def slicemef_vi(val, comp, p1, p2):
    """VI_doIt"""
    R = lib("slicemef")
    if R is None:
        return None
    p1, p2 = _f8(p1), _f8(p2)
    out = np.zeros(len(p1))
    R.ref_slicemef_vi(C.c_double(float(val)), C.c_int(int(comp)), C.c_int(len(p1)), _p(p1), _p(p2), _p(out))
    return out


def trimmef(nodes, elts, conds=(), rxy=-1.0, sign_rxy="lt"):
    """trim_surface, trim_surface_RXY, remove_unused_nodes as main calls them.  -> (nodes, elts [M'][3] int32 1-based, unused), or None"""
    R = lib("trimmef")
    if R is None:
        return None
    nodes, elts = _f8(nodes), _i4(elts).reshape(-1, 3)
    comps, signs, vals = _i4([c for c, _, _ in conds]), _i4([SIGNS.index(s) for _, s, _ in conds]), _f8([v for _, _, v in conds])
    counts = np.zeros(3, dtype=np.int64)
    R.ref_trimmef_run.restype = C.c_int
    rc = R.ref_trimmef_run(C.c_int64(len(nodes)), C.c_int(nodes.shape[1]), _p(nodes), C.c_int64(len(elts)), _p(elts), C.c_int(len(conds)), _p(comps), _p(signs),
                           _p(vals), C.c_double(float(rxy)), C.c_int(SIGNS.index(sign_rxy)), _p(counts))
    assert rc == 0
    out, oe = np.zeros((int(counts[0]), nodes.shape[1])), np.zeros((int(counts[1]), 3), dtype=np.int32)
    R.ref_trimmef_get(_p(out), _p(oe))
    return out, oe, int(counts[2])


def trimmef_areas(nodes, elts):
    """-> (surface_area's term of every element, triangle_area of every element, surface_area of the surface), or None"""
    R = lib("trimmef")
    if R is None:
        return None
    nodes, elts = _f8(nodes), _i4(elts).reshape(-1, 3)
    per, tri = np.zeros(len(elts)), np.zeros(len(elts))
    R.ref_trimmef_areas.restype = C.c_double
    tot = R.ref_trimmef_areas(C.c_int64(len(nodes)), C.c_int(nodes.shape[1]), _p(nodes), C.c_int64(len(elts)), _p(elts), _p(per), _p(tri))
    return per, tri, float(tot)


NO_ELEMENTS = "the reference divides by zero"  # mergemef: M or S without elements (mergeMEF.cpp:150, :154)


def mergemef(nodes_m, elts_m, nodes_s, elts_s, eps=1.0e-8, rem_dup_nodes=False):
    """merge_iso.  -> (nodes, elts) of M afterwards, NO_ELEMENTS, or None"""
    R = lib("mergemef")
    if R is None:
        return None
    nm, ns, em, es = _f8(nodes_m), _f8(nodes_s), _i4(elts_m).reshape(-1, 3), _i4(elts_s).reshape(-1, 3)
    counts = np.zeros(2, dtype=np.int64)
    R.ref_mergemef_run.restype = C.c_int
    rc = R.ref_mergemef_run(C.c_int64(len(nm)), C.c_int(nm.shape[1]), _p(nm), C.c_int64(len(em)), _p(em), C.c_int64(len(ns)), _p(ns), C.c_int64(len(es)), _p(es),
                            C.c_double(float(eps)), C.c_int(1 if rem_dup_nodes else 0), _p(counts))
    if rc == 2:
        return NO_ELEMENTS
    assert rc == 0
    out, oe = np.zeros((int(counts[0]), nm.shape[1])), np.zeros((int(counts[1]), 3), dtype=np.int32)
    R.ref_mergemef_get(_p(out), _p(oe))
    return out, oe


class Tube:
    """streamTubeStats.cpp's arithmetic on one set of Str boxes: boxes = [(jlo, a [ncomp][nj][ni], ids)] with ids the 1-based node numbers
    of the box's lines in order (X Y Z are components 0 1 2).  One instance at a time: the library keeps the data of the last one.
    None from Tube.make where the library does not exist."""

    @classmethod
    def make(cls, boxes):
        return cls(boxes) if lib_tube() is not None else None

    def __init__(self, boxes):
        self.R = lib_tube()
        desc = np.array([(a.shape[2], a.shape[1], jlo) for jlo, a, _ in boxes], dtype=np.int64)
        data = np.concatenate([_f8(a).ravel() for _, a, _ in boxes])
        ids = [_i4(i).ravel() for _, _, i in boxes]
        off = np.concatenate([[0], np.cumsum([len(i) for i in ids])]).astype(np.int64)
        flat = _i4(np.concatenate(ids))
        self.R.ref_tube_load.restype = C.c_int64
        self.n_nodes = int(self.R.ref_tube_load(C.c_int(len(boxes)), _p(desc), C.c_int(boxes[0][1].shape[0]), _p(data), _p(off), _p(flat)))

    def wedges(self, face, pt, comp):
        """-> (wedge_volume_int [nElts], wedge_surf_area at pt [nElts]), or None where a box does not hold pt .. pt + 1"""
        face = _i4(face).ravel()
        vol, area = np.zeros(len(face) // 3), np.zeros(len(face) // 3)
        self.R.ref_tube_wedges.restype = C.c_int
        rc = self.R.ref_tube_wedges(C.c_int64(len(face) // 3), _p(face), C.c_int(int(pt)), C.c_int(int(comp)), _p(vol), _p(area))
        return None if rc else (vol, area)

    def areas(self, face, pt):
        face = _i4(face).ravel()
        area = np.zeros(len(face) // 3)
        self.R.ref_tube_wedges.restype = C.c_int
        rc = self.R.ref_tube_wedges(C.c_int64(len(face) // 3), _p(face), C.c_int(int(pt)), C.c_int(-1), None, _p(area))
        return None if rc else area

    def max_grad(self, comp):
        out = np.zeros(self.n_nodes)
        self.R.ref_tube_max_grad(C.c_int(int(comp)), _p(out))
        return out

    def peaks(self, pcomp, sample_comps):
        sc = _i4(list(sample_comps))
        samples, ok = np.zeros((len(sc), self.n_nodes)), np.zeros(self.n_nodes, dtype=np.uint8)
        self.R.ref_tube_peaks(C.c_int(int(pcomp)), C.c_int(len(sc)), _p(sc), _p(samples), _p(ok))
        return samples, ok.astype(bool)

    def neighbors(self, face, n_nodes):
        """buildNodeNeighbors -> (rowptr [nElts + 1] int64, cols int32); the lists stay loaded for smooth()"""
        face = _i4(face).ravel()
        rp = np.zeros(len(face) // 3 + 1, dtype=np.int64)
        self.R.ref_tube_neighbors.restype = C.c_int64
        n = int(self.R.ref_tube_neighbors(C.c_int64(len(face) // 3), _p(face), C.c_int(int(n_nodes)), _p(rp)))
        cols = np.zeros(n, dtype=np.int32)
        self.R.ref_tube_neighbor_cols(_p(cols))
        return rp, cols

    def smooth(self, vals, area):
        """one pass of smoothVals over the lists of the last neighbors()"""
        vals, area = _f8(vals), _f8(area)
        out = np.zeros(len(vals))
        self.R.ref_tube_smooth(C.c_int64(len(vals)), _p(vals), _p(area), _p(out))
        return out


def lib_tube():
    return O._ref_lib("libtubestats_ref.so", "Src/streamTubeStats.cpp")
