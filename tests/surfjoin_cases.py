"""The case matrix of the surface joining tests (tests/test_surfjoin_ref.py on the CPU, tests/test_gpu_surfjoin.py on the GPU): the
smallest surfaces at which each rule of mergeMEF.cpp / scaleMEF.cpp / multMEF.cpp / combineMEF.cpp can still go wrong, one named case per
rule.  A surface is (nodes [N][ncomp >= 3] float64, elts [M][3] int32, 1-based); node fields beyond x, y, z are seeded random doubles, a
different seed per surface, so that a duplicate's values differ between M and S.
MERGES: name -> dict(M=surface, S=[surface, ...] merged one after the other, eps, rem, path=[per step: "append" | "grid" | "brute"]);
the builder's docstring says which rule the case is for.  `path` is what method = 0 must report; method = 1 is allowed exactly where it says "grid" (or "append": nothing is compared).
The largest inputs are two 64 x 64 grid halves and the 5120-face sphere."""
import functools
import math

import numpy as np

import decimate_cases as DC
from surfcut_cases import _surf, with_fields

NC = 5  # x, y, z and two fields


def _f(xyz, elts1, seed, ncomp=NC):
    return with_fields((np.asarray(xyz, dtype=np.float64).reshape(-1, 3), np.asarray(elts1, dtype=np.int32).reshape(-1, 3)), ncomp, seed)


def _compact(xyz, e1):
    """the nodes the elements use, in their order; elements renumbered"""
    used = np.unique(e1 - 1)
    m = np.full(len(xyz), -1, dtype=np.int64)
    m[used] = np.arange(len(used))
    return xyz[used], (m[e1 - 1] + 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def halves(n, shift=0.0):
    """the n x n patch cut at x = 1/2: left and right half, each with its own copy of the seam column (n + 1 coincident nodes)"""
    xyz, e = DC.grid(n)
    cx = xyz[e - 1][:, :, 0].mean(axis=1)
    out = []
    for k, keep in enumerate((cx < 0.5, cx > 0.5)):
        x, f = _compact(xyz, e[keep])
        out.append(_f(x + shift, f, 300 + 2 * n + k))
    return tuple(out)


def cell_width(eps, ext):
    """the cell width pa_surfjoin.hip chooses (its header): only the neighbour-cell case is BUILT from it; no expected value depends on it"""
    e2 = eps * eps
    r = max(math.sqrt(e2), 2.0 ** -499) * (1.0 + 2.0 ** -40)
    return max(2.0 * r * (1.0 + 2.0 ** -30), ext * 2.0 ** -40)


def cell_of(x, lo, h):
    return math.floor((x - lo) / h)


_OCT = DC.octahedron()
_TRI = [(1, 2, 3)]


def first_match():
    """two nodes of M within eps = 1e-3 of node 0 of S: the farther one (9e-4) has the smaller index, the nearer one (1e-4) the larger"""
    p = np.array([0.3, 0.2, 0.1])
    xm = np.vstack([_OCT[0], p + [9.0e-4, 0, 0], p + [1.0e-4, 0, 0]])
    xs = np.array([p, p + [0.2, 0, 0], p + [0, 0.2, 0]])
    return dict(M=_f(xm, _OCT[1], 1), S=[_f(xs, _TRI, 2)], eps=1.0e-3, rem=True, path=["grid"])


def m_coincident():
    """M holds two more copies of its node 3 and one of its node 7 (no element uses them): S joins the FIRST copy, M's copies stay apart"""
    xyz, e = DC.grid(4)
    xm = np.vstack([xyz, xyz[3], xyz[3], xyz[7]])
    xs = np.array([xyz[3], xyz[7], [2.0, 2.0, 0.0]])
    return dict(M=_f(xm, e, 3), S=[_f(xs, _TRI, 4)], eps=1.0e-8, rem=True, path=["grid"])


def le_exact():
    """eps = 2^-10.  Node 0 of S lies at distance exactly 2^-10 along x from M's node 6 (the origin): dx*dx == eps*eps, joined by the <=.
    Node 1 of S lies one ulp farther along y: its square rounds above eps*eps, not joined.  Node 2 is new."""
    e = 2.0 ** -10
    xm = np.vstack([_OCT[0], [0.0, 0.0, 0.0]])
    xs = np.array([[e, 0.0, 0.0], [0.0, -e * (1.0 + 2.0 ** -52), 0.0], [0.5, 0.5, 0.5]])
    return dict(M=_f(xm, _OCT[1], 5), S=[_f(xs, _TRI, 6)], eps=e, rem=True, path=["grid"])


NEIGHBOURS = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
NB_EPS = 2.0 ** -4


@functools.lru_cache(maxsize=None)
def neighbours26():
    """eps = 2^-4.  For each of the 26 neighbour offsets one pair (node of S, node of M) eps/4 on either side of the cell boundaries the
    offset crosses (a face, an edge or a corner), mid-cell along the other axes: distance (eps/2) sqrt(1, 2 or 3) <= eps.  M's first
    node is its lowest corner (it defines lo): S's node 26 sits eps/2 below it on every axis, in cell (-1, -1, -1), outside M's bounding
    box, and joins it; S's node 27 lies far outside and is new."""
    lo = np.array([-1.0, -2.0, -3.0])
    ext = 3.0 * 27 * NB_EPS * 2 + 1.0
    h = cell_width(NB_EPS, ext)
    xm, xs = [lo.copy()], []
    for k, d in enumerate(NEIGHBOURS):
        base = np.array([3 * k + 2, 2, 2], dtype=np.float64)  # the cell of the S node
        s, m = np.empty(3), np.empty(3)
        for a in range(3):
            if d[a] == 0:
                s[a] = lo[a] + (base[a] + 0.5) * h
                m[a] = s[a]
            else:
                b = lo[a] + (base[a] + (1 if d[a] > 0 else 0)) * h  # the boundary crossed
                s[a] = b - d[a] * NB_EPS / 4
                m[a] = b + d[a] * NB_EPS / 4
        xs.append(s)
        xm.append(m)
    xm.append(lo + [ext, 1.0, 1.0])  # the far corner: fixes M's extent
    xs.append(lo - NB_EPS / 2)
    xs.append(lo - 50.0)
    es = [(k + 1, k + 2, k + 3) for k in range(0, 24, 3)] + [(26, 27, 28)]
    em = [(1, 2, 3), (4, 5, len(xm))]
    return dict(M=_f(xm, em, 7), S=[_f(xs, es, 8)], eps=NB_EPS, rem=True, path=["grid"], lo=lo, h=h)


def s_pair_close():
    """two nodes of S 1e-9 apart and near no node of M: the reference never compares S with itself, both are appended"""
    xs = np.array([[0.4, 0.4, 0.4], [0.4 + 1.0e-9, 0.4, 0.4], [0.0, 0.0, 2.0]])
    return dict(M=_f(*_OCT, 9), S=[_f(xs, _TRI, 10)], eps=1.0e-8, rem=True, path=["grid"])


def three_files():
    """file 2 appends the node (0.4, 0.4, 0.4); node 0 of file 3 matches it: file 3 sees what file 2 added"""
    b = np.array([[0.4, 0.4, 0.4], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    c = np.array([[0.4 + 1.0e-9, 0.4, 0.4], [0.0, 0.0, -3.0], [0.7, 0.7, 0.7]])
    return dict(M=_f(*_OCT, 11), S=[_f(b, _TRI, 12), _f(c, _TRI, 13)], eps=1.0e-8, rem=True, path=["grid", "grid"])


def all_duplicates():
    """every node of S is a node of M (5e-9 away): nothing is appended, the elements of S are dropped, appended == 0"""
    xyz, e = DC.grid(8)
    pick = np.array([0, 9, 10, 40, 80, 44])
    return dict(M=_f(xyz, e, 14), S=[_f(xyz[pick] + [5.0e-9, 0, 0], [(1, 2, 3), (4, 5, 6)], 15)], eps=1.0e-8, rem=True, path=["grid"])


def eps0_zero_sign():
    """eps = 0: only equal coordinates join, and +0.0 equals -0.0 (M's node 0 is (+0, +0, +0); S has (-0, -0, -0)); M keeps its +0.0.
    A node one ulp off does not join."""
    xyz, e = DC.grid(8)
    xs = np.array([[-0.0, -0.0, -0.0], [0.5, 0.25, -0.0], [np.nextafter(0.5, 1.0), 0.5, 0.0]])
    return dict(M=_f(xyz, e, 16), S=[_f(xs, _TRI, 17)], eps=0.0, rem=True, path=["grid"])


def dense_cells():
    """eps = 0.3 on the 8 x 8 patch: the cell width is 0.6, the patch spans 2 x 2 cells of about 20 nodes each; every node of S (the patch
    shifted by 0.01) has dozens of candidates and joins the smallest j within 0.3; one far node is new"""
    xyz, e = DC.grid(8)
    xs = np.vstack([xyz + [0.01, 0.01, 0.0], [5.0, 5.0, 5.0]])
    return dict(M=_f(xyz, e, 18), S=[_f(xs, e, 19)], eps=0.3, rem=True, path=["grid"])


def eps_ge_extent():
    """eps = 2 on the unit patch: fewer than 2 cells span M, auto must report brute force and method = 1 must refuse"""
    xyz, e = DC.grid(8)
    xs = np.vstack([xyz + [0.01, 0.01, 0.0], [5.0, 5.0, 5.0]])
    return dict(M=_f(xyz, e, 20), S=[_f(xs, e, 21)], eps=2.0, rem=True, path=["brute"])


def coords_1e6():
    """the 8 x 8 halves moved to 1e6 (the spacing 1/8 stays exact): the grid still applies"""
    a, b = halves(8, 1.0e6)
    return dict(M=a, S=[b], eps=1.0e-8, rem=True, path=["grid"])


def coords_1e300():
    """coordinates near 1e300, one node of S at 1.5e308: its cell index passes 2^51 -- auto must report brute force, method = 1 must
    refuse.  The squares of the differences overflow to inf and compare false; coincident nodes (dx = 0) still join."""
    xm = _OCT[0] * 1.0e300
    xs = np.vstack([xm[[0, 2, 4]], [1.5e308, 0.0, 0.0], [0.5e300, 0.5e300, 0.0]])
    return dict(M=_f(xm, _OCT[1], 22), S=[_f(xs, [(1, 2, 3), (3, 4, 5)], 23)], eps=1.0e-8, rem=True, path=["brute"])


def nonfinite():
    """NaN, +inf and -inf coordinates in M (left out of the table) and in S (skip the probe): they never match, not even inf with inf
    (inf - inf is NaN); the finite nodes join as usual"""
    xyz, e = DC.grid(4)
    xm = np.array(xyz)
    xm[5, 1] = np.nan
    xm[11] = [np.inf, 0.0, 0.0]
    xm[17, 2] = -np.inf
    xs = np.array([xyz[0], [np.nan, 0.25, 0.0], [np.inf, 0.0, 0.0], [0.0, 0.0, -np.inf], xyz[5], xyz[24], [np.nan, np.nan, np.nan]])
    return dict(M=_f(xm, e, 24), S=[_f(xs, [(1, 2, 3), (4, 5, 6), (5, 6, 7)], 25)], eps=1.0e-8, rem=True, path=["grid"])


def empty_s():
    xyz, e = DC.grid(4)
    return dict(M=_f(xyz, e, 26), S=[_surf(np.zeros((0, NC)), np.zeros((0, 3), dtype=np.int32))], eps=1.0e-8, rem=True, path=["append"])


def m_without_elements():
    xyz, _ = DC.grid(4)
    xs = np.array([xyz[6], [3.0, 0.0, 0.0], [0.0, 3.0, 0.0]])
    return dict(M=_f(xyz, np.zeros((0, 3), dtype=np.int32), 27), S=[_f(xs, _TRI, 28)], eps=1.0e-8, rem=True, path=["grid"])


def degenerate_elements():
    """S carries (1,1,2), an element twice, and one whose three nodes all join M's node 0: all are kept as they are"""
    xyz, e = DC.grid(4)
    xs = np.array([xyz[0], xyz[0] + [1.0e-9, 0, 0], xyz[0] + [0, 1.0e-9, 0], [2.0, 0.0, 0.0], [2.0, 1.0, 0.0]])
    es = [(1, 1, 2), (1, 4, 5), (1, 4, 5), (1, 2, 3), (4, 4, 4)]
    return dict(M=_f(xyz, e, 29), S=[_f(xs, es, 30)], eps=1.0e-8, rem=True, path=["grid"])


@functools.lru_cache(maxsize=None)
def sum_order():
    """a node of S whose squared distance to M's node 6 (the origin) is <= eps*eps summed as ((dx0^2 + dx1^2) + dx2^2) and > eps*eps summed
    from the other end, or the reverse (found by a seeded search): the order of the sum is the reference's"""
    rng = np.random.default_rng(77)
    for _ in range(200000):
        d = rng.uniform(0.2, 1.0, size=3).tolist()
        s1 = ((0.0 + d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2]
        s2 = (d[2] * d[2] + d[1] * d[1]) + d[0] * d[0]
        if s1 == s2:
            continue
        lo, hi = min(s1, s2), max(s1, s2)
        e = math.sqrt(lo)
        for eps in (np.nextafter(e, 0.0), e, np.nextafter(e, 2.0)):
            eps = float(eps)
            if lo <= eps * eps < hi:
                xm = np.vstack([_OCT[0] * 4.0, [0.0, 0.0, 0.0]])
                xs = np.array([d, [9.0, 9.0, 9.0], [9.0, 0.0, 9.0]])
                return dict(M=_f(xm, _OCT[1], 31), S=[_f(xs, _TRI, 32)], eps=eps, rem=True, path=["grid"], joined=s1 <= eps * eps)
    raise AssertionError("no triple found")


def sphere():
    """the 5120-face sphere against itself: the nodes above z = 0.5 moved by 1e-9 (duplicates), the others by 1e-3 (new)"""
    xyz, e = DC.icosphere(4)
    xs = xyz + np.where(xyz[:, 2:3] > 0.5, 1.0e-9, 1.0e-3) * np.array([1.0, 0.0, 0.0])
    return dict(M=_f(xyz, e, 33, 4), S=[_f(xs, e, 34, 4)], eps=1.0e-8, rem=True, path=["grid"])


MERGES = {
    "append_coincident": lambda: dict(M=_f(*DC.grid(8), 35), S=[_f(*DC.grid(8), 36)], eps=1.0e-8, rem=False, path=["append"]),
    "seam8": lambda: dict(M=halves(8)[0], S=[halves(8)[1]], eps=1.0e-8, rem=True, path=["grid"]),
    "seam64": lambda: dict(M=halves(64)[0], S=[halves(64)[1]], eps=1.0e-8, rem=True, path=["grid"]),
    "first_match": first_match,
    "m_coincident": m_coincident,
    "le_exact": le_exact,
    "neighbours26": neighbours26,
    "s_pair_close": s_pair_close,
    "three_files": three_files,
    "all_duplicates": all_duplicates,
    "eps0_zero_sign": eps0_zero_sign,
    "dense_cells": dense_cells,
    "eps_ge_extent": eps_ge_extent,
    "coords_1e6": coords_1e6,
    "coords_1e300": coords_1e300,
    "nonfinite": nonfinite,
    "empty_s": empty_s,
    "m_without_elements": m_without_elements,
    "degenerate_elements": degenerate_elements,
    "sum_order": sum_order,
    "sphere5120": sphere,
}
SMALL = [n for n in MERGES if n not in ("seam64", "sphere5120")]  # the pure-Python double loop stays below a second on these


@functools.lru_cache(maxsize=None)
def merge_case(name):
    return MERGES[name]()


def _special():
    """+-0, inf, NaN and ordinary values in component 3"""
    xyz, e = DC.grid(4)
    nodes = np.array(_f(xyz, e, 40)[0])
    nodes[:6, 3] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.5]
    return _surf(nodes, e)


# scale: name -> (surface, comps, vals)
SCALES = {
    "one": (lambda: _f(*DC.grid(8), 41), [3], [2.5]),
    "twice": (lambda: _f(*DC.grid(8), 42), [4, 0, 4], [0.2, 3.0, 0.3]),           # (d * 0.2) * 0.3, not d * (0.2 * 0.3)
    "special": (_special, [3, 3], [-2.0, 0.0]),                                     # signs of zero, inf * 0 = NaN
    "sphere": (lambda: _f(*DC.icosphere(3), 43, 4), [0, 1, 2, 3], [2.0, 2.0, 2.0, -1.0]),
}
# product: name -> (surface, comps)
PRODUCTS = {
    "one": (lambda: _f(*DC.grid(8), 44), [3]),
    "two": (lambda: _f(*DC.grid(8), 45), [3, 4]),
    "four_repeat": (lambda: _f(*DC.icosphere(3), 46, 6), [3, 5, 3, 4]),
    "special": (_special, [3, 4]),
}
# select: name -> (L, R or None, [(which, comp) ...])
SELECTS = {
    "reorder": (lambda: _f(*DC.grid(8), 47), lambda: _f(*DC.grid(8), 48, 4), [(0, 2), (0, 0), (1, 3), (1, 1), (0, 4)]),
    "repeats": (lambda: _f(*DC.grid(8), 49), lambda: _f(*DC.grid(8), 50), [(1, 4), (1, 4), (0, 0), (0, 0)]),
    "no_r": (lambda: _f(*DC.icosphere(3), 51, 6), None, [(0, 5), (0, 1), (0, 2), (0, 0)]),
    "two_comps": (lambda: _f(*DC.grid(8), 52), lambda: _f(*DC.grid(8), 53), [(0, 3), (1, 3)]),
}
