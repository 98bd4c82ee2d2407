"""Restatement of the reference's Src/binMEF.cpp in plain Python floats: the area-weighted (joint) PDF of node fields over a triangulated
surface.  Every triangle is clipped recursively against the bin edges of each binned component; the pieces (leaves) add their area to
the bin they lie in.  The tool as a program needs AMReX; its arithmetic (triangleArea through processTriangle) does not: `make -C oracle
ref` compiles it, tests/golden/binmef_ref.npz holds what it returns, and tests/test_surf_reference_pin.py holds this file to that record
leaf by leaf (tests/test_gpu_surf_reference.py: the kernels).  tests/test_binmef_ref.py pins this file with known answers,
tests/test_gpu_binmef.py pins the kernels (peleanalysis_amd/csrc/pa_binmef.hip) with this file.

A vertex is the tuple of ALL node components (x, y, z first); a bin vector is a tuple of one index per binned component.  The
recursion of processTriangle is unrolled onto an explicit stack that visits the calls in the reference's order.

Defined where the reference is undefined: an element with a value that is not finite in x, y, z, a binned component
or the condition component is skipped and counted."""
import math
from bisect import bisect_right

import numpy as np

FAB_DESC = "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))"


def triangle_area(p0, p1, p2):
    """binMEF.cpp:46-60; pow(x, 2) is x * x"""
    a = (p1[1] - p0[1]) * (p2[2] - p0[2]) - (p1[2] - p0[2]) * (p2[1] - p0[1])
    b = (p1[2] - p0[2]) * (p2[0] - p0[0]) - (p1[0] - p0[0]) * (p2[2] - p0[2])
    c = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0])
    return 0.5 * math.sqrt(a * a + b * b + c * c)


def bin_edges(bin_min, bin_max, nbins):
    """:477-489: the lower edges binMin + i * dBin of every component"""
    out = []
    for j in range(len(nbins)):
        d = (bin_max[j] - bin_min[j]) / nbins[j]
        out.append([bin_min[j] + i * d for i in range(nbins[j])])
    return out


def get_bin(val, bin_comps, binLO, bin_max):
    """:168-200: -1 below the first edge, nBins above binMax, else upper_bound - 1 (== binMax is the last bin)"""
    r = []
    for j, c in enumerate(bin_comps):
        v = val[c]
        if v < binLO[j][0]:
            r.append(-1)
        elif v > bin_max[j]:
            r.append(len(binLO[j]))
        else:
            r.append(bisect_right(binLO[j], v) - 1)
    return tuple(r)


def order_nodes(A, Ab, B, Bb, C, Cb, k):
    """:63-90: big to small, three compare-swaps on the bin INDEX of component k"""
    if Bb[k] > Ab[k]:
        A, Ab, B, Bb = B, Bb, A, Ab
    if Cb[k] > Bb[k]:
        B, Bb, C, Cb = C, Cb, B, Bb
    if Bb[k] > Ab[k]:
        A, Ab, B, Bb = B, Bb, A, Ab
    return A, Ab, B, Bb, C, Cb


class SplitFractionError(ArithmeticError):
    """the reference's AMREX_ALWAYS_ASSERT at :121 / :159"""


def find_de(A, B, C, lo, bmax, abin, comp):
    """:93-129: A and B share the top bin; cut AC and BC at its lower edge"""
    if abin < 0:
        fAC = (lo[0] - A[comp]) / (C[comp] - A[comp])
        fBC = (lo[0] - B[comp]) / (C[comp] - B[comp])
    elif abin >= len(lo):
        fAC = (A[comp] - bmax) / (A[comp] - C[comp])
        fBC = (B[comp] - bmax) / (B[comp] - C[comp])
    else:
        fAC = (A[comp] - lo[abin]) / (A[comp] - C[comp])
        fBC = (B[comp] - lo[abin]) / (B[comp] - C[comp])
    if not (0 <= fAC <= 1 and 0 <= fBC <= 1):
        raise SplitFractionError("split fraction outside [0, 1]")
    D = tuple(a - fAC * (a - c) for a, c in zip(A, C))
    E = tuple(b - fBC * (b - c) for b, c in zip(B, C))
    return D, E


def find_fg(A, B, C, lo, bmax, abin, comp):
    """:132-165: A alone in the top bin; cut AB and AC at its lower edge"""
    if abin < 0:
        fAB = (lo[0] - A[comp]) / (A[comp] - B[comp])
        fAC = (lo[0] - C[comp]) / (A[comp] - C[comp])
    elif abin >= len(lo):
        fAB = (A[comp] - bmax) / (A[comp] - B[comp])
        fAC = (A[comp] - bmax) / (A[comp] - C[comp])
    else:
        fAB = (A[comp] - lo[abin]) / (A[comp] - B[comp])
        fAC = (A[comp] - lo[abin]) / (A[comp] - C[comp])
    if not (0 <= fAB <= 1 and 0 <= fAC <= 1):
        raise SplitFractionError("split fraction outside [0, 1]")
    F = tuple(a - fAB * (a - b) for a, b in zip(A, B))
    G = tuple(a - fAC * (a - c) for a, c in zip(A, C))
    return F, G


def satisfy_condition(A, B, C, cond_comp, cond_val, cond_sgn):
    """:206-226"""
    a, b, c = A[cond_comp], B[cond_comp], C[cond_comp]
    if cond_sgn > 0:
        return a > cond_val and b > cond_val and c > cond_val
    if cond_sgn < 0:
        return a < cond_val and b < cond_val and c < cond_val
    return a == cond_val and b == cond_val and c == cond_val


def flat_key(bins, nbins):
    """the position of a bin vector in the lexicographic order of the reference's std::map"""
    k = 0
    for b, n in zip(bins, nbins):
        k = k * n + b
    return k


class Binned:
    """what bin_surface returns: keys / areas of the leaves in visiting order (the terms), the area of every element, the leaf areas that
    failed the condition, NmyTriangles, the skipped elements and the deepest recursion"""

    def __init__(self):
        self.keys, self.areas, self.elem_areas, self.outside = [], [], [], []
        self.n_my = 0
        self.nonfinite = 0
        self.depth = 0
        self.nbins = ()

    def table(self):
        """dense (area by math.fsum, hits) in flat key order"""
        nt = int(np.prod(self.nbins, dtype=np.int64))
        per = [[] for _ in range(nt)]
        for k, a in zip(self.keys, self.areas):
            per[k].append(a)
        return np.array([math.fsum(p) for p in per]), np.array([len(p) for p in per], dtype=np.int64)

    def table_serial(self):
        """the reference's own sums: bins[k] += area in visiting order"""
        nt = int(np.prod(self.nbins, dtype=np.int64))
        area, hits = np.zeros(nt), np.zeros(nt, dtype=np.int64)
        for k, a in zip(self.keys, self.areas):
            area[k] += a
            hits[k] += 1
        return area, hits


def bin_surface(nodes, elts, bin_comps, bin_min, bin_max, nbins, cond_apply=False, cond_comp=0, cond_val=0.0, cond_sgn=0, area_eps=1.0e-20):
    """the element loop (:522-540) and processTriangle (:231-331).  nodes [N][nComp], elts [M][3] 1-based."""
    nc = len(bin_comps)
    bin_comps = [int(c) for c in bin_comps]
    bin_min, bin_max = [float(v) for v in bin_min], [float(v) for v in bin_max]
    nbins = [int(n) for n in nbins]
    binLO = bin_edges(bin_min, bin_max, nbins)
    used = sorted(set([0, 1, 2] + bin_comps + ([int(cond_comp)] if cond_apply else [])))
    P = [tuple(float(v) for v in row) for row in np.asarray(nodes, dtype=np.float64)]
    R = Binned()
    R.nbins = tuple(nbins)
    for e in np.asarray(elts):
        A, B, C = P[int(e[0]) - 1], P[int(e[1]) - 1], P[int(e[2]) - 1]
        if not all(math.isfinite(V[c]) for V in (A, B, C) for c in used):
            R.nonfinite += 1
            continue
        R.elem_areas.append(triangle_area(A, B, C))  # :535, before the areaEps test
        stack = [(A, get_bin(A, bin_comps, binLO, bin_max), B, get_bin(B, bin_comps, binLO, bin_max), C, get_bin(C, bin_comps, binLO, bin_max), 0, 1)]
        while stack:
            A, Ab, B, Bb, C, Cb, k, depth = stack.pop()
            if depth > R.depth:
                R.depth = depth
            area = triangle_area(A, B, C)
            if area < area_eps:  # :244, at EVERY call
                continue
            if k >= nc:  # :248-269
                if all(0 <= Ab[i] < nbins[i] for i in range(nc)):
                    R.n_my += 1
                    if (not cond_apply) or satisfy_condition(A, B, C, cond_comp, cond_val, cond_sgn):
                        R.keys.append(flat_key(Ab, nbins))
                        R.areas.append(area)
                    else:
                        R.outside.append(area)
                continue
            if Ab[k] == Bb[k] and Bb[k] == Cb[k]:  # :270-274
                stack.append((A, Ab, B, Bb, C, Cb, k + 1, depth + 1))
                continue
            A, Ab, B, Bb, C, Cb = order_nodes(A, Ab, B, Bb, C, Cb, k)
            if Ab[k] == Bb[k]:  # :284-306
                D, E = find_de(A, B, C, binLO[k], bin_max[k], Ab[k], bin_comps[k])
                Db, Eb = get_bin(D, bin_comps, binLO, bin_max), get_bin(E, bin_comps, binLO, bin_max)
                Db = Ab[:k + 1] + Db[k + 1:]  # :291-295: bins 0..binID of the new vertices are A's
                Eb = Db[:k + 1] + Eb[k + 1:]
                Db2 = Db[:k] + (Ab[k] - 1,) + Db[k + 1:]  # :302-303: the far side
                Eb2 = Eb[:k] + (Eb[k] - 1,) + Eb[k + 1:]
                calls = [(A, Ab, B, Bb, E, Eb, k + 1, depth + 1), (A, Ab, E, Eb, D, Db, k + 1, depth + 1), (D, Db2, C, Cb, E, Eb2, k, depth + 1)]
            else:  # :307-329
                F, G = find_fg(A, B, C, binLO[k], bin_max[k], Ab[k], bin_comps[k])
                Fb, Gb = get_bin(F, bin_comps, binLO, bin_max), get_bin(G, bin_comps, binLO, bin_max)
                Fb = Ab[:k + 1] + Fb[k + 1:]
                Gb = Fb[:k + 1] + Gb[k + 1:]
                Fb2 = Fb[:k] + (Ab[k] - 1,) + Fb[k + 1:]
                Gb2 = Gb[:k] + (Ab[k] - 1,) + Gb[k + 1:]
                calls = [(A, Ab, F, Fb, G, Gb, k + 1, depth + 1), (F, Fb2, B, Bb, C, Cb, k, depth + 1), (F, Fb2, C, Cb, G, Gb2, k, depth + 1)]
            stack.extend(reversed(calls))  # the reference's order of the child calls
    return R


def cxx(v):
    """operator<<(double) with the default precision of 6"""
    return "%g" % v


def tool_output(area, hits, bin_comps, bin_min, bin_max, nbins, total_area, outside_area=None, dump_fab=False, normalize=False, dump_bins=False,
                n_my=None, nonfinite=0):
    """:491-501 and :594-670 from a finished table (dense, flat key order).  A bin is nonempty when it was touched (hits > 0): with
    areaEps <= 0 a touched bin can hold 0.  Returns (stdout text, stderr lines, .fab bytes or None, binSum)."""
    nc = len(nbins)
    binLO = bin_edges([float(v) for v in bin_min], [float(v) for v in bin_max], [int(n) for n in nbins])
    out = ""
    if dump_bins:
        for j in range(nc):
            out += "bin: %d bounds: \n" % bin_comps[j]
            for i in range(nbins[j]):
                hi = bin_max[j] if i == nbins[j] - 1 else binLO[j][i + 1]
                out += "         bin: [%s,%s]\n" % (cxx(binLO[j][i]), cxx(float(hi)))
            out += "\n"
    keys = [int(k) for k in np.nonzero(np.asarray(hits) > 0)[0]]  # flat order IS the map's lexicographic order
    err = ["number of nonempty bins: %d" % len(keys)]
    bin_sum = 0.0
    for k in keys:  # :599-601: serial, in key order
        bin_sum += float(area[k])
    fab = None
    if dump_fab and nc <= 2:
        n0, n1 = nbins[0], (nbins[1] if nc == 2 else 1)
        data = np.zeros((n1, n0))  # x = component 0 runs fastest
        for k in keys:
            b0, b1 = (k // n1, k % n1) if nc == 2 else (k, 0)
            data[b1, b0] = area[k]
        if normalize:
            data = data * (1. / bin_sum)  # :637: mult by the reciprocal
        fab = (FAB_DESC + "((0,0,0) (%d,%d,0) (0,0,0)) 1\n" % (n0 - 1, n1 - 1)).encode() + data.astype("<f8").tobytes()
    else:
        for k in keys:
            idx, r = [], k
            for n in reversed(nbins):
                idx.append(r % n)
                r //= n
            idx.reverse()
            for j in range(nc):
                lo = binLO[j][idx[j]]
                hi = float(bin_max[j]) if idx[j] == nbins[j] - 1 else binLO[j][idx[j] + 1]
                out += cxx(0.5 * (lo + hi)) + " "
            out += cxx(float(area[k])) + "\n"
    err.append("Total area of this surface: %s (sum of bins: %s)" % (cxx(total_area), cxx(bin_sum)))
    if outside_area is not None:
        err.append("   area outside condition: %s (total: %s)" % (cxx(outside_area), cxx(outside_area + bin_sum)))
    if nonfinite:
        err.append("skipped %d elements with a value that is not finite" % nonfinite)
    return out, err, fab, bin_sum


# ----------------------------------------------------------------------------- the test surface
def latlong_sphere(n):
    """unit sphere of 2n latitude bands x n longitude sectors, two triangles per quad: 4 n^2 elements, of which the 2n at the poles
    have two coincident vertices (zero area exactly: sin is set to 0 there).  Node components: x y z T s with
    T = 300 + 1700 (1/2 + 1/2 tanh(3z + 0.7xy)) and s = sin 5x cos 3y + 0.2z.  Returns (nodes [N][5], elts [M][3] 1-based int32)."""
    nlat, nlon = 2 * n, n
    nodes = []
    for i in range(nlat + 1):
        th = math.pi * i / nlat
        st = 0.0 if i in (0, nlat) else math.sin(th)
        ct = 1.0 if i == 0 else (-1.0 if i == nlat else math.cos(th))
        for j in range(nlon):
            ph = 2.0 * math.pi * j / nlon
            x, y, z = st * math.cos(ph), st * math.sin(ph), ct
            T = 300.0 + 1700.0 * (0.5 + 0.5 * math.tanh(3.0 * z + 0.7 * x * y))
            s = math.sin(5.0 * x) * math.cos(3.0 * y) + 0.2 * z
            nodes.append((x, y, z, T, s))
    elts = []
    for i in range(nlat):
        for j in range(nlon):
            a, b = i * nlon + j, i * nlon + (j + 1) % nlon
            d, c = (i + 1) * nlon + j, (i + 1) * nlon + (j + 1) % nlon
            elts.append((a + 1, b + 1, c + 1))
            elts.append((a + 1, c + 1, d + 1))
    return np.array(nodes, dtype=np.float64), np.array(elts, dtype=np.int32)


NAMES = ("X", "Y", "Z", "T", "s")
# case -> (n, binComps, binMin, binMax, nBins): tests/test_gpu_binmef.py
CASES = {
    "n8_16x16": (8, (3, 4), (350.0, -0.9), (1950.0, 0.9), (16, 16)),
    "n24_32x8": (24, (3, 4), (350.0, -0.9), (1950.0, 0.9), (32, 8)),
    "n4_128": (4, (3,), (350.0,), (1950.0,), (128,)),
    "n6_8x8x8": (6, (3, 4, 2), (350.0, -0.9, -1.0), (1950.0, 0.9, 1.0), (8, 8, 8)),
    "onebin": (8, (3, 4), (0.0, -2.0), (3000.0, 2.0), (1, 1)),
    "allout": (8, (3,), (5000.0,), (6000.0,), (4,)),
    # not one of the six named cases: two components on a list of 1000 items, sliced from the first round on
    "n12_32x32": (12, (3, 4), (350.0, -0.9), (1950.0, 0.9), (32, 32)),
}


def mef_bytes(nodes, elts, names=NAMES, title="0"):
    """the MEF layout the surface tools write: title, names, 'nElts 3', the node FAB (node-major), 1-based int32 triples"""
    nodes = np.ascontiguousarray(nodes, dtype="<f8")
    head = "%s\n%s\n%d 3\n" % (title, " ".join(names), len(elts))
    head += FAB_DESC + "((0,0,0) (%d,0,0) (0,0,0)) %d\n" % (len(nodes) - 1, nodes.shape[1])
    return head.encode() + nodes.tobytes() + np.ascontiguousarray(elts, dtype="<i4").tobytes()
