"""CPU restatement (numpy) of the reference's Src/streamTubeStats.cpp: the key handling and component bookkeeping of main (with its
quirks: the crossed gradient / peak components, the integer 1/nodesPerElt of the auxiliary averages, smoothedInt = output component
4, the at-peak samples that start at the FCR component itself), build_nodeMap, get_jlo / get_nPts, wedge_volume_int / tetVol /
wedge_surf_area, max_grad, peak_val, buildNodeNeighbors, smoothVals and the writers (write_binary_mef_file, write_ascii_tec_file,
stdout).  It is written the reference's way -- per element, per j, per component, calling a wedge_volume_int that recomputes its own
tets -- so it is a formulation independent of pa_tubestats.hip's sharing.  Vectorised over elements (or the lines of a box), never
over j.  Not a test module: test_tubestats_ref.py (CPU) and test_gpu_tubestats.py (GPU, bit for bit) import it.

Two places do not follow the reference text, both on purpose (streamTubeStats3d):
  - max_grad: both passes walk the line's own segments; see max_grad below for what the reference's second pass starts from.
  - out-of-range indices (node ids, components, a j range a box does not hold) raise TubeAbort; the reference asserts in debug builds.
"""
from __future__ import annotations

import numpy as np

import streamsample_ref as S

FAB_HDR = "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))"
PEAK_MSG = "peakVal on end of line!"


class TubeAbort(RuntimeError):
    pass


# ------------------------------------------------------------------------------------------------ the lines in memory
class Lines:
    """The MultiFabs of read_ml_streamline_data: components mem (file indices; X / Y / Z first) of every Str FAB, and nodeMap"""

    def __init__(self, path, mem):
        self.boxes = []  # (lev, b, lo, hi)
        self.fab = []    # [len(mem)][nj][ni]
        nc = len(path["names"])
        for c in mem:
            if c < 0 or c >= nc:
                raise TubeAbort("component %d out of range (the stream file has %d)" % (c, nc))
        gid = {}
        for l, fabs in enumerate(path["levels"]):
            for b, (lo, hi, a) in enumerate(fabs):
                gid[(l, b)] = len(self.boxes)
                self.boxes.append((l, b, lo, hi))
                self.fab.append(np.ascontiguousarray(np.asarray(a)[list(mem)]))
        num = sum(len(ids) for per in path["ins"] for ids in per)  # build_nodeMap (:1256-1281)
        self.node_box = np.full(num, -1, np.int64)
        self.node_pt = np.zeros(num, np.int64)
        for l, per in enumerate(path["ins"]):
            for b, ids in enumerate(per):
                g = gid[(l, b)]
                ni = self.boxes[g][3][0] - self.boxes[g][2][0] + 1
                for k, v in enumerate(ids):
                    if v < 1 or v > num:
                        raise TubeAbort("inside_nodes id %d outside 1 .. %d" % (v, num))
                    if k >= ni:
                        raise TubeAbort("more inside_nodes than lines in a Str box")
                    self.node_box[v - 1], self.node_pt[v - 1] = g, k
        if (self.node_box < 0).any():
            raise TubeAbort("node %d has no inside_nodes entry" % (int(np.argmin(self.node_box)) + 1))
        self.jlo_b = np.array([bx[2][1] for bx in self.boxes], np.int64)
        self.jhi_b = np.array([bx[3][1] for bx in self.boxes], np.int64)

    def get_jlo(self):  # :830-838, placeholders included
        return int(self.jlo_b.min())

    def get_nPts(self):  # :840-848
        return int((self.jhi_b - self.jlo_b + 1).max())

    def val(self, nodes, j, comp):
        """fab(IntVect(pt, j, 0), comp) for an array of 0-based node numbers"""
        out = np.empty(len(nodes))
        g = self.node_box[nodes]
        for q in np.unique(g):
            if j < self.jlo_b[q] or j > self.jhi_b[q]:
                raise TubeAbort("Str box %d (j = %d .. %d) does not hold j = %d" % (q, self.jlo_b[q], self.jhi_b[q], j))
            m = g == q
            out[m] = self.fab[q][comp, j - self.jlo_b[q], self.node_pt[nodes[m]]]
        return out

    def lines_of_box(self, q):
        """0-based node numbers whose line lives in box q, and their i"""
        m = np.nonzero(self.node_box == q)[0]
        return m, self.node_pt[m]


# ------------------------------------------------------------------------------------------------ arithmetic
def tet_vol(A, B, C, D):
    """:850-873, six times the volume; [n][3] each"""
    R1, R2, R3 = D - A, B - A, C - A
    R4 = [R2[:, 1] * R3[:, 2] - R3[:, 1] * R2[:, 2], R2[:, 2] * R3[:, 0] - R3[:, 2] * R2[:, 0], R2[:, 0] * R3[:, 1] - R3[:, 0] * R2[:, 1]]
    res = np.zeros(len(A))
    for i in range(3):
        res = res + R1[:, i] * R4[i]
    return np.abs(res)


def _xyz(L, nodes, j, idX):
    return np.stack([L.val(nodes, j, idX[d]) for d in range(3)], axis=1)


def wedge_surf_area(L, n, idX, pt):
    """:1174-1254, three nodes; n = [3] arrays of node numbers"""
    A, B, C = (_xyz(L, n[k], pt, idX) for k in range(3))
    R1, R2 = B - A, C - A
    R3 = [R1[:, 1] * R2[:, 2] - R2[:, 1] * R1[:, 2], R1[:, 2] * R2[:, 0] - R2[:, 2] * R1[:, 0], R1[:, 0] * R2[:, 1] - R2[:, 0] * R1[:, 1]]
    res = np.zeros(len(A))
    for i in range(3):
        res = res + R3[i] * R3[i]
    return 0.5 * np.sqrt(res)


def wedge_volume_int(L, n, pt, comp, idX):
    """:1003-1172, three nodes: the volume (comp < 0) or the integral of component comp over the wedge pt .. pt + 1"""
    A, B, C = (_xyz(L, n[k], pt, idX) for k in range(3))
    D, E, F = (_xyz(L, n[k], pt + 1, idX) for k in range(3))
    vol_EABC, vol_ADEF, vol_ACEF = tet_vol(A, B, C, E), tet_vol(A, D, E, F), tet_vol(C, E, F, A)
    if comp < 0:
        return (vol_EABC + vol_ADEF + vol_ACEF) / 6.
    vol_DABC, vol_FABC, vol_BDEF = tet_vol(A, B, C, D), tet_vol(A, B, C, F), tet_vol(B, D, E, F)
    vol_CDEF, vol_ACED, vol_BCDF = tet_vol(C, D, E, F), tet_vol(C, E, D, A), tet_vol(B, C, D, F)
    vol_BCDE, vol_ABDF, vol_ABEF = tet_vol(B, C, D, E), tet_vol(B, D, F, A), tet_vol(B, E, F, A)
    vA, vB, vC = (L.val(n[k], pt, comp) for k in range(3))
    vD, vE, vF = (L.val(n[k], pt + 1, comp) for k in range(3))
    int_1 = ((vD + vA + vB + vC) * vol_DABC + (vB + vD + vE + vF) * vol_BDEF + (vB + vC + vD + vF) * vol_BCDF)
    int_2 = ((vD + vA + vB + vC) * vol_DABC + (vC + vD + vE + vF) * vol_CDEF + (vB + vC + vD + vE) * vol_BCDE)
    int_3 = ((vE + vA + vB + vC) * vol_EABC + (vA + vD + vE + vF) * vol_ADEF + (vA + vC + vE + vF) * vol_ACEF)
    int_4 = ((vE + vA + vB + vC) * vol_EABC + (vC + vD + vE + vF) * vol_CDEF + (vA + vC + vE + vD) * vol_ACED)
    int_5 = ((vF + vA + vB + vC) * vol_FABC + (vA + vD + vE + vF) * vol_ADEF + (vA + vB + vE + vF) * vol_ABEF)
    int_6 = ((vF + vA + vB + vC) * vol_FABC + (vB + vD + vE + vF) * vol_BDEF + (vA + vB + vD + vF) * vol_ABDF)
    return (int_1 + int_2 + int_3 + int_4 + int_5 + int_6) / 144.


def _seg(a, idX, i):
    tot = 0
    for d in range(3):
        dx = a[idX[d], i] - a[idX[d], i - 1]
        tot = tot + dx * dx
    return np.sqrt(tot)


def max_grad(L, comp, idX, use_eps=False):
    """:876-952 for every node -> [nNodes].  Two passes along the whole line of the box: maxs = the longest segment, then
    |dv / L| over the segments with L > maxs -- none, so 0 -- or, use_eps (the tool's grad_use_eps=1), L > 1.e-4 * maxs.
    The reference's second pass keeps the coordinates of the line's LAST point from the first pass as the low end of its first
    segment (hiX is not reset at :920); here both passes walk the same segments, which is what its comments describe."""
    out = np.zeros(len(L.node_box))
    for q in range(len(L.boxes)):
        m, pts = L.lines_of_box(q)
        if len(m) == 0:
            continue
        a = L.fab[q][:, :, pts]  # [c][nj][lines]
        nPts = a.shape[1]
        maxs = np.zeros(len(m))
        for i in range(1, nPts):
            Ls = _seg(a, idX, i)
            maxs = Ls if i == 1 else np.where(maxs < Ls, Ls, maxs)  # std::max(maxs, L)
        thr = 1.e-4 * maxs if use_eps else maxs
        gradMax = np.zeros(len(m))
        with np.errstate(divide="ignore", invalid="ignore"):
            for i in range(1, nPts):
                Ls = _seg(a, idX, i)
                grad = np.abs((a[comp, i] - a[comp, i - 1]) / Ls)
                gradMax = np.where((Ls > thr) & (grad >= gradMax), grad, gradMax)
        out[m] = gradMax
    return out


def peak_val(L, pComp, sampleComps):
    """:955-1001 for every node -> (samples [len(sampleComps)][nNodes], ok [nNodes] bool)"""
    nN = len(L.node_box)
    samples, ok = np.zeros((len(sampleComps), nN)), np.zeros(nN, bool)
    for q in range(len(L.boxes)):
        m, pts = L.lines_of_box(q)
        if len(m) == 0:
            continue
        a = L.fab[q][:, :, pts]
        nPts = a.shape[1]
        loc = np.zeros(len(m), np.int64)
        peak = a[pComp, 0].copy()
        for i in range(1, nPts):
            new = a[pComp, i]
            up = new > peak
            peak = np.where(up, new, peak)
            loc = np.where(up, i, loc)
        for s, c in enumerate(sampleComps):
            samples[s, m] = a[c, loc, np.arange(len(m))]
        ok[m] = ~((loc == 0) | (loc == nPts - 1))
    return samples, ok


def build_node_neighbors(face, nNodes):
    """buildNodeNeighbors (:196-235): per element the other elements sharing a node, ascending"""
    nElts = len(face) // 3
    nodeN = [[] for _ in range(nNodes)]
    for i in range(nElts):
        for j in range(3):
            nodeN[face[3 * i + j] - 1].append(i)
    out = []
    for i in range(nElts):
        s = set()
        for j in range(3):
            for nc in nodeN[face[3 * i + j] - 1]:
                if nc != i:
                    s.add(nc)
        out.append(sorted(s))
    return out


def smooth_vals(vals, area, neighbors):
    """smoothVals (:274-298), one pass"""
    new = np.empty(len(vals))
    with np.errstate(divide="ignore", invalid="ignore"):
        for i, nb in enumerate(neighbors):
            accumArea = area[i]
            for n in nb:
                accumArea = accumArea + area[n]
            accumWt = vals[i] * area[i]
            for n in nb:
                accumWt = accumWt + vals[n] * area[n]
            new[i] = np.float64(accumWt) / np.float64(accumArea)
    return new


# ------------------------------------------------------------------------------------------------ files
def out_root(infile):
    """:314-317: infile without its last '.'-separated token (Tokenize skips empty tokens) when the directory part has no '.';
    otherwise only a final .ext of the last path component goes"""
    d, _, base = infile.rpartition("/")
    if "." not in d:
        t = [x for x in infile.split(".") if x]
        return t[0] if len(t) == 1 else ".".join(t[:-1])
    p = base.rfind(".")
    return infile if p <= 0 else infile[:len(infile) - (len(base) - p)]


def read_mef_bytes(b):
    """read_iso (:1721-1763) -> (title, names, nElts, npe, nodes [N][ncomp], conn)"""
    p1 = b.index(b"\n")
    p2 = b.index(b"\n", p1 + 1)
    p3 = b.index(b"\n", p2 + 1)
    p4 = b.index(b"\n", p3 + 1)
    names = b[p1 + 1:p2].decode().replace(",", " ").split()
    nElts, npe = (int(v) for v in b[p2 + 1:p3].split())
    hdr = b[p3 + 1:p4].decode()
    N = int(hdr[hdr.rindex("((0,0,0) (") + 10:].split(",")[0]) + 1
    nodes = np.frombuffer(b, "<f8", N * len(names), p4 + 1).reshape(N, len(names))
    conn = np.frombuffer(b, "<i4", nElts * npe, p4 + 1 + 8 * N * len(names))
    return b[:p1].decode(), names, nElts, npe, nodes, conn


def _fake_nodes(L, face, idX, integrals):
    """the multiply defined nodes of the writers (:1638-1665): [3 * nElts][3 + nCompOut], node-major"""
    nodes = np.asarray(face, np.int64) - 1
    xyz = np.stack([L.val(nodes, 0, idX[d]) for d in range(3)], axis=1)
    return np.concatenate([xyz, np.repeat(integrals, 3, axis=0)], axis=1)


def mef_bytes(outNames, fake, nElts, title="Volume integrals"):
    """write_binary_mef_file (:1610-1704)"""
    nPts, nComp = fake.shape
    head = title + "\n" + "X Y Z" + "".join(" " + n for n in outNames) + "\n" + "%d %d\n" % (nElts, 3)
    head += FAB_HDR + "((0,0,0) (%d,0,0) (0,0,0)) %d\n" % (nPts - 1, nComp)
    return head.encode() + np.ascontiguousarray(fake, "<f8").tobytes() + np.arange(1, nPts + 1, dtype="<i4").tobytes()


def dat_bytes(outNames, fake, nElts, title="Volume integrals"):
    """write_ascii_tec_file (:1542-1607): operator<< at default precision = %g"""
    nPts, nComp = fake.shape
    s = ["VARIABLES = X Y Z" + "".join(" " + n for n in outNames) + "\n", 'ZONE T="%s" N=%d E=%d F=FEBLOCK ET=TRIANGLE\n' % (title, nPts, nElts)]
    for k in range(nComp):
        s.append("".join("%g" % fake[i, k] + ("\n" if i % 5 == 4 else " ") for i in range(nPts)) + "\n")
    for i in range(nElts):
        s.append("%d %d %d \n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))
    return "".join(s).encode()


# ------------------------------------------------------------------------------------------------ the tool
def run_tool(files, infile="strm.sample", *, intComps=(), avgComps=(), peakComp=(), gradComps=(), FCRComp=-1, compsAtPeakFCR=(), namesAtPeakFCR=(),
             aux_mef=None, aux_mef_comps=(), jlo=None, nSmooth=0, write_tec=0, write_mef=1, grad_use_eps=0, verbose=0):
    """main (:300-828) on {relative path: bytes} of a streamSampleFile; aux_mef = the bytes of that file.  -> dict(outNames,
    integrals [nElts][nCompOut], total, root, mef, dat, stdout, peak_lines)"""
    path = S.read_stream_dir(files)
    fileNames = path["names"]
    Nlev, nCompPath = len(path["levels"]), len(fileNames)
    if path["npe"] != 3:
        raise TubeAbort("nodesPerElt = %d: only triangles" % path["npe"])
    compsAtPeakFCR, namesAtPeakFCR = (list(compsAtPeakFCR), list(namesAtPeakFCR)) if FCRComp >= 0 else ([], [])
    auxNames, auxNodes = [], None
    if aux_mef is not None:
        _, anames, _, _, anodes, _ = read_mef_bytes(aux_mef)
        for c in aux_mef_comps:
            if c < 0 or c >= len(anames):
                raise TubeAbort("aux_mef_comps: component %d out of range" % c)
        auxNames = [anames[c] for c in aux_mef_comps]
        auxNodes = anodes[:, list(aux_mef_comps)]
    strComps = list(intComps) + list(avgComps) + list(peakComp) + list(gradComps)  # :414-422: int, avg, PEAK, GRAD
    idPFCR = -1
    if FCRComp >= 0:
        idPFCR = len(strComps)
        strComps += [FCRComp] + compsAtPeakFCR
    out = []
    # read_ml_streamline_names (:1327-1363)
    out.append("NlevPath:  %d\nnCompPath: %d\n" % (Nlev, nCompPath))
    readXYZ = [-1, -1, -1]
    for i, n in enumerate(fileNames):
        for d in range(3):
            if n == "XYZ"[d]:
                readXYZ[d] = i
    if min(readXYZ) < 0:
        raise TubeAbort("the stream file has no component named X, Y or Z")
    for c in strComps:
        if c < 0 or c >= nCompPath:
            raise TubeAbort("component %d out of range (the stream file has %d)" % (c, nCompPath))
    names = ["X", "Y", "Z"] + [fileNames[c] for c in strComps]
    idX = [-1, -1, -1]
    for i, n in enumerate(names):
        for d in range(3):
            if n == "XYZ"[d]:
                idX[d] = i
    nInt, nAvg, nAux, nPeak, nGrad = len(intComps), len(avgComps), len(auxNames), len(peakComp), len(gradComps)
    nPFCR = len(compsAtPeakFCR) if idPFCR >= 0 else 0
    nCompOut = 4 + nInt + nAvg + nAux + nGrad + 2 * nPeak + nPFCR
    oVol, oArea, oWA, oSmInt, oFirstInt = 0, 1, 2, 3, 4
    oFirstAvg = oFirstInt + nInt
    oFirstAux = oFirstAvg + nAvg
    oFirstGr = oFirstAux + nAux
    oFirstPk = oFirstGr + nGrad
    oFirstPkAtFCR = oFirstPk + 2 * nPeak
    outNames = [""] * nCompOut
    outNames[:4] = ["volume", "area", "area_wtAvg", "smoothedInt"]
    namescnt = 3
    sCompInt = namescnt
    for i in range(nInt):
        outNames[oFirstInt + i] = names[namescnt] + "_int"
        namescnt += 1
    sCompAvg = namescnt
    for i in range(nAvg):
        outNames[oFirstAvg + i] = names[namescnt] + "_avg"
        namescnt += 1
    for i in range(nAux):
        outNames[oFirstAux + i] = auxNames[i] + "_avg"
    sCompGr = namescnt  # :502-522 counts int, avg, GRAD, PEAK: crossed with the order in memory
    for i in range(nGrad):
        outNames[oFirstGr + i] = names[namescnt] + "_gradMax"
        namescnt += 1
    sCompPk = namescnt
    for i in range(nPeak):
        outNames[oFirstPk + i] = names[namescnt] + "_peak"
        outNames[oFirstPk + nPeak + i] = outNames[oFirstPk + i] + "OK"
        namescnt += 1
    sCompFCR = namescnt
    for i in range(nPFCR):
        if i >= len(namesAtPeakFCR):
            raise TubeAbort("namesAtPeakFCR has too few values")
        outNames[oFirstPkAtFCR + i] = namesAtPeakFCR[i] + "_at_peakFCR"
    out.append("outNames: " + "".join(n + " " for n in outNames) + "\n")
    for flag, lab, v in ((nInt, "sCompInt", sCompInt), (nAvg, "sCompAvg", sCompAvg), (nPeak, "sCompPk", sCompPk), (nGrad, "sCompGr", sCompGr), (nPFCR, "sCompFCR", sCompFCR)):
        if flag:
            out.append("%s: %d\n" % (lab, v))
    # read_ml_streamline_data (:1365-1453)
    out.append("NlevPath:  %d\nnCompPath: %d\n" % (Nlev, nCompPath))
    out += ["Calling ReadMF() at lev: %d ...\n" % l for l in range(Nlev)]
    L = Lines(path, readXYZ + strComps)
    face, nElts = np.asarray(path["face"], np.int64), path["nElts"]
    nNodes = len(L.node_box)
    if nElts < 1:
        raise TubeAbort("no elements")
    if face.min() < 1 or face.max() > nNodes:
        raise TubeAbort("Elements: node id outside 1 .. %d" % nNodes)
    nPtsOnStr_max = L.get_nPts()
    jl = L.get_jlo() if jlo is None else jlo
    nPtsOnStr = min(nPtsOnStr_max, -2 * jl + 1)
    peak_lines = 0
    grad = [max_grad(L, sCompGr + j, idX, bool(grad_use_eps)) for j in range(nGrad)]
    peak, peakOK = [], []
    for j in range(nPeak):
        s, ok = peak_val(L, sCompPk + j, [sCompPk + j])
        peak.append(s[0])
        peakOK.append(ok)
        peak_lines += int((~ok).sum())
    valsAtPeakFCR = None
    if idPFCR >= 0:
        valsAtPeakFCR, ok = peak_val(L, idPFCR + 3, [sCompFCR + i for i in range(nPFCR)])  # :612-620: the samples start AT the FCR component
        peak_lines += int((~ok).sum())
    if verbose:
        out.append("cnt: %d\n" % len(strComps) + "".join("outNames[%d]: %s\n" % (i, n) for i, n in enumerate(outNames)) + "\n" + "Integrating paths ...\n")
    n = [face[k::3] - 1 for k in range(3)]
    integrals = np.zeros((nElts, nCompOut))
    with np.errstate(divide="ignore", invalid="ignore"):
        integrals[:, oArea] = wedge_surf_area(L, n, idX, 0)
        for j in range(nPtsOnStr - 1):
            jSh = jl + j
            integrals[:, oVol] += wedge_volume_int(L, n, jSh, -1, idX)
            for k in range(nInt):
                thisVolInt = wedge_volume_int(L, n, jSh, sCompInt + k, idX)
                integrals[:, oFirstInt + k] += thisVolInt
                if k == 0:
                    area = 0.5 * (wedge_surf_area(L, n, idX, jSh) + wedge_surf_area(L, n, idX, jSh + 1))
                    integrals[:, oWA] += thisVolInt * area
        total = [0.0] * nInt
        for k in range(nInt):
            for i in range(nElts):
                total[k] = total[k] + integrals[i, oFirstInt + k]
            integrals[:, oFirstInt + k] /= integrals[:, oArea]
        for j in range(nAvg):
            s = np.zeros(nElts)
            for k in range(3):
                s = s + L.val(n[k], 0, sCompAvg + j)
            integrals[:, oFirstAvg + j] = s / 3
        for j in range(nAux):
            if face.max() > len(auxNodes):
                raise TubeAbort("aux_mef has fewer nodes than the stream file")
            s = np.zeros(nElts)
            for k in range(3):
                s = s + auxNodes[n[k], j]
            integrals[:, oFirstAux + j] = s * float(1 // 3)  # :721: 1/nodesPerElt in integer arithmetic
        for j in range(nGrad):
            integrals[:, oFirstGr + j] = (grad[j][n[0]] + grad[j][n[1]] + grad[j][n[2]]) / 3.
        for j in range(nPeak):
            integrals[:, oFirstPk + j] = (peak[j][n[0]] + peak[j][n[1]] + peak[j][n[2]]) / 3.
            integrals[:, oFirstPk + nPeak + j] = (peakOK[j][n[0]] & peakOK[j][n[1]] & peakOK[j][n[2]]).astype(np.float64)
        for j in range(nPFCR):
            v = valsAtPeakFCR[j]
            integrals[:, oFirstPkAtFCR + j] = (v[n[0]] + v[n[1]] + v[n[2]]) / 3.
    integrals[:, oSmInt] = integrals[:, oFirstInt] if nCompOut > oFirstInt else 0.0  # :758-759 (the reference reads past the end when there is nothing else)
    if nSmooth > 0:
        nb = build_node_neighbors(path["face"], nNodes)
        area, vals = integrals[:, 1].copy(), integrals[:, oSmInt].copy()
        for _ in range(nSmooth):
            vals = smooth_vals(vals, area, nb)
        integrals[:, oSmInt] = vals
    root = out_root(infile)
    fake = _fake_nodes(L, face, idX, integrals)
    dat = mef = None
    if write_tec:
        out.append("Building new node data\n")
        dat = dat_bytes(outNames, fake, nElts)
    if write_mef:
        out.append("Building new node data\n")
        mef = mef_bytes(outNames, fake, nElts)
    out.append("Total integrals: \n" + "".join("  %s: %g\n" % (names[3 + j], total[j]) for j in range(nInt)))
    return dict(outNames=outNames, integrals=integrals, total=total, root=root, mef=mef, dat=dat, stdout="".join(out), peak_lines=peak_lines, lines=L, idX=idX,
                jlo=jl, nPtsOnStr=nPtsOnStr)
