"""CPU restatement (numpy) of the gradient-streamline tool of the reference, Src/stream.cpp with the Fortran of
Src/stream_nd.f90: seed handling (push_nodes_inside, trim_surface, setInsideNodes), the state preparation of
stream.cpp:796-884, vtrace / RK4 / ntrpv / vnrml, and the bytes of both writers (write_ml_streamline_data,
dump_ml_streamline_data).  Every step is vectorised over the seeds of one box.  Not a test module: the tests of
test_streamgrad_ref.py (CPU) and test_gpu_streamgrad.py (GPU, bit for bit) import it.

Nodes are component-major arrays [3][N] (the node FAB of stream.cpp:451-471); states are hierarchy.MultiFab's
(components: progress, [x/y/z_velocity], aux...; nGrow ghost layers)."""
from __future__ import annotations

import numpy as np

from peleanalysis_amd.hierarchy import Level, MultiFab

EPS_PUSH = 1.0e-4                       # stream.cpp:30
EPS_VNRML = float(np.float32(1.0e-12))  # stream_nd.f90:216, `parameter (eps=1.e-12)`: a default-real literal


# ------------------------------------------------------------------------------------------------ seeds
def push_nodes_inside(nodes: np.ndarray, plo, phi, eps_push: float) -> None:
    """stream.cpp:116-134, in place: x = max(plo + eps, min(phi - eps, x))"""
    for d in range(3):
        nodes[d] = np.maximum(plo[d] + eps_push, np.minimum(phi[d] - eps_push, nodes[d]))


def trim_surface(bbll, bbur, nodes: np.ndarray, face: np.ndarray, npe: int):
    """stream.cpp:218-290: drop nodes outside [bbll, bbur] (closed), then every element that uses a dropped node;
    the rest are renumbered (1-based).  Returns (nodes, face)."""
    x, y, z = nodes[0], nodes[1], nodes[2]
    rm = (x < bbll[0]) | (x > bbur[0]) | (y < bbll[1]) | (y > bbur[1]) | (z < bbll[2]) | (z > bbur[2])
    idx = np.where(rm, -1, np.cumsum(~rm) - 1)
    newnodes = np.ascontiguousarray(nodes[:, ~rm])
    f = np.asarray(face, dtype=np.int64).reshape(-1, npe)
    mapped = idx[f - 1]
    good = np.all(mapped >= 0, axis=1)
    return newnodes, (mapped[good] + 1).astype(np.int32).ravel()


def level_dx(lv: Level) -> np.ndarray:
    """stream.cpp:718-719: dx = ProbSize / ProbDomain[lev].length (not the file's dx)"""
    return (lv.prob_hi - lv.prob_lo) / (lv.domhi - lv.domlo + 1).astype(np.float64)


def coarsen_box(b, r):
    return np.concatenate([np.floor_divide(b[:3], r), np.floor_divide(b[3:], r)])


def ratio_of(fine: Level, crse: Level) -> int:
    return int((fine.domhi[0] - fine.domlo[0] + 1) // (crse.domhi[0] - crse.domlo[0] + 1))


def inside_nodes(levels, nodes: np.ndarray):
    """stream.cpp:710-766 + setInsideNodes (:141-216): per level, per FILE box, the 1-based ids (node order) of the nodes in
    [plo + lo dx, plo + (hi+1) dx) (half-open, recomputed dx) and in no coarsened finer box that intersects it (same test).
    A node in no box appears nowhere."""
    out = []
    for l, lv in enumerate(levels):
        dx = level_dx(lv)
        plo = lv.prob_lo
        fc = None
        if l + 1 < len(levels):
            r = ratio_of(levels[l + 1], lv)
            fc = np.array([coarsen_box(b, r) for b in levels[l + 1].boxes])
        per_box = []
        for b in lv.boxes:
            lo = plo + b[:3] * dx
            hi = plo + (b[3:] + 1.0) * dx
            isin = np.all((nodes >= lo[:, None]) & (nodes < hi[:, None]), axis=0)
            if fc is not None:
                for f in fc:  # baf_c.intersections(box): only the coarsened fine boxes that meet this box
                    if np.any(np.maximum(f[:3], b[:3]) > np.minimum(f[3:], b[3:])):
                        continue
                    ilo, ihi = np.maximum(f[:3], b[:3]), np.minimum(f[3:], b[3:])
                    flo = plo + ilo * dx
                    fhi = plo + (ihi + 1.0) * dx
                    infine = np.all((nodes >= flo[:, None]) & (nodes < fhi[:, None]), axis=0)
                    isin &= ~infine
            per_box.append((np.nonzero(isin)[0] + 1).astype(np.int32))
        out.append(per_box)
    return out


# ------------------------------------------------------------------------------------------------ state
def _owner_grid(lv: Level, lo, hi):
    """index of the box owning each cell of [lo, hi] (-1: none); array [z][y][x]"""
    n = np.asarray(hi) - np.asarray(lo) + 1
    own = np.full((n[2], n[1], n[0]), -1, dtype=np.int64)
    for bi, b in enumerate(lv.boxes):
        a = np.maximum(b[:3], lo) - lo
        e = np.minimum(b[3:], hi) - lo
        if np.any(a > e):
            continue
        own[a[2]:e[2] + 1, a[1]:e[1] + 1, a[0]:e[0] + 1] = bi
    return own


def _fab_cells(lv: Level, b: int, ng: int):
    lo = lv.boxes[b, :3] - ng
    nz, ny, nx = lv.box_shape(b, ng)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return i + lo[0], j + lo[1], k + lo[2]


def fill_boundary(mf: MultiFab, periodic: bool = True) -> None:
    """FillBoundary: every ghost cell that is (a periodic image of, when the direction is periodic) a valid cell of the level"""
    lv, ng = mf.level, mf.ng
    n = lv.domhi - lv.domlo + 1
    shifts = [(sx, sy, sz) for sz in (-1, 0, 1) for sy in (-1, 0, 1) for sx in (-1, 0, 1)
              if periodic and all(s == 0 or lv.is_per[d] for d, s in enumerate((sx, sy, sz)))] or [(0, 0, 0)]
    for b in range(lv.nboxes):
        f = mf.fab(b)
        glo = lv.boxes[b, :3] - ng
        ghi = lv.boxes[b, 3:] + ng
        for s in shifts:
            sh = np.asarray(s) * n
            for o in range(lv.nboxes):
                if o == b and not any(s):
                    continue
                olo, ohi = lv.boxes[o, :3] + sh, lv.boxes[o, 3:] + sh
                a, e = np.maximum(glo, olo), np.minimum(ghi, ohi)
                if np.any(a > e):
                    continue
                src = mf.valid(o)
                f[:, a[2] - glo[2]:e[2] - glo[2] + 1, a[1] - glo[1]:e[1] - glo[1] + 1, a[0] - glo[0]:e[0] - glo[0] + 1] = \
                    src[:, a[2] - olo[2]:e[2] - olo[2] + 1, a[1] - olo[1]:e[1] - olo[1] + 1, a[0] - olo[0]:e[0] - olo[0] + 1]


class NestingError(RuntimeError):
    pass


def _fill_cf(levels, l: int, fine: MultiFab, crse_src: MultiFab) -> None:
    """FillCFgrowCells (stream.cpp:63-99) + the bigMF copy of :836-845: every cell of a fine FAB (ghosts) that no fine box covers
    (index test, no wrap) gets the value at its parent cell in the grown coarse FABs (after crse_src.FillBoundary).  The coarse
    cells are those of GetBndryCells(coarsen(fine BA), nGrow): a parent that the coarsened fine BoxArray covers, or that no grown
    coarse FAB holds, is never set there -> NestingError."""
    lv, cl = levels[l], levels[l - 1]
    r = ratio_of(lv, cl)
    ng = fine.ng
    fc = np.array([coarsen_box(b, r) for b in lv.boxes])
    for b in range(lv.nboxes):
        i, j, k = _fab_cells(lv, b, ng)
        glo, ghi = lv.boxes[b, :3] - ng, lv.boxes[b, 3:] + ng
        own = _owner_grid(lv, glo, ghi)
        cf = own < 0
        if not cf.any():
            continue
        qi, qj, qk = np.floor_divide(i, r), np.floor_divide(j, r), np.floor_divide(k, r)
        val = np.zeros((fine.ncomp,) + i.shape)
        done = np.zeros(i.shape, dtype=bool)
        # an unset value outside the index domain is harmless: FixOOB zeroes the cell afterwards
        inside = ((i >= lv.domlo[0]) & (i <= lv.domhi[0]) & (j >= lv.domlo[1]) & (j <= lv.domhi[1]) & (k >= lv.domlo[2]) & (k <= lv.domhi[2]))
        for f in fc:
            covered = (qi >= f[0]) & (qi <= f[3]) & (qj >= f[1]) & (qj <= f[4]) & (qk >= f[2]) & (qk <= f[5])
            if np.any(covered & cf & inside):
                raise NestingError("a coarse-fine ghost cell's parent lies in the coarsened fine BoxArray (unset in FillCFgrowCells)")
        for c in range(cl.nboxes):
            cg = crse_src.ng
            clo, chi = cl.boxes[c, :3] - cg, cl.boxes[c, 3:] + cg
            inb = cf & ~done & (qi >= clo[0]) & (qi <= chi[0]) & (qj >= clo[1]) & (qj <= chi[1]) & (qk >= clo[2]) & (qk <= chi[2])
            if not inb.any():
                continue
            cfab = crse_src.fab(c)
            val[:, inb] = cfab[:, qk[inb] - clo[2], qj[inb] - clo[1], qi[inb] - clo[0]]
            done |= inb
        if np.any(cf & ~done & inside):
            raise NestingError("a coarse-fine ghost cell's parent lies in no grown coarse FAB (unset in FillCFgrowCells)")
        fab = fine.fab(b)
        fab[:, cf] = val[:, cf]


def fix_oob(mf: MultiFab) -> None:
    """FixOOB (stream.cpp:384-392): every cell outside the index domain becomes 0"""
    lv = mf.level
    for b in range(lv.nboxes):
        i, j, k = _fab_cells(lv, b, mf.ng)
        out = (i < lv.domlo[0]) | (i > lv.domhi[0]) | (j < lv.domlo[1]) | (j > lv.domhi[1]) | (k < lv.domlo[2]) | (k > lv.domhi[2])
        mf.fab(b)[:, out] = 0.0


def prepare_states(levels, raw):
    """stream.cpp:796-884 for all levels: raw[l] = MultiFab with the file's data in the valid cells (ghosts ignored).  Returns
    the states each level's vtrace reads.  The coarse source of level l+1 is level l's state after ANOTHER FillBoundary
    (FillCFgrowCells' first line mutates state[lev-1] -- after its trace, so the trace sees the FixOOB'd state)."""
    out = []
    src_prev = None
    for l, lv in enumerate(levels):
        s = MultiFab(lv, raw[l].ncomp, raw[l].ng)  # setVal(0) + FillVar (:804-805)
        for b in range(lv.nboxes):
            s.valid(b)[...] = raw[l].valid(b)
        fill_boundary(s)                       # :820
        if l > 0:
            _fill_cf(levels, l, s, src_prev)   # :822-844
        fill_boundary(s)                       # :849
        fix_oob(s)                             # :866-870
        out.append(s)
        src_prev = s.copy()
        fill_boundary(src_prev)                # FillCFgrowCells :71, for the next level
    return out


# ------------------------------------------------------------------------------------------------ vtrace
class Fab:
    """a FAB as vtrace sees it: data [ncomp][nz][ny][nx] on lo..hi"""

    def __init__(self, data, lo):
        self.a = data
        self.lo = np.asarray(lo, dtype=np.int64)
        self.hi = self.lo + np.array(data.shape[:0:-1]) - 1


def _locate(x, dx, plo, phi, blo, bhi):
    """ntrpv up to the sum (stream_nd.f90:158-192); x [n][3]"""
    ok = ~np.any((x < plo) | (x > phi), axis=1)
    with np.errstate(invalid="ignore"):
        tmp = (x - plo) / dx - 0.5
        fl = np.floor(tmp)
        b = np.where(np.isfinite(fl), fl, 0).astype(np.int64)
        n = (x - ((b + 0.5) * dx + plo)) / dx
    n = np.where(n < 1.0, n, 1.0)
    n = np.where(0.0 < n, n, 0.0)
    ok &= np.all((b >= blo) & (b <= bhi - 1), axis=1)
    return ok, np.where(ok[:, None], b, blo), n


def _sum8(n, f):
    n1, n2, n3 = n[:, 0], n[:, 1], n[:, 2]
    return (+n1 * n2 * n3 * f(1, 1, 1)
            + n1 * (1.0 - n2) * n3 * f(1, 0, 1)
            + n1 * n2 * (1.0 - n3) * f(1, 1, 0)
            + n1 * (1.0 - n2) * (1.0 - n3) * f(1, 0, 0)
            + (1.0 - n1) * n2 * n3 * f(0, 1, 1)
            + (1.0 - n1) * (1.0 - n2) * n3 * f(0, 0, 1)
            + (1.0 - n1) * n2 * (1.0 - n3) * f(0, 1, 0)
            + (1.0 - n1) * (1.0 - n2) * (1.0 - n3) * f(0, 0, 0))


def ntrpv(x, F: Fab, comps, dx, plo, phi):
    """-> ok [n], u [len(comps)][n]"""
    ok, b, n = _locate(x, dx, plo, phi, F.lo, F.hi)
    r = b - F.lo
    u = np.empty((len(comps), len(x)))
    for q, m in enumerate(comps):
        A = F.a[m]
        u[q] = _sum8(n, lambda di, dj, dk: A[r[:, 2] + dk, r[:, 1] + dj, r[:, 0] + di])
    return ok, u


def vnrml(v):
    """stream_nd.f90:213-225; v [3][n]"""
    s = 0.0 + v[0] * v[0]
    s = s + v[1] * v[1]
    s = s + v[2] * v[2]
    big = s > EPS_VNRML
    r = np.sqrt(np.where(big, s, 1.0))
    return np.where(big[None, :], v / r[None, :], v)


def rk4(x, h, G: Fab, gcomps, dx, plo, phi):
    """stream_nd.f90:122-156; x [n][3] -> (ok, new x) -- x kept where a stage fails"""
    ok, v = ntrpv(x, G, gcomps, dx, plo, phi)
    v = vnrml(v)
    k1 = v.T * h
    ok2, v = ntrpv(x + k1 * 0.5, G, gcomps, dx, plo, phi)
    v = vnrml(v)
    k2 = v.T * h
    ok3, v = ntrpv(x + k2 * 0.5, G, gcomps, dx, plo, phi)
    v = vnrml(v)
    k3 = v.T * h
    ok4, v = ntrpv(x + k3, G, gcomps, dx, plo, phi)
    v = vnrml(v)
    k4 = v.T * h
    allok = ok & ok2 & ok3 & ok4
    xn = x + (k1 + k4) / 6.0 + (k2 + k3) / 3.0
    return allok, np.where(allok[:, None], xn, x)


def gradient_fab(T: Fab, glo, ghi) -> Fab:
    """stream_nd.f90:33-44: g = T(i+1) - T(i-1) per direction over glo..ghi (neither scaled nor normalised)"""
    glo, ghi = np.asarray(glo), np.asarray(ghi)
    a = T.a[0]
    o = glo - T.lo
    e = ghi - T.lo
    sl = lambda d, s: tuple(slice(o[q] + (s if q == d else 0), e[q] + 1 + (s if q == d else 0)) for q in (2, 1, 0))
    g = np.empty((3,) + tuple((ghi - glo + 1)[::-1]))
    for d in range(3):
        g[d] = a[sl(d, +1)] - a[sl(d, -1)]
    return Fab(g, glo)


def vtrace(T: Fab, nT: int, loc: np.ndarray, ids, G: Fab | None, gcomps, nRKsteps: int, dx, plo, phi, hRK: float):
    """stream_nd.f90:11-108 for one box.  T: the state FAB (nT comps); loc [3][N]; ids 1-based; G: the vector field FAB
    (None: computeVec = 1, g over T's box grown by -1); gcomps: its 3 components.  -> (strm [3+nT][nRKsteps][n], errFlag)"""
    ids = np.asarray(ids, dtype=np.int64)
    nRKh = (nRKsteps - 1) // 2
    if G is None:
        G = gradient_fab(T, T.lo + 1, T.hi - 1)
        gcomps = (0, 1, 2)
    dx, plo, phi = (np.asarray(v, dtype=np.float64) for v in (dx, plo, phi))
    n = len(ids)
    strm = np.zeros((3 + nT, nRKsteps, n))
    x0 = np.ascontiguousarray(loc[:, ids - 1].T)
    comps = list(range(nT))
    ok0, u0 = ntrpv(x0, T, comps, dx, plo, phi)
    if not ok0.all():
        return strm, 1
    strm[:3, nRKh] = x0.T
    strm[3:, nRKh] = u0
    events = np.zeros(n, dtype=np.int64)  # last cut-short event of each seed: 2 * i + dir + 1 (dir 1 = forward)
    for sgn, nlen, h in ((-1, nRKh, -hRK), (+1, nRKsteps - 1 - nRKh, hRK)):
        x = x0.copy()
        for s in range(1, nlen + 1):
            j = nRKh + sgn * s
            ok, x = rk4(x, h, G, gcomps, dx, plo, phi)
            events = np.where(~ok, 2 * np.arange(n) + (sgn > 0) + 1, events)
            strm[:3, j] = x.T
            oku, u = ntrpv(x, T, comps, dx, plo, phi)
            strm[3:, j] = np.where(oku[None, :], u, strm[3:, j - sgn])
    e = int(events.max()) if n else 0
    return strm, 0 if e == 0 else (4 if (e - 1) & 1 else 2)


def trace_hierarchy(levels, states, nodes, ins, nRKsteps: int, hRK: float, vcomp: int | None):
    """the loop of stream.cpp:886-938 -> (per level, per box: strm or None), per level per box errFlag"""
    plo, phi = levels[0].prob_lo, levels[0].prob_hi
    out, flags = [], []
    for l, lv in enumerate(levels):
        dx = level_dx(lv)
        S = states[l]
        per, fl = [], []
        for b in range(lv.nboxes):
            ids = ins[l][b]
            if len(ids) == 0:
                per.append(None)
                fl.append(0)
                continue
            T = Fab(S.fab(b), lv.boxes[b, :3] - S.ng)
            G = None if vcomp is None else T
            st, e = vtrace(T, S.ncomp, nodes, ids, G, None if vcomp is None else (vcomp, vcomp + 1, vcomp + 2), nRKsteps, dx, plo, phi, hRK)
            per.append(st)
            fl.append(e)
        out.append(per)
        flags.append(fl)
    return out, flags


# ------------------------------------------------------------------------------------------------ writers
def _g17(v):
    return "%.17g" % v


def _box_str(lo, hi):
    return "((%d,%d,%d) (%d,%d,%d) (0,0,0))" % (lo[0], lo[1], lo[2], hi[0], hi[1], hi[2])


def str_fabs(lines, nRKsteps: int, ncs: int):
    """the Str FABs of one level (stream.cpp:752-761): (lo, hi, data [ncs][nRKsteps or 1][n]) per box, null box of zeros
    where a box has no seed"""
    nRKh = (nRKsteps - 1) // 2
    out = []
    for st in lines:
        if st is None:
            out.append(((0, 0, 0), (0, 0, 0), np.zeros((ncs, 1, 1))))
        else:
            n = st.shape[2]
            out.append(((0, -nRKh, 0), (n - 1, nRKsteps - 1 - nRKh, 0), st))
    return out


def vismf_bytes(fabs, fname="Str_D_00000"):
    """VisMF::Write of a ghost-free multifab, one data file: (header text, data bytes) -- the same layout the plotfile writer
    uses for Cell_H / Cell_D_00000"""
    data = bytearray()
    offs = []
    ncomp = fabs[0][2].shape[0] if fabs else 0
    for lo, hi, a in fabs:
        offs.append(len(data))
        data += ("FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))" + _box_str(lo, hi) + " %d\n" % ncomp).encode()
        data += np.ascontiguousarray(a, dtype="<f8").tobytes()
    nb = len(fabs)
    h = "1\n1\n%d\n0\n(%d 0\n" % (ncomp, nb)
    h += "".join(_box_str(lo, hi) + "\n" for lo, hi, _ in fabs)
    h += ")\n%d\n" % nb
    h += "".join("FabOnDisk: %s %d\n" % (fname, o) for o in offs)
    h += "\n%d,%d\n" % (nb, ncomp)
    h += "".join("".join(_g17(a[c].min()) + "," for c in range(ncomp)) + "\n" for _, _, a in fabs)
    h += "\n%d,%d\n" % (nb, ncomp)
    h += "".join("".join(_g17(a[c].max()) + "," for c in range(ncomp)) + "\n" for _, _, a in fabs)
    return h.encode(), bytes(data)


def stream_file_bytes(names, face, nElts, ins, lines, nRKsteps):
    """write_ml_streamline_data (stream.cpp:2091-2226, OLDFORMAT) -> {relative path: bytes}"""
    files = {}
    h = "Oddball-multilevel-connected-data-format\n%d\n%d\n" % (len(lines), len(names)) + "".join(n + "\n" for n in names)
    files["Header"] = h.encode()
    npe = len(face) // nElts
    e = "%d\n%d\n" % (nElts, npe) + "".join("%d " % v for v in face) + "\n"
    for per in ins:
        e += "%d\n" % sum(1 for ids in per if len(ids) > 0)
        for j, ids in enumerate(per):
            if len(ids) > 0:
                e += "%d %d" % (j, len(ids)) + "".join(" %d" % v for v in ids) + "\n"
    files["Elements"] = e.encode()
    for l, per in enumerate(lines):
        hb, db = vismf_bytes(str_fabs(per, nRKsteps, len(names)))
        files["Level_%d/Str_H" % l] = hb
        files["Level_%d/Str_D_00000" % l] = db
    return files


def out_file_bytes(names, lines, nRKsteps):
    """dump_ml_streamline_data (stream.cpp:2228-2302), one process -> bytes of str_00000.dat, or None when no box is non-null"""
    fabs = [f for per in lines for f in str_fabs(per, nRKsteps, len(names))]
    live = [f for f in fabs if not (tuple(f[0]) == (0, 0, 0) and tuple(f[1]) == (0, 0, 0))]
    if not live:
        return None
    s = ["VARIABLES = " + "".join(n + " " for n in names) + "\n"]
    for lo, hi, a in live:
        for i in range(a.shape[2]):
            s.append("ZONE I=1 J=%d k=1 FORMAT=POINT\n" % a.shape[1])
            for L in range(a.shape[1]):
                s.append("".join("%g " % v for v in a[:, L, i]) + "\n")
    return "".join(s).encode()


# ------------------------------------------------------------------------------------------------ the tool
def run_tool(levels, raw, nodes, names, face, nElts, *, nRKsteps=51, hRK=0.1, vcomp=None, eps_dx=None, bounds=None):
    """stream.cpp main for one process, after the plotfile and seeds are read: push, trim, membership, state, trace.
    raw: per-level MultiFab of the input components (nGrow = the tool's nGrow); hRK before scaling; eps_dx: the file's dx of
    the finest level (push_nodes_inside).  -> dict(nodes, face, nElts, ins, lines, flags, states)"""
    nodes = np.array(nodes, dtype=np.float64)
    fin = levels[-1]
    push_nodes_inside(nodes, fin.prob_lo, fin.prob_hi, EPS_PUSH * (eps_dx if eps_dx is not None else level_dx(fin)[0]))
    face = np.asarray(face, dtype=np.int32)
    npe = len(face) // nElts
    if bounds is not None:
        nodes, face = trim_surface(bounds[:3], bounds[3:], nodes, face, npe)
        nElts = len(face) // npe
    h = hRK * (fin.prob_hi[0] - fin.prob_lo[0]) / (fin.domhi[0] - fin.domlo[0] + 1)
    ins = inside_nodes(levels, nodes)
    states = prepare_states(levels, raw)
    lines, flags = trace_hierarchy(levels, states, nodes, ins, nRKsteps, h, vcomp)
    return dict(nodes=nodes, face=face, nElts=nElts, ins=ins, lines=lines, flags=flags, states=states, hRK=h)
