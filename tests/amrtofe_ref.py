"""Plain-Python restatement of PeleAnalysis Src/amrToFE.cpp (3-D, nGrowPer = 0), written from the reference's text.

The data structures are the reference's: one NodeFab per grid of every level on the box grown by one cell (here: numpy
arrays of the node's type, level and IntVect over that box), a dict for std::map<Node,int> and a set of 8-tuples for
std::set<Element>.  A node is the tuple (level, k, j, i): Node::operator< (:25-30) compares the level and then the
IntVect, whose operator< has z most significant and x least, so Python's tuple order IS the reference's order, and an
element -- a tuple of eight such tuples -- sorts as Element::operator< (:68-74) does.

Where the reference prints and carries on with misnumbered connectivity ("Node not found in node map", :615-619) or
writes outside a FAB (:499-507, a fine box that is not aligned to its ratio) the restatement raises FeError, as the tool
aborts.  Both writers (:854-879 tec, :884-896 flt) return bytes."""
import numpy as np

INIT, COVERED, VALID = 0, 1, 2


class FeError(RuntimeError):
    pass


def _isect(a, b):
    lo = np.maximum(a[:3], b[:3])
    hi = np.minimum(a[3:], b[3:])
    return None if np.any(lo > hi) else np.concatenate([lo, hi]).astype(np.int64)


def _refine(b, r):
    return np.concatenate([b[:3] * r, (b[3:] + 1) * r - 1]).astype(np.int64)


def _coarsen(b, r):
    return np.concatenate([b[:3] // r, b[3:] // r]).astype(np.int64)  # floor division, as amrex::coarsen


def _grow(b, n):
    return np.concatenate([b[:3] - n, b[3:] + n]).astype(np.int64)


def grids(levels, ratios, subbox=None, finest_level=None):
    """:374-452 -> (subboxArray, gridArray); gridArray[lev] = [(index of the box in the file, box & subbox), ...]"""
    dom0 = np.concatenate([levels[0].domlo, levels[0].domhi]).astype(np.int64)
    sub = dom0 if subbox is None else _isect(np.asarray(subbox, dtype=np.int64), dom0)
    if sub is None:
        raise FeError("the box does not intersect the domain")
    nlev = len(levels) if finest_level is None else finest_level + 1
    subs, grid = [], []
    for lev in range(nlev):
        s = sub if lev == 0 else _refine(subs[lev - 1], int(ratios[lev - 1]))
        g = []
        for fb, b in enumerate(levels[lev].boxes.astype(np.int64)):
            x = _isect(b, s)
            if x is not None:
                g.append((fb, x))
        if not g:  # :445-451
            break
        subs.append(s)
        grid.append(g)
    return subs, grid


def _occupancy(boxes, frame):
    """bool[nz, ny, nx] over `frame`: cells that lie in one of the boxes"""
    n = frame[3:] - frame[:3] + 1
    occ = np.zeros((n[2], n[1], n[0]), dtype=bool)
    for b in boxes:
        x = _isect(b, frame)
        if x is not None:
            l, h = x[:3] - frame[:3], x[3:] - frame[:3]
            occ[l[2]:h[2] + 1, l[1]:h[1] + 1, l[0]:h[0] + 1] = True
    return occ


def _in_box(K, J, I, b):
    return (I >= b[0]) & (I <= b[3]) & (J >= b[1]) & (J <= b[4]) & (K >= b[2]) & (K <= b[5])


class FeMeshRef:
    """nodes: [(level, i, j, k, file box)] in id order; elements: the sorted list of 8-tuples of (level, k, j, i);
    conn: int32 [nElts][8], 1-based (:603-633)"""

    def __init__(self, levels, ratios, subbox=None, finest_level=None, connect_cc=True):
        self.levels, self.ratios, self.connect_cc = levels, [int(r) for r in ratios], bool(connect_cc)
        self.subs, self.grid = grids(levels, ratios, subbox, finest_level)
        self.nlev = len(self.grid)
        finest = self.nlev - 1
        for lev in range(1, self.nlev):
            r = self.ratios[lev - 1]
            b = levels[lev].boxes.astype(np.int64)
            if np.any(b[:, :3] % r) or np.any((b[:, 3:] + 1) % r):
                raise FeError("a fine box is not aligned to its refinement ratio")
        node_map, fabs = {}, []
        self.nodes = []
        for lev in range(self.nlev):
            sub, g = self.subs[lev], self.grid[lev]
            frame = _grow(np.concatenate([np.min([v[:3] for _, v in g], axis=0), np.max([v[3:] for _, v in g], axis=0)]), 1)
            occ = _occupancy([v for _, v in g], frame)
            cov = None
            if lev < finest:  # :523-540
                cov = _occupancy([_coarsen(v, self.ratios[lev]) for _, v in self.grid[lev + 1]], frame)
            lev_fabs = []
            for fb, valid in g:
                G = _grow(valid, 1)
                K, J, I = np.meshgrid(np.arange(G[2], G[5] + 1), np.arange(G[1], G[4] + 1), np.arange(G[0], G[3] + 1), indexing="ij")
                typ = np.full(K.shape, INIT)
                nl = np.full(K.shape, -1)
                nk, nj, ni = K.copy(), J.copy(), I.copy()
                insub = _in_box(K, J, I, sub)
                typ[insub] = VALID  # :469-475
                nl[insub] = lev
                sl = tuple(slice(G[2 - d] - frame[2 - d], G[5 - d] - frame[2 - d] + 1) for d in range(3))
                if lev != 0:  # :477-520: the cells of grow(valid, ref) & subbox that belong to no grid of the level, inside this FAB
                    r = self.ratios[lev - 1]
                    m = insub & ~occ[sl] & _in_box(K, J, I, _grow(valid, r))
                    nl[m] = lev - 1
                    nk[m], nj[m], ni[m] = K[m] // r, J[m] // r, I[m] // r
                if cov is not None:
                    c = cov[sl]
                    typ[c] = COVERED
                    nl[c] = lev
                    nk[c], nj[c], ni[c] = K[c], J[c], I[c]
                lev_fabs.append((G, typ, nl, nk, nj, ni))
                # :543-556: ids in the order of the cells of valid & subbox (x fastest)
                v = tuple(slice(1, -1) for _ in range(3))
                for k, j, i, t, l in zip(K[v].ravel(), J[v].ravel(), I[v].ravel(), typ[v].ravel(), nl[v].ravel()):
                    if t == VALID:
                        assert l == lev, "bad level"
                        node_map[(lev, int(k), int(j), int(i))] = len(self.nodes)
                        self.nodes.append((lev, int(i), int(j), int(k), fb))
            fabs.append(lev_fabs)
        elements = set()  # :561-601
        for lev in range(self.nlev):
            for G, typ, nl, nk, nj, ni in fabs[lev]:
                box = _isect(G, self.subs[lev])
                box[3:] -= 1
                if np.any(box[:3] > box[3:]):
                    continue
                l, h = box[:3] - G[:3], box[3:] - G[:3]
                corner = []
                ok = None
                for dz, dy, dx in ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0)):  # :585-592
                    s = (slice(l[2] + dz, h[2] + dz + 1), slice(l[1] + dy, h[1] + dy + 1), slice(l[0] + dx, h[0] + dx + 1))
                    corner.append(np.stack([nl[s], nk[s], nj[s], ni[s]], axis=-1))
                    ok = (typ[s] == VALID) if ok is None else ok & (typ[s] == VALID)
                C = np.stack(corner, axis=-2)[ok]  # [kept cubes][8][4]
                for e in C.tolist():
                    elements.add(tuple(tuple(n) for n in e))
        self.elements = sorted(elements)
        self.nnodes = len(self.nodes)
        if self.connect_cc:
            conn = np.zeros((len(self.elements), 8), dtype=np.int32)
            for q, e in enumerate(self.elements):
                for j, n in enumerate(e):
                    if n not in node_map:
                        raise FeError("Node not found in node map")
                    conn[q, j] = node_map[n] + 1
            self.nelts, self.nnodes_final = len(self.elements), self.nnodes
        else:  # :626-633
            self.nelts, self.nnodes_final = self.nnodes, 8 * self.nnodes
            conn = np.arange(1, 8 * self.nelts + 1, dtype=np.int32).reshape(-1, 8)
        self.conn = conn

    def node_data(self, mfs, comps):
        """:711-814 -> float64 [3 + len(comps)][nNodesFINAL], block ordering.  mfs: MultiFab per level on the file's boxes"""
        L0 = self.levels[0]
        plo = L0.prob_lo
        size = L0.prob_hi - L0.prob_lo
        dxl = [size / (lv.domhi - lv.domlo + 1).astype(np.float64) for lv in self.levels]  # :718-724
        out = np.zeros((3 + len(comps), self.nnodes_final))
        cnt = 0
        for lev, i, j, k, fb in self.nodes:
            iv = np.array([i, j, k])
            if self.connect_cc:
                ivt, offset = [iv], 0.5
            else:  # :779-787: the block under #if BLSPACEDIM==3 is never compiled, the upper corners stay at iv
                ivt, offset = [iv.copy() for _ in range(8)], 0.0
                ivt[1][0] += 1
                ivt[2] = ivt[1].copy()
                ivt[2][1] += 1
                ivt[3][1] += 1
            lo = self.levels[lev].boxes[fb, :3]
            vals = [mfs[lev].valid(fb)[c, k - lo[2], j - lo[1], i - lo[0]] for c in comps]
            for t in ivt:
                for d in range(3):
                    out[d, cnt] = plo[d] + (t[d] + offset) * dxl[lev][d]
                for n, v in enumerate(vals):
                    out[3 + n, cnt] = v
                cnt += 1
        return out

    def bad_data(self, mfs, comps):
        """:702-707: a value above 1e29 in the first selected component on the grids of some level"""
        for lev in range(self.nlev):
            for fb, v in self.grid[lev]:
                lo = self.levels[lev].boxes[fb, :3]
                a = mfs[lev].valid(fb)[comps[0], v[2] - lo[2]:v[5] - lo[2] + 1, v[1] - lo[1]:v[4] - lo[1] + 1, v[0] - lo[0]:v[3] - lo[0] + 1]
                if np.any(a > 1.0e29):
                    return True
        return False


def _g(v):
    """a double through operator<< of a default stream: 6 significant digits"""
    return "%g" % v


def write_tec(infile, time, names, data, conn):
    """:854-879"""
    out = ['VARIABLES= "X" "Y" "Z"' + "".join(' "%s"' % n for n in names) + "\n"]
    out.append('ZONE T="%s time = %s", N=%d, E=%d, F=FEPOINT ET=BRICK\n' % (infile, "%g" % time, data.shape[1], len(conn)))
    for i in range(data.shape[1]):
        out.append("".join(_g(v) + " " for v in data[:, i]) + "\n")
    for e in conn:
        out.append("".join("%d " % v for v in e) + "\n")
    out.append("\n")
    return "".join(out).encode()


def write_flt(infile, time, names, data, conn):
    """:884-896; FArrayBox::writeOn of the (0..N-1, 0, 0) x nComp block array, then the raw int connectivity"""
    n, nc = data.shape[1], data.shape[0]
    head = "%s time = %s\n%s\n%d 8\n" % (infile, _g(time), " ".join(["X", "Y", "Z"] + list(names)), len(conn))
    fab = "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))((0,0,0) (%d,0,0) (0,0,0)) %d\n" % (n - 1, nc)
    return head.encode() + fab.encode() + np.ascontiguousarray(data, dtype="<f8").tobytes() + np.ascontiguousarray(conn, dtype="<i4").tobytes()
