"""The case matrix of the composite smoothing solve (do_smooth, curvature.cpp:328-406), shared by the CPU tier
(tests/test_oracle_smooth.py: the oracle's operator against the PDE) and the GPU tier (tests/test_gpu_smooth.py: pa_smooth_solve
against the oracle).  What nested_hierarchy never shows the one-rank operator: L-shaped refined regions, concave coarse-fine
corners, fine boxes on a wall and through a periodic face, faces that are partly fine-fine and partly coarse-fine, dx that differs
by direction, 4-cell-wide and 2-cell-thin fine boxes, a fourth level."""
import numpy as np

from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, _occupancy, chop_box, fill_analytic, nested_hierarchy, union_hierarchy


def _level(boxes, domhi, per, prob_hi):
    return Level(np.asarray(boxes, dtype=np.int32), (0, 0, 0), domhi, np.asarray(per), np.zeros(3), np.asarray(prob_hi, float))


def assert_aligned(H):
    """every fine box starts on an even index and has an even width in each refined direction (pa_smooth_solve's contract)"""
    for lv in H.levels[1:]:
        nd = 2 if lv.domlo[2] == lv.domhi[2] else 3
        assert np.all(lv.boxes[:, :nd] % 2 == 0) and np.all(lv.boxes[:, 3:3 + nd] % 2 == 1), lv.boxes
    return H


def hand(per):
    """3 levels, ratio 2, 16 x 20 x 16 cells on [0,1] x [0,1.25] x [0,1] (a non-cubic domain; dx is 1/16 in every direction -- the
    unions below have dx = 1/16, 1/20, 1/16).  Level 1 is L-shaped with concave edges and fine boxes on both x faces
    (neighbours through the periodic face when per[0]); the high-x face of its first box is partly fine-fine, partly coarse-fine.
    Level 2 has a 4-cell-wide and a 2-cell-thin box and another concave corner."""
    ph = (1.0, 1.25, 1.0)
    l0 = _level(chop_box((0, 0, 0), (15, 19, 15), 8), (15, 19, 15), per, ph)
    l1 = _level([[0, 8, 8, 15, 23, 23], [16, 8, 8, 23, 15, 23], [0, 24, 8, 7, 31, 23], [24, 8, 8, 31, 15, 15]], (31, 39, 31), per, ph)
    l2 = _level([[4, 20, 20, 19, 35, 35], [20, 20, 20, 23, 27, 35], [4, 36, 20, 11, 37, 35]], (63, 79, 63), per, ph)
    return assert_aligned(Hierarchy([l0, l1, l2], 2))


UNION_PER = {4: (0, 0, 0), 9: (1, 1, 0), 14: (1, 0, 1)}


def union(seed, per=None):
    """random unions of rectangles (seeds 4, 9, 14: three levels, a fine level on a domain face; seed 9: 4-wide boxes on level 2);
    16 x 20 x 16 cells on the unit cube, so dx differs by direction"""
    H = union_hierarchy(seed, nlev=3, n0=(16, 20, 16), is_per=UNION_PER[seed] if per is None else per)
    assert H.nlev == 3
    assert any(np.any(lv.boxes[:, :3] == 0) or np.any(lv.boxes[:, 3:] == lv.domhi) for lv in H.levels[1:]), "no fine box on a domain face"
    return assert_aligned(H)


def nested4(per=(0, 1, 0)):
    return nested_hierarchy(16, 4, 8, is_per=per)


def planar_L(per):
    """the 2-D build (one plane of cells per level): an L-shaped level 1 on the low-x wall with a concave corner, dx = 1/32, 1/32"""
    per3 = (per[0], per[1], 0)
    ph = (1.0, 0.75, 1.0)
    l0 = _level(chop_box((0, 0, 0), (31, 23, 0), 16), (31, 23, 0), per3, ph)
    l1 = _level([[0, 16, 0, 31, 31, 0], [32, 16, 0, 47, 23, 0], [0, 32, 0, 15, 47, 0]], (63, 47, 0), per3, ph)
    return assert_aligned(Hierarchy([l0, l1], 2))


def march_shapes():
    """one level of 132 x 22 x 66 cells, periodic in x, in 12 boxes: x widths 33, 65, 2, 32 (one past the narrow / wide switch of
    the marching kernels at 32, one past a full 64-lane tile, thinner than any other box, the two-rows-per-wavefront form) times row
    counts 9, 2, 11 (the last tile of rows partly outside the box for 4 and for 8 rows per tile), 66 planes (a chunk of 64 and 2)"""
    boxes = [[x0, y0, 0, x1, y1, 65] for (y0, y1) in ((0, 8), (9, 10), (11, 21)) for (x0, x1) in ((0, 32), (33, 97), (98, 99), (100, 131))]
    return Hierarchy([_level(boxes, (131, 21, 65), (1, 0, 0), (2.0, 1.0 / 3.0, 1.0))], 2)


def is_planar(H):
    return int(H.levels[0].domlo[2]) == int(H.levels[0].domhi[2])


def refine(H):
    """the same hierarchy with every box and domain index doubled (z left alone on a one-plane hierarchy)"""
    nd = 2 if is_planar(H) else 3
    out = []
    for lv in H.levels:
        b = lv.boxes.astype(np.int64).copy()
        b[:, :nd] *= 2
        b[:, 3:3 + nd] = 2 * b[:, 3:3 + nd] + 1
        dh = lv.domhi.astype(np.int64).copy()
        dh[:nd] = 2 * dh[:nd] + 1
        dl = lv.domlo.astype(np.int64).copy()
        dl[:nd] *= 2
        out.append(Level(b, dl, dh, lv.is_per.copy(), lv.prob_lo.copy(), lv.prob_hi.copy()))
    return Hierarchy(out, H.ref_ratio)


def manufactured(H, per, dt):
    """(phi, rhs): functions of (x, y, z); phi = 0.5 + 0.3 prod_d cos(pi k_d x_d / L_d) solves (I - dt Lap) phi = rhs exactly under
    Neumann walls and under periodicity (k even), rhs = 0.5 + (1 + dt lam)(phi - 0.5), lam = pi^2 sum (k_d / L_d)^2"""
    lv = H.levels[0]
    L = lv.prob_hi - lv.prob_lo
    lo = lv.prob_lo
    k = np.array([2.0, 2.0, 2.0]) if any(per) else np.array([1.0, 2.0, 1.0])
    if is_planar(H):
        k[2] = 0.0
    lam = float(np.pi ** 2 * ((k / L) ** 2).sum())

    def phi(x, y, z):
        return 0.5 + 0.3 * np.cos(np.pi * k[0] * (x - lo[0]) / L[0]) * np.cos(np.pi * k[1] * (y - lo[1]) / L[1]) * np.cos(np.pi * k[2] * (z - lo[2]) / L[2])

    def rhs(x, y, z):
        return 0.5 + (1.0 + dt * lam) * (phi(x, y, z) - 0.5)
    return phi, rhs


def finest_dx2(H):
    """dx^2 of the finest level (the largest 1 / dx^2 over the refined directions: what pa_smooth_solve compares dt with)"""
    lv = H.levels[-1]
    nd = 2 if is_planar(H) else 3
    return float((lv.dx[:nd] ** 2).min())


HAND_PER = [(0, 0, 0), (1, 1, 0), (1, 0, 1)]
UNION_SEEDS = [4, 9, 14]
PLANAR_PER = [(0, 0), (1, 0), (0, 1)]

# name -> (builder, periodic flags as given to `manufactured`)
CASES = {}
for _p in HAND_PER:
    CASES["hand-%d%d%d" % _p] = ((lambda p=_p: hand(p)), _p)
for _s in UNION_SEEDS:
    CASES["union%d" % _s] = ((lambda s=_s: union(s)), UNION_PER[_s])
CASES["nested4"] = (nested4, (0, 1, 0))
for _p in PLANAR_PER:
    CASES["planar_L-%d%d" % _p] = ((lambda p=_p: planar_L(p)), _p)


def build(name):
    """-> (Hierarchy, per as `manufactured` takes it, bc flags (3) for bc_from_flags)"""
    fn, per = CASES[name]
    H = fn()
    return H, per, tuple(int(v) for v in H.levels[0].is_per)


# ---------------------------------------------------------------- fields and whole-domain views (both tiers)
def fill(H, fn, ng=0):
    out = []
    for lv in H.levels:
        m = MultiFab(lv, 1, ng)
        fill_analytic(m, 0, fn)
        out.append(m)
    return out


def with_ghosts(H, mfs):
    """copies of 1-comp multifabs as ng-1 multifabs (what the oracle's smooth_apply takes; it overwrites ghosts and covered cells)"""
    out = []
    for lv, m in zip(H.levels, mfs):
        x = MultiFab(lv, 1, 1)
        for b in range(lv.nboxes):
            x.valid(b)[0] = m.valid(b)[0]
        out.append(x)
    return out


def dense(lv, mf):
    """component 0 of mf over the level's whole domain, [nz, ny, nx]; NaN where the level has no cell"""
    n = lv.domhi - lv.domlo + 1
    a = np.full((int(n[2]), int(n[1]), int(n[0])), np.nan)
    for b in range(lv.nboxes):
        lo, hi = lv.boxes[b, :3] - lv.domlo, lv.boxes[b, 3:] - lv.domlo
        a[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = mf.valid(b)[0]
    return a


def uncovered(H):
    """per level, bool[nz, ny, nx] over the domain: cells of the level that no finer level covers"""
    occ = [_occupancy(lv) for lv in H.levels]
    rz = 1 if is_planar(H) else 2
    out = []
    for l, o in enumerate(occ):
        u = o.copy()
        if l + 1 < len(occ):
            f = occ[l + 1]
            u &= ~f[::rz, ::2, ::2]  # aligned boxes: a coarse cell is covered entirely or not at all
        out.append(u)
    return out


def max_uncovered(H, a_mfs, b_mfs=None, fn=None):
    """max |a - b| (b: multifabs, or a function of the cell centre) over the uncovered cells of the hierarchy"""
    unc = uncovered(H)
    worst = 0.0
    for l, lv in enumerate(H.levels):
        a = dense(lv, a_mfs[l])
        if fn is not None:
            ref = MultiFab(lv, 1, 0)
            fill_analytic(ref, 0, fn)
            b = dense(lv, ref)
        else:
            b = dense(lv, b_mfs[l])
        worst = max(worst, float(np.abs(a - b)[unc[l]].max()))
    return worst
