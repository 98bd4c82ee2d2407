"""The case matrix of the ghost-fill tests, shared by the CPU tier (test_ghost_ref.py: reference against oracle) and the GPU tier
(test_gpu_ghost.py: kernels against reference).  Every geometry is at most 32 cells a side per level's boxes, level 0 covers the
domain, every case is properly nested.  A case names the branch of the kernels it was written for and `expect`s facts that
`facts()` computes from the geometry alone (and from the reference's class maps), so that a later edit of a geometry that no
longer reaches its branch fails on the CPU."""
import dataclasses
import functools
import math

import numpy as np

import ghost_ref as GR
from peleanalysis_amd.hierarchy import Level, MultiFab, chop_box, mf_layout, nested_hierarchy

PA_MAXB = 4


def _lv(boxes, domlo, domhi, per):
    domlo, domhi = np.asarray(domlo), np.asarray(domhi)
    return Level(np.asarray(boxes, dtype=np.int32).reshape(-1, 6), domlo, domhi, per, np.zeros(3), np.ones(3))


def _dom(lo, n, per, box=None):
    """level 0: the whole domain, chopped"""
    lo = np.asarray(lo)
    hi = lo + np.asarray(n) - 1
    return _lv(chop_box(lo, hi, box or 32), lo, hi, per)


def _fine(crse: Level, boxes, r=2):
    return _lv(boxes, crse.domlo * r, (crse.domhi + 1) * r - 1, crse.is_per)


@dataclasses.dataclass
class FillCase:
    name: str
    levels: list
    branch: str            # what the case was written for
    expect: dict           # facts that must hold (facts())
    ratio: int = 2
    alloc: int = 4         # ghost width of the multifabs
    ngs: tuple = None      # ng argument per level (default: alloc)
    nc: int = 1            # components of the multifabs
    comp: int = 0
    ncomp: int = 1
    interp: int = 1
    foextrap: int = 1
    seed: int = 1
    two_slopes: bool = False  # a coarse periodic length of 2: the lower and upper neighbour are one cell, that direction's slope is always 0

    def __post_init__(self):
        if self.ngs is None:
            self.ngs = (self.alloc,) * len(self.levels)
        assert len(self.ngs) == len(self.levels) and max(self.ngs) <= self.alloc

    @property
    def nlev(self):
        return len(self.levels)

    @property
    def comps(self):
        return list(range(self.comp, self.comp + self.ncomp))


# ----------------------------------------------------------------------------- geometries
def geo_a():  # one box = a fully periodic domain: the box fills its ghost cells from its own 26 images
    return [_dom((0, 0, 0), (6, 5, 4), (1, 1, 1))]


def geo_b():  # fine level 8 cells wide in periodic x, boxes 3 and 5 wide, odd corners in y: with ng 4 a shell passes the neighbour and enters its own image
    c = _dom((0, 0, 0), (4, 8, 8), (1, 0, 0))
    return [c, _fine(c, [[0, 5, 0, 2, 12, 7], [3, 5, 0, 7, 12, 7]])]


def geo_c(split):  # fine level 4 cells wide in periodic x = coarse length 2: a parent's neighbours lie two periods out
    c = _dom((0, 0, 0), (2, 8, 8), (1, 0, 0))
    boxes = [[0, 4, 0, 0, 11, 7], [1, 4, 0, 3, 11, 7]] if split else [[0, 4, 0, 3, 11, 7]]
    return [c, _fine(c, boxes)]


def geo_d():  # everything even, walls on every side, fine boxes in a wall corner
    c = _dom((0, 0, 0), (8, 8, 8), (0, 0, 0))
    return [c, _fine(c, [[0, 0, 0, 7, 7, 7], [8, 0, 0, 15, 7, 7]])]


def geo_e():  # the domain starts at (-3, -1, 1): negative, odd cell indices
    c = _dom((-3, -1, 1), (8, 8, 8), (0, 0, 0))
    return [c, _fine(c, [[-5, -1, 3, 1, 4, 7], [2, -1, 3, 6, 4, 7]])]


def geo_f():  # L-shaped fine region (concave corner at x = y = 4) in the wall corner y = z = 0; one arm on the periodic face x = 0, whose image is coarse
    c = _dom((0, 0, 0), (8, 8, 8), (1, 0, 0))
    return [c, _fine(c, [[0, 0, 0, 3, 7, 7], [4, 0, 0, 11, 3, 7]])]


def geo_g():  # refinement ratio 4, negative origin, periodic y
    c = _dom((-3, -1, 1), (8, 8, 8), (0, 1, 0))
    return [c, _fine(c, [[-8, 0, 4, -1, 7, 11], [0, 0, 4, 5, 7, 11]], 4)]


def geo_h():  # one level, boxes of 15 x 16 x 17 and 16 x 16 x 17 cells side by side: owner grid of single cells, unequal component strides
    return [_lv([[0, 0, 0, 14, 15, 16], [15, 0, 0, 30, 15, 16]], (0, 0, 0), (30, 15, 16), (1, 0, 1))]


def geo_i3(per=(1, 1, 0)):  # three levels for ghost widths 1 / 2 / 4
    l0 = _dom((0, 0, 0), (12, 12, 12), per, 6)
    l1 = _fine(l0, chop_box((4, 4, 4), (19, 19, 19), 8))
    l2 = _fine(l1, chop_box((16, 16, 16), (31, 31, 23), 8))
    return [l0, l1, l2]


def geo_i6():  # six levels: five level pairs, one more than a batched launch takes
    return nested_hierarchy(8, 6, 4, is_per=(1, 1, 0)).levels


def geo_thin():  # boxes thinner than the ghost width, next to each other and to a wall
    c = _dom((0, 0, 0), (8, 8, 8), (0, 1, 0))
    return [c, _fine(c, [[0, 4, 4, 0, 11, 11], [1, 4, 4, 2, 11, 11], [3, 4, 4, 5, 11, 11], [6, 4, 4, 9, 11, 11]])]


@functools.lru_cache(maxsize=None)
def fill_cases():
    C = []
    # a: self-copy through all 26 images; ng up to the period
    for ng in (1, 2, 4):
        C.append(FillCase(f"a_ng{ng}", geo_a(), "FillBoundary of one box from its own 26 periodic images; ng equal to the period (ng 4)", dict(self_images=26, classes={0}),
                          ngs=(ng,), nc=4, comp=1, ncomp=2))
    # b: shell past the neighbour, per-child classification
    for it in (0, 1):
        C.append(FillCase(f"b_interp{it}", geo_b(), "shell past the neighbour into the box's own image; odd box corners: per-child k_fp_find", dict(uniform=[False], classes={0, 1, 2}, own_image=True),
                          interp=it, nc=4, comp=0, ncomp=4))
    C.append(FillCase("b_interp1_ng2", geo_b(), "the same levels with ng 2 after ng 4: the k_fp_find plan is kept per (coarse level, ng), FillBoundary's per ng", dict(uniform=[False], classes={0, 1, 2}),
                      ngs=(2, 2), nc=4, comp=0, ncomp=4))
    # c: double wrap of coarse neighbours
    C.append(FillCase("c_one", geo_c(False), "coarse periodic length 2: neighbours of a parent two periods out (one box)", dict(double_wrap=True, classes={0, 1, 2}), ngs=(2, 4), two_slopes=True))
    C.append(FillCase("c_split", geo_c(True), "the same with boxes 1 and 3 wide; a box thinner than ng", dict(double_wrap=True, thin=True, uniform=[False], classes={0, 1, 2}), ngs=(2, 4), nc=4, comp=3, ncomp=1, two_slopes=True))
    # d: uniform path, foextrap through a coarse-fine ghost
    C.append(FillCase("d_uniform", geo_d(), "`uniform` k_fp_find; foextrap of edge and corner ghosts whose clamped cell is a coarse-fine ghost", dict(uniform=[True], clamped_is_cf=True, classes={0, 1, 2})))
    C.append(FillCase("d_uniform_nofo", geo_d(), "the same without foextrap: cells beyond a wall stay unwritten", dict(uniform=[True], classes={0, 1, 2}), foextrap=0, ngs=(4, 2), nc=4, comp=1, ncomp=2))
    # e: negative indices
    C.append(FillCase("e_negative", geo_e(), "floor division of negative cell indices in coarsen_idx", dict(negative_odd=True, uniform=[False], classes={0, 1, 2}), alloc=3))
    C.append(FillCase("e_negative_pc", geo_e(), "the same, piecewise constant, ng argument below the allocated width", dict(negative_odd=True, classes={0, 1, 2}), alloc=4, ngs=(1, 1), interp=0))
    # f: coarse-fine ghost through a periodic image
    C.append(FillCase("f_lshape", geo_f(), "L-shaped fine region: concave corner, coarse-fine ghosts reached through a periodic image", dict(cf_through_image=True, concave=True, classes={0, 1, 2}), alloc=3))
    # g: ratio 4
    for it in (0, 1):
        C.append(FillCase(f"g_ratio4_interp{it}", geo_g(), "refinement ratio 4: per-cell kernel; floor division at ratio 4", dict(negative_odd=True, classes={0, 1, 2}), ratio=4, alloc=3, interp=it, nc=4, comp=1, ncomp=2))
    # h: O(n^2) candidates, unequal strides
    for comp, ncomp in ((0, 4), (1, 2), (3, 1)):
        C.append(FillCase(f"h_odd_c{comp}n{ncomp}", geo_h(), "owner grid of single cells: O(n^2) candidates in pa_fb_local_plan, region form all the same; boxes of unequal component strides; "
                          f"component range ({comp}, {ncomp}) of 4", dict(grid_cells_gt_4096=True, unequal_strides=True, classes={0, 2}), ngs=(2,), nc=4, comp=comp, ncomp=ncomp))
    # thin boxes
    for ng in (2, 4):
        C.append(FillCase(f"thin_ng{ng}", geo_thin(), "boxes 1, 2, 3 and 4 cells wide: thinner than ng, shells that pass two neighbours", dict(thin=True, classes={0, 1, 2}), ngs=(ng, ng)))
    # i: batches
    C.append(FillCase("i_three_124", geo_i3(), "three levels with ghost widths 1 / 2 / 4: batch kernels with a width per level", dict(classes={0, 1, 2}), ngs=(1, 2, 4), nc=4, comp=1, ncomp=2))
    C.append(FillCase("i_three_124_pc", geo_i3(), "the same, piecewise constant, without foextrap (the isosurface's fill)", dict(classes={0, 1, 2}), ngs=(1, 2, 4), interp=0, foextrap=0))
    C.append(FillCase("i_six", geo_i6(), "six levels: the second PA_MAXB batch of level pairs and of foextrap levels", dict(second_batch=True, classes={0, 1, 2}, windowed=True), alloc=2, ngs=(1, 2, 2, 2, 1, 2)))
    # j: no wall anywhere
    C.append(FillCase("j_periodic", geo_i3((1, 1, 1)), "fully periodic three levels: k_foextrap_levels skips every level", dict(no_wall=True, classes={0, 1}), ngs=(1, 2, 4)))
    names = [c.name for c in C]
    assert len(set(names)) == len(names)
    return C


def fill_case(name):
    return next(c for c in fill_cases() if c.name == name)


# ----------------------------------------------------------------------------- data
def random_mf(level, nc, ng, seed, fill_bits=None):
    """uniform random values times 10**k, k from -3 to 2, both signs, in the valid cells of every component; every other double of
    the multifab (ghost cells, padding) holds fill_bits (a sentinel of util.py) or NaN"""
    rng = np.random.default_rng(seed)
    _, _, total = mf_layout(level.boxes, nc, ng)
    data = np.full(total, np.nan) if fill_bits is None else np.full(total, fill_bits, dtype=np.uint64).view(np.float64)
    mf = MultiFab(level, nc, ng, data=data)
    for b in range(level.nboxes):
        v = mf.valid(b)
        v[...] = rng.uniform(-1.0, 1.0, size=v.shape) * 10.0 ** rng.integers(-3, 3, size=v.shape)
    return mf


@functools.lru_cache(maxsize=None)
def plant_sites(name):
    """per fine level of an interp_type 1 case, one coarse cell (level, (i, j, k)) that is the parent of a compared coarse-fine ghost
    cell and whose 26 neighbours are cells of the same coarse box: where case_data plants a parent with a common factor below 1.
    Independent random values hardly ever give one (the three limited slopes are at most twice the smallest one-sided difference
    each, so all three lower -- or upper -- neighbours must lie close to the parent), and the matrix must see that branch."""
    case = fill_case(name)
    mfs = [random_mf(lv, case.nc, case.alloc, l, None) for l, lv in enumerate(case.levels)]  # any data: the class maps are geometry
    R = GR.dense_levels(case.levels, mfs, [case.comp], case.ratio, 0, [case.alloc] * case.nlev)
    sites = []
    for l in range(1, case.nlev):
        lv, cl = case.levels[l], case.levels[l - 1]
        found = None
        for b in range(lv.nboxes):
            B = GR.box_ref(R[l], b, case.alloc, [case.comp])
            kz, jy, ix = np.nonzero(GR.write_mask(B, "fp", case.ngs[l]))
            q = np.stack([ix, jy, kz], axis=1) + (lv.boxes[b, :3].astype(np.int64) - B.G)
            for p in np.unique(np.floor_divide(q, case.ratio), axis=0):
                inside = ((cl.boxes[:, :3] <= p - 1) & (cl.boxes[:, 3:] >= p + 1)).all(axis=1)
                if inside.any():
                    found = (l - 1, tuple(int(v) for v in p))
                    break
            if found:
                break
        if found:
            sites.append(found)
    return sites


def plant(mf, cell, rng):
    """around the coarse cell (value v kept): the lower face neighbours at v - beta (1, 1.1, 1.2), the other 23 neighbours in
    v + beta [4, 10].  Every limited slope is then twice its lower difference, dumax = beta (2 + 2.2 + 2.4) (r - 1) / (2 r) exceeds
    v - umin = 1.2 beta for r = 2 (1.65 beta) and r = 4 (2.475 beta), and the common factor is 1.2 beta / dumax < 1"""
    p = np.asarray(cell)
    lv = mf.level
    b = int(np.nonzero(((lv.boxes[:, :3] <= p - 1) & (lv.boxes[:, 3:] >= p + 1)).all(axis=1))[0][0])
    o = p - lv.boxes[b, :3]
    for c in range(mf.ncomp):
        a = mf.valid(b)[c]
        v = a[o[2], o[1], o[0]]
        beta = 0.01 * abs(v) + 1e-3
        nb = v + beta * rng.uniform(4.0, 10.0, size=(3, 3, 3))
        nb[1, 1, 1] = v
        nb[1, 1, 0], nb[1, 0, 1], nb[0, 1, 1] = v - beta, v - 1.1 * beta, v - 1.2 * beta
        a[o[2] - 1:o[2] + 2, o[1] - 1:o[1] + 2, o[0] - 1:o[0] + 2] = nb


def case_data(case, fill_bits, seed_shift=0):
    """the multifabs of a case, level 0 first"""
    mfs = [random_mf(lv, case.nc, case.alloc, 1000 * case.seed + 10 * seed_shift + l, fill_bits) for l, lv in enumerate(case.levels)]
    if case.interp == 1:
        rng = np.random.default_rng(77 + seed_shift)
        for l, cell in plant_sites(case.name):
            plant(mfs[l], cell, rng)
    return mfs


@functools.lru_cache(maxsize=None)
def case_ref(name, seed_shift=0):
    """(dense levels, per level the BoxRef of every box) of a case's data"""
    case = fill_case(name)
    mfs = case_data(case, None, seed_shift)
    R = GR.dense_levels(case.levels, mfs, case.comps, case.ratio, case.interp, [case.alloc] * case.nlev)
    return R, [[GR.box_ref(R[l], b, case.alloc, case.comps) for b in range(lv.nboxes)] for l, lv in enumerate(case.levels)]


# ----------------------------------------------------------------------------- facts
def owner_grid(level):
    """(g, mlo): the owner map of pa_level_create -- cells of g^3 from the lowest box corner, g the gcd of box sizes and offsets"""
    mlo = level.boxes[:, :3].min(axis=0).astype(np.int64)
    g = 0
    for b in level.boxes.astype(np.int64):
        for d in range(3):
            g = math.gcd(g, int(b[d] - mlo[d]))
            g = math.gcd(g, int(b[3 + d] - b[d] + 1))
    return max(g, 1), mlo


def uniform_predicate(level):
    """fp_parent_plan: one classification stands for a parent's 8 children"""
    g, mlo = owner_grid(level)
    return bool(g % 2 == 0 and all(int(mlo[d]) % 2 == 0 and int(level.domlo[d]) % 2 == 0 and (int(level.domhi[d]) + 1) % 2 == 0 for d in range(3)))


def facts(case: FillCase) -> dict:
    R, BR = case_ref(case.name)
    F = {}
    F["uniform"] = [uniform_predicate(lv) for lv in case.levels[1:]]
    classes = set()
    for l, brs in enumerate(BR):
        for B in brs:
            classes |= set(int(v) for v in np.unique(B.cls[(B.layer > 0) & (B.layer <= case.ngs[l])]))
    F["classes"] = classes
    F["windowed"] = any(not r.whole for r in R)
    F["second_batch"] = case.nlev - 1 > PA_MAXB
    F["no_wall"] = all(bool(np.all(lv.is_per)) for lv in case.levels)
    F["thin"] = any(int((lv.boxes[:, 3:] - lv.boxes[:, :3] + 1).min()) < case.ngs[l] for l, lv in enumerate(case.levels))
    lv = case.levels[-1]
    n = lv.domhi.astype(np.int64) - lv.domlo + 1
    # a single box that is its whole periodic domain: ghost cells of all 26 directions are its own images
    F["self_images"] = 26 if (lv.nboxes == 1 and np.all(lv.is_per) and np.all(lv.boxes[0, 3:] - lv.boxes[0, :3] + 1 == n)) else 0
    # owner-grid cells under a grown box (pa_fb_local_plan walks at most 4096 of them)
    g, mlo = owner_grid(lv)
    mhi = lv.boxes[:, 3:].max(axis=0).astype(np.int64)
    most = 0
    for b in lv.boxes.astype(np.int64):
        lo, hi = np.maximum(b[:3] - case.ngs[-1], mlo), np.minimum(b[3:] + case.ngs[-1], mhi)
        most = max(most, int(np.prod((hi - mlo) // g - (lo - mlo) // g + 1)))
    F["grid_cells_gt_4096"] = most > 4096
    cs = mf_layout(lv.boxes, case.nc, case.alloc)[1]
    F["unequal_strides"] = bool(case.nc > 1 and len(set(int(c) for c in cs)) > 1)
    # facts about single ghost cells of the finest level
    F["double_wrap"] = F["negative_odd"] = F["cf_through_image"] = F["clamped_is_cf"] = F["own_image"] = F["concave"] = False
    if case.nlev > 1:
        r, ng = case.ratio, case.ngs[-1]
        cl = case.levels[-2]
        cn = cl.domhi.astype(np.int64) - cl.domlo + 1
        for b, B in enumerate(BR[-1]):
            blo = lv.boxes[b, :3].astype(np.int64)
            kz, jy, ix = np.nonzero((B.cls == 1) & (B.layer <= ng))
            q = np.stack([ix, jy, kz], axis=1) + (blo - B.G)  # unwrapped cell indices, x y z
            qc = np.floor_divide(q, r)
            for d in range(3):
                if lv.is_per[d]:
                    F["double_wrap"] |= bool(((qc[:, d] - 1 < cl.domlo[d] - cn[d]) | (qc[:, d] + 1 > cl.domhi[d] + cn[d])).any())
                    F["cf_through_image"] |= bool(((q[:, d] < lv.domlo[d]) | (q[:, d] > lv.domhi[d])).any())
                F["negative_odd"] |= bool(((q[:, d] < 0) & (q[:, d] % r != 0)).any())
            m2 = (B.cls == 2) & (B.layer <= ng)
            F["clamped_is_cf"] |= bool((B.cls[np.ix_(*B.clamp)][m2] == 1).any())
            # a class-1 ghost cell with covered neighbours in two directions: the concave corner of an L
            c1 = (B.cls == 1)
            cov = (B.cls <= 0)  # a valid cell of the box or of a neighbour
            F["concave"] |= bool((c1[1:-1, 1:-1, 1:-1] & ((cov[1:-1, 1:-1, :-2] | cov[1:-1, 1:-1, 2:]) & (cov[1:-1, :-2, 1:-1] | cov[1:-1, 2:, 1:-1]))).any())
    for b, B in enumerate(BR[-1]):
        # a class-0 ghost cell that is an image of a valid cell of its own box
        blo, bhi = lv.boxes[b, :3].astype(np.int64), lv.boxes[b, 3:].astype(np.int64)
        kz, jy, ix = np.nonzero((B.cls == 0) & (B.layer <= case.ngs[-1]))
        q = np.stack([ix, jy, kz], axis=1) + (blo - B.G)
        w = (q - lv.domlo) % n + lv.domlo
        F["own_image"] |= bool(((w >= blo) & (w <= bhi)).all(axis=1).any())
    return F


def check_expect(case: FillCase):
    F = facts(case)
    for k, v in case.expect.items():
        assert F[k] == v, f"case {case.name} ({case.branch}): fact {k} is {F[k]}, the case needs {v}"


# ----------------------------------------------------------------------------- applyBC
@dataclasses.dataclass
class BcCase:
    name: str
    levels: list
    bc: tuple              # per direction 0 periodic / 1 Neumann / 2 reflect-odd
    branch: str
    alloc: int = 1
    nc: int = 3
    comp: int = 2
    ccomp: int = 0
    only_dir: int = -1
    no_coarse: bool = False
    seed: int = 7
    ratio: int = 2


def _split(lo, t):
    """a block of 4 cells from lo cut into slabs t and 4 - t thick (what a re-tiling leaves: the union stays aligned to the coarse cells)"""
    return [(lo, lo + 3)] if t == 4 else [(lo, lo + t - 1), (lo + t, lo + 3)]


def _bc_levels(per, thick):
    """a 12^3 coarse domain.  Fine level: one block of 4 cells per direction cut into slabs `thick` and 4 - thick cells thick along it --
    in x on the low faces of the domain with faces of 18 x 16 cells (more than one chunk of 256), in y on the domain's high y face, in z
    in the interior -- and a box that covers part of the first block's high x face"""
    c = _dom((0, 0, 0), (12, 12, 12), per, 6)
    boxes = [[a, 0, 0, b, 17, 15] for a, b in _split(0, thick)]
    boxes += [[4, 0, 0, 7, 7, 7]]
    boxes += [[8, a, 16, 11, b, 23] for a, b in _split(20, thick)]
    boxes += [[14, 8, a, 21, 13, b] for a, b in _split(8, thick)]
    return [c, _fine(c, boxes)]


@functools.lru_cache(maxsize=None)
def bc_cases():
    C = []
    kinds = {"nnn": ((0, 0, 0), (1, 1, 1)), "rpn": ((0, 1, 0), (2, 0, 1)), "pnr": ((1, 0, 0), (0, 1, 2)), "nrp": ((0, 0, 1), (1, 2, 0))}
    # thickness 1 needs two allocated layers wherever a kernel that took the full-order stencil by mistake would read (kept inside the FAB)
    for t, alloc in ((1, 2), (2, 1), (3, 2), (4, 1)):
        for kn in ("nnn", "rpn") if t in (1, 4) else ("pnr", "nrp"):
            per, bc = kinds[kn]
            C.append(BcCase(f"t{t}_{kn}_ng{alloc}", _bc_levels(per, t), bc, f"boxes {t} thick along the face normal (NX = {min(t + 1, 4)}); bc {bc}; faces above and below 256 cells", alloc=alloc))
    for od in (0, 1, 2):
        per, bc = kinds["rpn" if od != 1 else "nrp"]
        C.append(BcCase(f"only_dir{od}", _bc_levels(per, 2), bc, f"only_dir = {od}: the faces of the other directions stay", alloc=2, only_dir=od))
    per, bc = kinds["nnn"]
    C.append(BcCase("no_coarse", _bc_levels(per, 3), bc, "a level > 0 without a coarse multifab: coarse-fine face ghosts are counted, not written", alloc=2, no_coarse=True))
    return C


def bc_case(name):
    return next(c for c in bc_cases() if c.name == name)


def bc_data(case, fill_bits):
    return [random_mf(lv, case.nc, case.alloc, 100 * case.seed + l, fill_bits) for l, lv in enumerate(case.levels)]


@functools.lru_cache(maxsize=None)
def bc_ref(name):
    case = bc_case(name)
    mfs = bc_data(case, None)
    R = GR.dense_levels(case.levels, mfs, [case.comp], case.ratio, 0, [case.alloc] * len(case.levels))
    return R, [[GR.box_ref(R[l], b, case.alloc, [case.comp]) for b in range(lv.nboxes)] for l, lv in enumerate(case.levels)]


# ----------------------------------------------------------------------------- expected multifabs
MODES = ("fb", "fp", "fo", "seq", "hier")  # each entry point alone, the three calls level by level, pa_fill_ghosts_hierarchy


def mode_calls(case, mode, l):
    """the calls a mode makes on level l, in order"""
    if mode in ("seq", "hier"):
        return ["fb"] + (["fp"] if l else []) + (["fo"] if case.foextrap else [])
    return [mode] if (mode != "fp" or l) else []


def expected(case, init, mode, seed_shift=0):
    """(copies of the multifabs `init` after the mode's calls according to the reference, number of doubles stored)"""
    _, BR = case_ref(case.name, seed_shift)
    out, n = [], 0
    for l, mf in enumerate(init):
        e = mf.copy()
        for call in mode_calls(case, mode, l):
            for b in range(mf.level.nboxes):
                n += GR.apply_call(e.fab(b), BR[l][b], case.comps, call, case.ngs[l])
        out.append(e)
    return out, n
