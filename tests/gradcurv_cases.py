"""The case matrix of the grad -> curvature reference tests, shared by the CPU tier (test_gradcurv_ref.py: tests/gradcurv_ref.py against
the oracle) and the GPU tier (test_gpu_gradcurv_ref.py: the kernels against that reference).  The shapes are the smallest at which
the kernels can still go wrong, not the workload's.  Every reference is computed once (functools.lru_cache) and never changed.

pa_apply_bc alone: random O(1) data (ghost_cases.random_mf), so a wrong weight shows at O(1).  Pipelines: a tilted ramp in all three
directions plus a smooth trigonometric term plus noise; no flat region, so |grad c| stays far from the 1e-14 branch of the normal
(asserted from the reference, ghost cells included: a normal is only ever formed on valid cells, from resolved ghost values).
The options of pa_curvature_run read a velocity at components 1..3 (field_vel, pipe_states(ncomp=4)): ramps and trigonometric terms in
all three directions in every component plus noise from a generator of its own, so that the scalar and every cached reference of the
core keep their bits."""
import dataclasses
import functools

import numpy as np

import ghost_cases as GC
import gradcurv_ref as GCR
from peleanalysis_amd.hierarchy import Level, MultiFab, cell_centers, nested_hierarchy, union_hierarchy

BcCase = GC.BcCase


def _bc_of(levels, odd=()):
    return tuple(0 if p else (2 if d in odd else 1) for d, p in enumerate(levels[0].is_per))


def geo_slots():
    """a fine base slab with three arms on its high y face that leave a slot ONE coarse cell wide (x 6..7) and a slot TWO coarse cells
    wide (x 10..13): the base's ghost cells in the first slot have a fine box on either side in x (1-point tangential stencil), those in
    the second slot have one on one side and, two coarse cells on, on the other (2-point stencil: the extension to -+2 is covered);
    the arms B and C are one coarse cell wide themselves (2 cells thick: NX = 3)"""
    c = GC._dom((0, 0, 0), (10, 10, 10), (0, 0, 0))
    boxes = [[2, 4, 4, 15, 7, 11], [2, 8, 4, 5, 11, 11], [8, 8, 4, 9, 11, 11], [14, 8, 4, 15, 11, 11]]
    return [c, GC._fine(c, boxes)]


@functools.lru_cache(maxsize=None)
def bc_cases():
    """every ghost_cases.bc_cases() entry and the geometries the coarse-fine stencil selection was written for"""
    C = list(GC.bc_cases())

    def add(name, levels, branch, odd=(), **kw):
        C.append(BcCase(name, levels, _bc_of(levels, odd), branch, **kw))
    add("geo_c", GC.geo_c(False), "fine level 4 cells wide in periodic x: the tangential neighbours lie two periods out", alloc=1)
    add("geo_c_split", GC.geo_c(True), "the same with boxes 1 and 3 wide in x (NX = 2 and 4 on the x faces, all of them covered)", alloc=2)
    add("geo_d", GC.geo_d(), "fine boxes in a wall corner: the tangential neighbour beyond the wall is not usable (one-sided stencils)", odd=(1,))
    add("geo_e", GC.geo_e(), "negative, odd cell indices: floor division in the coarse index and in xInt", alloc=2)
    add("geo_f", GC.geo_f(), "L-shaped fine region: concave corner, partly covered face, a periodic image that is coarse", odd=(2,))
    add("slots", geo_slots(), "slots one and two coarse cells wide between fine boxes: 1-point and 2-point tangential stencils")
    add("geo_g_ratio4", GC.geo_g(), "refinement ratio 4 (pa_apply_bc refuses it with coarse data: quirk Q11; the oracle takes it)", ratio=4, alloc=2)
    names = [c.name for c in C]
    assert len(set(names)) == len(names)
    return C


def bc_case(name):
    return next(c for c in bc_cases() if c.name == name)


def bc_data(case, fill_bits):
    return GC.bc_data(case, fill_bits)


@functools.lru_cache(maxsize=None)
def bc_ref(name, plant=None):
    """(per level (per box (value, bound, coarse-fine mask, wall mask) on the 1-grown box, cells without coarse data), the Ref)"""
    case = bc_case(name)
    mfs = bc_data(case, None)
    ref = GCR.Ref(case.levels, case.ratio, plant)
    out = []
    for l in range(len(case.levels)):
        has_crse = l > 0 and not case.no_coarse
        boxes, nmiss, _ = GCR.apply_bc(case.levels, l, mfs[l], case.comp, mfs[l - 1] if has_crse else None, case.ccomp, case.bc, case.ratio, case.only_dir, ref=ref)
        out.append((boxes, nmiss))
    return out, ref


# ----------------------------------------------------------------------------- pipelines
@dataclasses.dataclass
class PipeCase:
    name: str
    levels: list
    sym: tuple
    branch: str
    threshold: float
    expect: tuple = ()     # branch counts that must be non-zero
    seed: int = 11

    @property
    def bc(self):
        return [0 if p else (2 if s else 1) for p, s in zip(self.levels[0].is_per, self.sym)]


def _wide_levels():
    """fine boxes of 65 x 13 x 21 cells.  The wide sweep (pa_fused_sweep.hip: march_launch / march_grid; pa_fused_march3.h) cuts a box into
    tiles of 64 columns x MTY rows (13 rows from 52 rows per box up, 8 from 16 up, else 4) x kseg planes (FUSED_KSEG = 64, shortened by
    the launcher's model for small levels, never below 4: 11 here).  65 = 64 + 1 columns, 13 = 3 x 4 + 1 rows, 21 = 11 + 10 planes: two
    column tiles, four row tiles and two z segments, each with a remainder; boxes wider than 32 cells take the wide sweep"""
    per = (1, 0, 1)
    l0 = Level(np.array([[0, 0, 0, 79, 23, 31]]), (0, 0, 0), (79, 23, 31), per, (0, 0, 0), (1, 1, 1))
    fb = [[16 + 65 * a, 10 + 13 * b, 12 + 21 * c, 16 + 65 * a + 64, 10 + 13 * b + 12, 12 + 21 * c + 20] for c in range(2) for b in range(2) for a in range(2)]
    l1 = Level(np.array(fb), (0, 0, 0), (159, 47, 63), per, (0, 0, 0), (1, 1, 1))
    return [l0, l1]


def _general_levels():
    """two levels, the fine one a union of rectangles from hierarchy.union_hierarchy: not convex"""
    H = union_hierarchy(5, nlev=2, n0=(16, 16, 16), is_per=(1, 0, 0), base_box=8)
    assert H.nlev == 2
    return H.levels


def _tall_levels():
    """two fine boxes of more than 64 planes in ONE level, a narrow and a wide one.  The options pass (pa_curvopts.hip, k_curvopts) cuts a
    box into rows of 32 cells (boxes at most 32 wide) or 64, 4 rows per workgroup, and marches z in segments of 64 planes; its grid is
    sized by the largest box of the level and every box decodes it with its own tile counts.  16 x 10 x 70: rows of 32 with 16 lanes idle,
    10 = 8 + 2 rows, 70 = 64 + 6 planes.  34 x 6 x 66: one 64-column tile with 30 lanes idle, 6 = 4 + 2 rows, 66 = 64 + 2 planes.  The
    gap between the two is two coarse cells wide"""
    per = (1, 0, 0)
    l0 = Level(np.array([[0, 0, 0, 39, 11, 43]]), (0, 0, 0), (39, 11, 43), per, (0, 0, 0), (1, 1, 1))
    l1 = Level(np.array([[4, 2, 8, 19, 11, 77], [24, 4, 10, 57, 9, 75]]), (0, 0, 0), (79, 23, 87), per, (0, 0, 0), (1, 1, 1))
    return [l0, l1]


def _kgwide_levels():
    """every box of every level wider than 32 cells and at least 16 rows tall: pa_curvature_run forms the Gaussian curvature inside the
    sweep (pa_curvature_last_path == 2) and recomputes the first layer behind special faces.  Fine boxes of 34 x 18 x 10 (34 = 32 + 2
    columns, 18 = 2 x 8 + 2 rows), staggered in y and z across their shared x face"""
    per = (1, 0, 0)
    l0 = Level(np.array([[0, 0, 0, 47, 23, 11]]), (0, 0, 0), (47, 23, 11), per, (0, 0, 0), (1, 1, 1))
    l1 = Level(np.array([[10, 6, 4, 43, 23, 13], [44, 14, 6, 77, 31, 15]]), (0, 0, 0), (95, 47, 23), per, (0, 0, 0), (1, 1, 1))
    return [l0, l1]


@functools.lru_cache(maxsize=None)
def pipe_cases():
    C = [
        PipeCase("narrow", nested_hierarchy(32, 3, 16, is_per=(1, 1, 0)).levels, (0, 0, 0), "3 nested levels, boxes 16 wide (narrow sweep); periodic x y, wall z", 0.3,
                 ("st3c", "cross_on", "nx4", "clipped")),
        PipeCase("sym", nested_hierarchy(32, 3, 8, is_per=(0, 1, 1)).levels, (1, 0, 0), "3 levels, boxes 8 wide; reflect-odd x, periodic y z", 0.3, ("st3c", "cross_on", "nx4", "clipped")),
        PipeCase("ragged", nested_hierarchy(24, 2, 8, is_per=(0, 0, 0)).levels, (0, 1, 0), "2 levels, base 24, boxes 8 (CONFIGS amr2_allwalls_ragged); all walls, y symmetric", 0.3,
                 ("st3c", "cross_on", "nx4", "clipped")),
        PipeCase("deep", nested_hierarchy(16, 5, 8, is_per=(1, 1, 0)).levels, (0, 0, 0), "5 levels: more than one batched launch takes (PA_MAXB = 4); windowed dense arrays", 0.3,
                 ("st3c", "cross_on", "nx4", "clipped")),
        PipeCase("wide", _wide_levels(), (0, 0, 0), "boxes 65 x 13 x 21: the wide sweep with a remainder in columns, rows and planes", 0.3, ("st3c", "cross_on", "nx4", "clipped")),
        PipeCase("general", _general_levels(), (0, 1, 0), "non-convex fine BoxArray: concave corner, partly covered faces (the fused entry points list its irregular cells, pa_fused_irreg.hip; "
                 "pass by pass with fused = 0)", 0.3,
                 ("st3o", "cross_off", "clipped")),
        PipeCase("tall", _tall_levels(), (0, 0, 0), "a narrow (16 x 10 x 70) and a wide (34 x 6 x 66) fine box in one level: a second z segment of the options pass in both tile "
                 "shapes, a grid sized by one box and decoded by the other; periodic x, walls y z", 0.3, ("st3c", "cross_on", "nx4", "clipped")),
        PipeCase("kgwide", _kgwide_levels(), (0, 1, 0), "every box wider than 32 cells and at least 16 rows tall (Gaussian curvature inside the sweep), fine boxes 34 x 18 x 10 "
                 "staggered across their shared x face; periodic x, reflect-odd y, wall z", 0.3, ("st3c", "cross_on", "nx4", "clipped")),
    ]
    return C


def pipe_case(name):
    return next(c for c in pipe_cases() if c.name == name)


def field_ramp(x, y, z):
    """300 + 1500 (tilted ramp + trig): the ramp's slope (0.9, 0.7, 1.1) exceeds the trig term's gradient (at most 0.05 * 4 pi) everywhere"""
    return 300.0 + 1500.0 * ((0.9 * x + 0.7 * y + 1.1 * z) + 0.05 * np.sin(2 * np.pi * x + 0.4) * np.cos(2 * np.pi * y) * np.sin(4 * np.pi * z + 0.3))


@functools.lru_cache(maxsize=None)
def _pipe_valid(name):
    """the valid data, per level per box; the noise is 5 % of the ramp's step from cell to cell on the level (6e-4 of the field's range on
    a 32-cell level), so that the normal turns by a few per cent from cell to cell on every level and K is of the size of 1 / dx"""
    case = pipe_case(name)
    out = []
    for l, lv in enumerate(case.levels):
        rng = np.random.default_rng(1000 * case.seed + l)
        vals = []
        for b in range(lv.nboxes):
            x, y, z = cell_centers(lv, b, 0)
            v = field_ramp(x, y, z)
            vals.append(v + 0.05 * 1500.0 * float(lv.dx.min()) * rng.uniform(-1, 1, size=v.shape))
        out.append(vals)
    return out


def field_vel(x, y, z):
    """three velocity components, each a tilted ramp in all three directions plus a trigonometric term in all three: no derivative
    d u_d / d x_m vanishes, and the divergence (3.3 from the ramps, the trigonometric terms add at most 0.3 * 2 pi + 0.25 * 2 pi +
    0.2 * 2 pi = 4.7 with changing signs) is of the size of the single derivatives"""
    tp = 2 * np.pi
    return (2.0 + 1.3 * x + 0.4 * y - 0.6 * z + 0.3 * np.sin(tp * x + 0.2) * np.cos(tp * y) * np.cos(tp * z + 0.5),
            -1.0 + 0.5 * x + 0.9 * y + 0.7 * z + 0.25 * np.cos(tp * x) * np.sin(tp * y + 0.3) * np.sin(tp * z),
            0.5 - 0.8 * x + 0.6 * y + 1.1 * z + 0.2 * np.sin(tp * x + 0.7) * np.sin(tp * y + 0.1) * np.cos(tp * z))


@functools.lru_cache(maxsize=None)
def _pipe_vel_valid(name):
    """the velocity's valid data, per level per box three arrays; noise of 5 % of a unit slope's step from cell to cell on the level, as
    the scalar's is, from a generator of its own (the scalar keeps its bits)"""
    case = pipe_case(name)
    out = []
    for l, lv in enumerate(case.levels):
        rng = np.random.default_rng(1000 * case.seed + l + 500)
        vals = []
        for b in range(lv.nboxes):
            x, y, z = cell_centers(lv, b, 0)
            vals.append([u + 0.05 * float(lv.dx.min()) * rng.uniform(-1, 1, size=u.shape) for u in field_vel(x, y, z)])
        out.append(vals)
    return out


def pipe_states(name, ng, fill_bits=None, ncomp=1):
    """host multifabs (ncomp = 1: one component; ncomp = 4: the velocity at components 1..3; ng ghost layers) with the case's valid data;
    ghost cells and padding hold fill_bits (NaN if None)"""
    assert ncomp in (1, 4)
    case = pipe_case(name)
    out = []
    vel = _pipe_vel_valid(name) if ncomp == 4 else None
    for l, (lv, vals) in enumerate(zip(case.levels, _pipe_valid(name))):
        mf = MultiFab(lv, ncomp, ng)
        if fill_bits is None:
            mf.data[...] = np.nan
        else:
            mf.data.view(np.uint64)[...] = np.uint64(fill_bits)
        for b in range(lv.nboxes):
            mf.valid(b)[0] = vals[b]
            for d in range(ncomp - 1):
                mf.valid(b)[1 + d] = vel[l][b][d]
        out.append(mf)
    return out


@functools.lru_cache(maxsize=None)
def grad_ref(name, plant=None):
    """(per level [gx, gy, gz, |g|], the Ref)"""
    case = pipe_case(name)
    ref = GCR.Ref(case.levels, 2, plant)
    return ref.grad(pipe_states(name, 1), 0, case.bc), ref


@functools.lru_cache(maxsize=None)
def curv_ref(name, threshold, plant=None):
    """(per level dict c / n / K / clip, the Ref: its counts, its min_normgrad -- the smallest |grad c| less its bound over all cells where a
    normal is formed -- and its valid(l, b, dense array))"""
    case = pipe_case(name)
    ref = GCR.Ref(case.levels, 2, plant)
    out = ref.curvature(pipe_states(name, 2), 0, case.bc, threshold)
    return out, ref


OPT_NAMES = ("Kg", "SR", "VN") + tuple(f"ROST{q}" for q in range(9))   # output components 5, 6, 7, 8..16


def opt_field(o, k):
    """the F of output component k (5..16) in a level's dict of opts_ref"""
    return (o["Kg"], o["SR"], o["VN"])[k - 5] if k < 8 else o["ROST"][k - 8]


@functools.lru_cache(maxsize=None)
def opts_ref(name, threshold, plant=None):
    """(per level dict Kg / SR / VN / ROST, the Ref) of the options on the case's state with the velocity at components 1..3; on top of
    curv_ref's core (the new plants touch the options alone), which stays as it is"""
    case = pipe_case(name)
    core, _ = curv_ref(name, threshold)
    ref = GCR.Ref(case.levels, 2, plant)
    return ref.options(pipe_states(name, 2, ncomp=4), 0, 1, case.bc, threshold, core=core), ref


# ----------------------------------------------------------------------------- the comparison
LD = np.longdouble
CAP = 1e-8  # the bound must not hide a failure: largest bound / L-inf of the reference's component, per case


class Stat:
    """worst error / bound, largest bound and L-inf of the reference over the cells of one (case, component)"""

    def __init__(self):
        self.ratio, self.bound, self.linf, self.n = 0.0, 0.0, 0.0, 0

    def add(self, got, v, e, what):
        assert np.isfinite(got).all(), f"{what}: non-finite values"
        assert np.isfinite(v).all() and np.isfinite(e).all(), f"{what}: the reference is not finite"
        d, bd = np.abs(got.astype(LD) - v), 2 * e
        bad = d > bd
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} cells beyond the bound, worst |got - ref| = {float(d[bad].max()):.3e} at a bound of {float(bd[bad][np.argmax(d[bad])]):.3e}"
        nz = bd > 0
        if nz.any():
            self.ratio = max(self.ratio, float((d[nz] / bd[nz]).max()))
        if got.size:
            self.bound, self.linf, self.n = max(self.bound, float(bd.max())), max(self.linf, float(np.abs(v).max())), self.n + got.size

    def check_cap(self, what):
        assert self.n > 0 and self.linf > 0, what
        assert self.bound / self.linf < CAP, f"{what}: bound / L-inf = {self.bound / self.linf:.2e}"
        return f"{what}: err/bound {self.ratio:.3f}  bound/Linf {self.bound / self.linf:.1e}  ({self.n} cells)"
