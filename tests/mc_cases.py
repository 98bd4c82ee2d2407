"""The marching-cubes / marching-squares / merge case matrix shared by the golden generator (tests/golden/make_golden_mc.py),
the CPU tier (tests/test_mc_oracle.py: oracle against the reference's recorded output) and the GPU tier
(tests/test_gpu_mc_ref.py: kernels against the same recorded output).  Deterministic: default_rng with fixed seeds; the fields
of the hierarchy cases are rounded to multiples of 2^-10, so that a last-bit difference between two machines' sin / tanh
cannot change an input.  Every 3-D case carries 3 coordinate components and 2 fields (amr3: 1 field, which keeps the
recorded vertices inside the size of a fixture); every 2-D case 2 coordinate components and 2 fields.

A case is a dict:
  name, dim (3 | 2), nc, isocomp, iso, merge (its per-FAB fragments go through the merge, level-then-box order)
  fabs   list of dict(state [nc][nz][ny][nx] (2-D: [nc][ny][nx]), mask, lo, hi, llo, lhi, level, box): every per-FAB run
  H, states, ng, ratio, loops [level] -> (nboxes, 6)      hierarchy cases only (the level entry points of the library)
"""
import ctypes as C
import hashlib

import numpy as np

from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, chop_box


# ------------------------------------------------------------------------------------------------- single FABs, 3-D
def mc_case(n, seed, masked):
    """state FAB over box (-1..n)^3 with 3 coordinate comps + 2 fields; iso field = wrinkled sphere"""
    lo, hi = np.array([-1, -1, -1]), np.array([n, n, n])
    ax = (np.arange(lo[0], hi[0] + 1) + 0.5) / n
    X, Y, Z = ax[None, None, :] + 0 * ax[:, None, None], ax[None, :, None] + 0 * ax[:, None, None], ax[:, None, None] + 0 * ax[None, None, :]
    X, Y, Z = np.broadcast_arrays(X, Y, Z)
    rng = np.random.default_rng(seed)
    r = np.sqrt((X - 0.5) ** 2 + (Y - 0.47) ** 2 + (Z - 0.52) ** 2)
    f = 1000.0 + 900.0 * np.tanh((r - 0.31) / 0.05) + 5.0 * rng.standard_normal(X.shape)
    g = np.sin(3 * X) * np.cos(2 * Y) + Z
    state = np.ascontiguousarray(np.stack([X, Y, Z, f, g]))
    mask = np.ones(X.shape)
    if masked:
        mask[n // 2:, n // 3: 2 * n // 3, : n // 2] = -1.0  # "covered by a finer level"
    # a few exact hits of the iso value and equal neighbours (eps branches of VI_doIt)
    state[3, 3, 4, 5] = 1090.0
    state[3, 7, 7, 7] = state[3, 7, 7, 8]
    return lo, hi, state, mask


_CORNERS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]  # p0 .. p7 of Polygonise as (di, dj, dk)


def cube_indices(f, mask, lo, llo, lhi, iso):
    """cube index of every unmasked loop cell (numpy; -1 where a corner is masked): [nk][nj][ni] over the loop box"""
    o = [int(llo[d] - lo[d]) for d in range(3)]
    n = [int(lhi[d] - llo[d] + 1) for d in range(3)]
    idx = np.zeros((n[2], n[1], n[0]), dtype=np.int64)
    bad = np.zeros(idx.shape, dtype=bool)
    for m, (di, dj, dk) in enumerate(_CORNERS):
        sl = (slice(o[2] + dk, o[2] + dk + n[2]), slice(o[1] + dj, o[1] + dj + n[1]), slice(o[0] + di, o[0] + di + n[0]))
        idx |= (f[sl] < iso).astype(np.int64) << m
        bad |= mask[sl] < 0
    return np.where(bad, -1, idx)


def _fab(state, mask, lo, hi, llo, lhi, level=0, box=0):
    return dict(state=np.ascontiguousarray(state), mask=np.ascontiguousarray(mask), lo=np.asarray(lo, np.int64), hi=np.asarray(hi, np.int64),
                llo=np.asarray(llo, np.int64), lhi=np.asarray(lhi, np.int64), level=level, box=box)


def _coords(lo, hi, dx):
    ax = [(np.arange(lo[d], hi[d] + 1) + 0.5) * dx for d in range(3)]
    return np.broadcast_arrays(ax[0][None, None, :], ax[1][None, :, None], ax[2][:, None, None])


def all_cubes():
    """33 x 33 x 3 points; the cube at base (2a, 2b, 0) has index 16 a + b: all 256 corner sign patterns, every crossing generic"""
    rng = np.random.default_rng(256)
    lo, hi = np.zeros(3, np.int64), np.array([32, 32, 2])
    X, Y, Z = _coords(lo, hi, 1.0 / 33.0)
    sign = rng.choice([-1.0, 1.0], size=X.shape)
    for a in range(16):
        for b in range(16):
            c = 16 * a + b
            for m, (di, dj, dk) in enumerate(_CORNERS):
                sign[dk, 2 * b + dj, 2 * a + di] = -1.0 if (c >> m) & 1 else 1.0
    f = sign * (1.0 + rng.random(X.shape))
    g = rng.random(X.shape)
    state = np.stack([X, Y, Z, f, g])
    mask = np.ones(X.shape)
    llo, lhi = lo.copy(), hi - 1
    ci = cube_indices(f, mask, lo, llo, lhi, 0.0)
    assert set(range(256)) <= set(ci.ravel().tolist()), "all_cubes: not every cube index occurs"
    assert [int(ci[0, 2 * (c % 16), 2 * (c // 16)]) for c in range(256)] == list(range(256))
    return dict(name="all_cubes", dim=3, nc=5, isocomp=3, iso=0.0, merge=False, fabs=[_fab(state, mask, lo, hi, llo, lhi)])


def vi_branches(O, state, mask, lo, llo, lhi, isocomp, iso, eps=1.0e-15):
    """from the inputs alone: the edges of one FAB by the branch of VI_doIt they take, in the orientation (p1, p2) of the FIRST
    VertexInterp call that meets them (base points x fastest; edge e of a cube joins the corners _EDGE_ENDS[e], in that order).
    -> dict: 'p1_below' / 'p1_above' (first early return, the near value < iso or not), 'p2_below' / 'p2_above', 'equal', 'generic'"""
    edge_table, _ = O.mc_tables()
    ends = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
    f = state[isocomp]
    ci = cube_indices(f, mask, lo, llo, lhi, iso)
    seen, out = set(), dict(p1_below=0, p1_above=0, p2_below=0, p2_above=0, equal=0, generic=0)
    for kk in range(ci.shape[0]):
        for jj in range(ci.shape[1]):
            for ii in range(ci.shape[2]):
                c = int(ci[kk, jj, ii])
                if c <= 0 or edge_table[c] == 0:
                    continue
                base = (int(llo[0]) + ii, int(llo[1]) + jj, int(llo[2]) + kk)
                for e in range(12):
                    if not (edge_table[c] >> e) & 1:
                        continue
                    pa, pb = (tuple(base[d] + _CORNERS[q][d] for d in range(3)) for q in ends[e])
                    key = (min(pa[::-1], pb[::-1]), max(pa[::-1], pb[::-1]))
                    if key in seen:
                        continue
                    seen.add(key)
                    v1, v2 = (float(f[p[2] - lo[2], p[1] - lo[1], p[0] - lo[0]]) for p in (pa, pb))
                    if abs(iso - v1) < eps:
                        out["p1_below" if v1 < iso else "p1_above"] += 1
                    elif abs(iso - v2) < eps:
                        out["p2_below" if v2 < iso else "p2_above"] += 1
                    elif abs(v1 - v2) < eps:
                        out["equal"] += 1
                    else:
                        out["generic"] += 1
    return out


def near_iso_fab(seed, n=16):
    """one n^3-point FAB, O(1) field, iso 0.5; a quarter of the points at 0.5 + m 1e-16, m in [-14, 14]: within VI_doIt's 1e-15 of
    the iso value on either side of the `<` that sets the cube index (at the workload's 1090 one ulp is 2.3e-13, and those
    branches fire on exact equality only); a few masked points"""
    rng = np.random.default_rng(seed)
    lo, hi = np.zeros(3, np.int64), np.full(3, n - 1)
    X, Y, Z = _coords(lo, hi, 1.0 / n)
    f = rng.random(X.shape)
    near = rng.random(X.shape) < 0.25
    m = rng.integers(-14, 15, size=X.shape)
    f = np.where(near, 0.5 + m * 1.0e-16, f)
    g = rng.random(X.shape)
    mask = np.ones(X.shape)
    mask.ravel()[rng.choice(mask.size, 5, replace=False)] = -1.0
    return _fab(np.stack([X, Y, Z, f, g]), mask, lo, hi, lo.copy(), hi - 1)


def near_iso(O):
    fb = near_iso_fab(1090)
    br = vi_branches(O, fb["state"], fb["mask"], fb["lo"], fb["llo"], fb["lhi"], 3, 0.5)
    for k in ("p1_below", "p1_above", "p2_below", "p2_above", "generic"):
        assert br[k] > 0, f"near_iso: no edge takes VI_doIt's branch {k}: {br}"
    return dict(name="near_iso", dim=3, nc=5, isocomp=3, iso=0.5, merge=False, fabs=[fb], branches=br)


def exact_1090():
    lo, hi, state, mask = mc_case(12, 7 + 12, False)
    return dict(name="exact_1090", dim=3, nc=5, isocomp=3, iso=1090.0, merge=False, fabs=[_fab(state, mask, lo, hi, lo.copy(), hi - 1)])


def masked_edges():
    """one 12^3-point FAB, four runs: a single masked point; a masked slab flush with the loop box's high side; a loop box one
    cell thick; an empty loop box"""
    lo, hi, state, ones = mc_case(10, 5, False)
    assert tuple(ones.shape) == (12, 12, 12)
    llo, lhi = lo.copy(), hi - 1
    m1 = ones.copy(); m1[6, 5, 4] = -1.0
    m2 = ones.copy(); m2[:, :, -1] = -1.0  # the points i = hi: every cell with base i = lhi loses a corner
    thin_lo, thin_hi = llo.copy(), lhi.copy()
    thin_lo[2] = thin_hi[2] = 4
    empty_hi = lhi.copy(); empty_hi[0] = llo[0] - 1
    fabs = [_fab(state, m1, lo, hi, llo, lhi, box=0), _fab(state, m2, lo, hi, llo, lhi, box=1), _fab(state, ones, lo, hi, thin_lo, thin_hi, box=2),
            _fab(state, ones, lo, hi, llo, empty_hi, box=3)]
    return dict(name="masked_edges", dim=3, nc=5, isocomp=3, iso=1090.0, merge=False, fabs=fabs)


# ------------------------------------------------------------------------------------------------- hierarchies
def _round10(v):
    return np.round(v * 1024.0) / 1024.0


def build_states(O, H, field_fn, nfield, ng, ratio, seed, dim=3):
    """state build of isosurface.cpp:1434-1528 through the oracle's pieces: analytic coordinates on the grown FABs, the fields
    on the valid cells (rounded to 2^-10), FillBoundary, piecewise-constant FillPatchTwoLevels"""
    nc = dim + nfield
    states = []
    for l, lv in enumerate(H.levels):
        rng = np.random.default_rng(seed + 17 * l)
        st = MultiFab(lv, nc, ng, fill=-666.0)
        for b in range(lv.nboxes):
            f = st.fab(b)
            lo = lv.boxes[b, :3] - ng
            nz, ny, nx = f.shape[1:]
            x = ((np.arange(lo[0], lo[0] + nx) + 0.5) * lv.dx[0] + lv.prob_lo[0])[None, None, :]
            y = ((np.arange(lo[1], lo[1] + ny) + 0.5) * lv.dx[1] + lv.prob_lo[1])[None, :, None]
            z = ((np.arange(lo[2], lo[2] + nz) + 0.5) * lv.dx[2] + lv.prob_lo[2])[:, None, None]
            f[0], f[1] = x, y
            if dim == 3:
                f[2] = z
            v = st.valid(b)
            xv, yv, zv = x[:, :, ng:nx - ng], y[:, ng:ny - ng, :], z[ng:nz - ng, :, :]
            for m in range(nfield):
                v[dim + m] = _round10(field_fn(xv, yv, zv, m) + 1e-3 * rng.uniform(-1, 1, size=v[dim + m].shape))
        O.fill_boundary(st, 0, nc, ng)
        if l > 0:
            assert O.lib().orc_fillpatch_two_levels(C.byref(O._mf(st)), C.byref(O._mf(states[l - 1])), 0, nc, ng, ratio, 0) == 0
        states.append(st)
    return states


def _hier_case(O, name, H, states, ng, ratio, iso, dim=3, merge=True):
    nc = states[0].ncomp
    fabs, loops = [], []
    for l, lv in enumerate(H.levels):
        lp = np.zeros((lv.nboxes, 6), np.int64)
        for b in range(lv.nboxes):
            lo, hi, mask, llo, lhi = O.iso_fab_inputs(H.levels, states, l, b, ng, ratio=ratio)
            st = np.ascontiguousarray(states[l].fab(b))
            if dim == 2:  # the plane k = 0 of a hierarchy one cell thick
                llo[2] = lhi[2] = 0
                lp[b, :3], lp[b, 3:] = llo, lhi
                fabs.append(_fab(st[:, ng], mask[ng], lo[:2], hi[:2], llo[:2], lhi[:2], l, b))
            else:
                lp[b, :3], lp[b, 3:] = llo, lhi
                fabs.append(_fab(st, mask, lo, hi, llo, lhi, l, b))
        loops.append(lp)
    return dict(name=name, dim=dim, nc=nc, isocomp=dim, iso=float(iso), merge=merge, fabs=fabs, H=H, states=states, ng=ng, ratio=ratio, loops=loops)


def _median_iso(states, comp):
    return float(np.median(np.concatenate([s.valid(b)[comp].ravel() for s in states for b in range(s.level.nboxes)])))


def field_tube(x, y, z, m=0):
    """a wrinkled tube along x, through the periodic face: small surfaces keep the recorded vertices inside a fixture's size"""
    r = np.sqrt((y - 0.5) ** 2 + (z - 0.47) ** 2)
    return (1.0 + 0.1 * m) * (1000.0 + 600.0 * np.tanh((r - 0.07 - 0.015 * np.sin(2 * np.pi * x + 0.4)) / 0.05)) + 3.0 * m * np.sin(2 * np.pi * x)


def field_ball(x, y, z, m=0):
    """a wrinkled ball across the high-x face of ratio4_hierarchy's fine level (x = 2/3)"""
    r = np.sqrt((x - 0.66) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    return (1.0 + 0.1 * m) * (1000.0 + 600.0 * np.tanh((r - 0.09 - 0.01 * np.sin(9 * y) * np.cos(7 * z)) / 0.04)) + 3.0 * m * np.sin(5 * x)


def amr_r2_periodic(O, ng):
    """2 levels, base 24^3 (dx is no power of two: fine and coarse coordinates differ in the last bits), periodic in x; the fine
    level refines coarse cells [0, 9] x [6, 17] x [6, 17] -- flush with the periodic face -- in boxes <= 16 cells wide.
    A merge case with either ghost width (the fragments untrimmed)."""
    per = (1, 0, 0)
    l0 = Level(chop_box((0, 0, 0), (23, 23, 23), 12), (0, 0, 0), (23, 23, 23), per, np.zeros(3), np.ones(3))
    l1 = Level(chop_box((0, 12, 12), (19, 35, 35), 16), (0, 0, 0), (47, 47, 47), per, np.zeros(3), np.ones(3))
    assert (l1.boxes[:, 3:] - l1.boxes[:, :3] + 1).max() <= 16 and (l1.boxes[:, 0] == 0).any()
    H = Hierarchy([l0, l1], 2)
    states = build_states(O, H, field_tube, 2, ng, 2, seed=24 + ng)
    return _hier_case(O, f"amr_r2_periodic_ng{ng}", H, states, ng, 2, 1040.0)


def ratio4_hierarchy(per):
    """2 levels, refinement ratio 4: base 24^3 in 12^3 boxes; level 1 = coarse cells [6, 15] x [6, 17] x [8, 15] refined (x4) in boxes <= 24"""
    l0 = Level(chop_box((0, 0, 0), (23, 23, 23), 12), (0, 0, 0), (23, 23, 23), per, np.zeros(3), np.ones(3))
    l1 = Level(chop_box((24, 24, 32), (63, 71, 63), 24), (0, 0, 0), (95, 95, 95), per, np.zeros(3), np.ones(3))
    return Hierarchy([l0, l1], 4)


def amr_r4(O):
    H = ratio4_hierarchy((0, 0, 0))
    states = build_states(O, H, field_ball, 2, 1, 4, seed=5)
    return _hier_case(O, "amr_r4", H, states, 1, 4, 1040.0)


def amr3(O):
    """amr3_wall_z of util.build_config (base 32^3, 3 levels, 16^3 boxes, periodic in x and y), iso at the median; ONE field"""
    from util import build_config
    H, per, sym, fn = build_config("amr3_wall_z")
    states = build_states(O, H, fn, 1, 1, 2, seed=11)
    return _hier_case(O, "amr3", H, states, 1, 2, _median_iso(states, 3))


# ------------------------------------------------------------------------------------------------- 2-D
def squares_all():
    """one 2-D FAB (a level of one box, one cell thick, 1 ghost layer): the square at base (2a - 1, 2b - 1) has case 4 a + b,
    all 16 cases, the two saddles (5, 10) included"""
    rng = np.random.default_rng(16)
    ng = 1
    lv = Level(np.array([[0, 0, 0, 6, 6, 0]], np.int32), (0, 0, 0), (6, 6, 0), (0, 0, 0), np.zeros(3), np.array([1.0, 1.0, 1.0 / 7.0]))
    H = Hierarchy([lv], 2)
    st = MultiFab(lv, 4, ng, fill=-666.0)
    f = st.fab(0)  # [4][3][9][9]
    x = ((np.arange(-1, 8) + 0.5) * lv.dx[0])[None, None, :]
    y = ((np.arange(-1, 8) + 0.5) * lv.dx[1])[None, :, None]
    f[0], f[1] = x, y
    sign = rng.choice([-1.0, 1.0], size=(9, 9))
    corners = [(0, 0), (1, 0), (1, 1), (0, 1)]  # p0 .. p3 of Segmentise as (di, dj)
    for a in range(4):
        for b in range(4):
            for m, (di, dj) in enumerate(corners):
                sign[2 * b + dj, 2 * a + di] = -1.0 if ((4 * a + b) >> m) & 1 else 1.0
    f[2] = (sign * (1.0 + rng.random((9, 9))))[None, :, :]
    f[3] = rng.random((9, 9))[None, :, :]
    lo, hi = np.array([-1, -1]), np.array([7, 7])
    llo, lhi = lo.copy(), hi - 1
    v = f[2, ng]
    case = sum(((v[dj:dj + 8, di:di + 8] < 0.0).astype(int) << m) for m, (di, dj) in enumerate(corners))
    assert set(range(16)) <= set(case.ravel().tolist())
    loops = [np.array([[llo[0], llo[1], 0, lhi[0], lhi[1], 0]], np.int64)]
    fabs = [_fab(np.ascontiguousarray(f[:, ng]), np.ones((9, 9)), lo, hi, llo, lhi)]
    return dict(name="squares_all", dim=2, nc=4, isocomp=2, iso=0.0, merge=False, fabs=fabs, H=H, states=[st], ng=ng, ratio=2, loops=loops)


def squares_amr(O, per):
    """the two-level 2-D hierarchy of test_marching_squares_level_matches_oracle, stored as one plane of cells"""
    ng, nc = 1, 4
    l0 = Level(chop_box((0, 0, 0), (15, 15, 0), 8), (0, 0, 0), (15, 15, 0), np.asarray(per), np.zeros(3), np.ones(3))
    l1 = Level(chop_box((8, 8, 0), (23, 23, 0), 8), (0, 0, 0), (31, 31, 0), np.asarray(per), np.zeros(3), np.ones(3))
    H = Hierarchy([l0, l1], 2)
    rng = np.random.default_rng(8)
    states = []
    for l, lv in enumerate(H.levels):
        st = MultiFab(lv, nc, ng, fill=-666.0)
        for b in range(lv.nboxes):
            f = st.fab(b)
            lo = lv.boxes[b, :3] - ng
            nz, ny, nx = f.shape[1:]
            x = ((np.arange(lo[0], lo[0] + nx) + 0.5) * lv.dx[0] + lv.prob_lo[0])[None, None, :]
            y = ((np.arange(lo[1], lo[1] + ny) + 0.5) * lv.dx[1] + lv.prob_lo[1])[None, :, None]
            f[0], f[1] = x, y
            v = st.valid(b)
            xv, yv = x[:, :, ng:-ng], y[:, ng:-ng, :]
            v[2] = _round10(1000.0 + 500.0 * np.sin(2 * np.pi * xv) * np.cos(2 * np.pi * yv) + 200.0 * (yv - 0.5) + 1e-3 * rng.standard_normal(v[2].shape))
            v[3] = _round10(xv * yv)
        O.fill_boundary(st, 0, nc, ng)
        if l > 0:
            assert O.lib().orc_fillpatch_two_levels(C.byref(O._mf(st)), C.byref(O._mf(states[l - 1])), 0, nc, ng, 2, 0) == 0
        states.append(st)
    return _hier_case(O, "squares_amr_per%d" % per[0], H, states, ng, 2, 1040.0, dim=2)


# ------------------------------------------------------------------------------------------------- the matrix
def cases(O):
    return [all_cubes(), near_iso(O), exact_1090(), masked_edges(), amr_r2_periodic(O, 1), amr_r2_periodic(O, 2), amr_r4(O), amr3(O), squares_all(),
            squares_amr(O, (0, 0, 0)), squares_amr(O, (1, 0, 0))]


SMALL_INPUT = 20000  # numbers: a case's inputs are stored in the fixture up to this size (an array that several runs share
#                       counted once), as a SHA-256 of their bytes beyond it


def input_arrays(case):
    """the inputs of a case as one list of arrays, in a fixed order"""
    out = []
    for fb in case["fabs"]:
        out += [fb["state"], fb["mask"], fb["lo"], fb["hi"], fb["llo"], fb["lhi"]]
    return out


def unique_inputs(arrays):
    """-> (the distinct arrays in order of first use, for every array its index among them)"""
    uniq, index, seen = [], [], {}
    for a in arrays:
        a = np.ascontiguousarray(a)
        key = (a.dtype.str, a.shape, a.tobytes())
        if key not in seen:
            seen[key] = len(uniq)
            uniq.append(a)
        index.append(seen[key])
    return uniq, np.array(index, dtype=np.int64)


def input_digest(case):
    h = hashlib.sha256()
    for a in input_arrays(case):
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def fragments(per_fab):
    """per-FAB (verts, keys, elts) in level-then-box order -> the merge's fragments (FABs without a vertex are left out)"""
    return [(v, t) for (v, _, t) in per_fab if len(v)]


def synthetic_cluster_fragments(nc=5):
    """the hand-made merge input of test_gpu_filter_mc.test_iso_merge_synthetic_clusters: exact copies and copies 1-3 ulp away in
    later fragments (in either direction), nodes on and next to the faces of the 1e-14 hash cells, an element that collapses once
    its nodes merge, the same element from two fragments in two rotations.  -> (fragments, data(p): positions -> node rows)"""
    rng = np.random.default_rng(17)
    base = np.concatenate([rng.random((400, 3)), 0.25 + 1.0e-14 * rng.integers(0, 50, (60, 3)), 0.5 + 1.0e-14 * rng.integers(0, 4, (60, 3)) + rng.choice([0.0, 1e-16, -1e-16], (60, 3))])
    base = np.unique(base, axis=0)
    rng.shuffle(base)

    def data(p):  # node data is carried along from the FIRST copy: make the copies distinguishable
        return np.concatenate([p, rng.random((len(p), nc - 3))], axis=1)

    frags = []
    n0 = len(base)
    t0 = rng.integers(0, n0, (900, 3)).astype(np.int32)
    frags.append((data(base), t0))
    for rep in range(3):
        pick = rng.choice(n0, 150, replace=False)
        p = base[pick].copy()
        ulps = rng.integers(-3, 4, p.shape)
        for _ in range(3):
            p = np.where(ulps > 0, np.nextafter(p, 2.0), np.where(ulps < 0, np.nextafter(p, -1.0), p))
            ulps = ulps - np.sign(ulps)
        extra = rng.random((40, 3))
        pts = np.concatenate([p, extra])
        rng.shuffle(pts)
        t = rng.integers(0, len(pts), (500, 3)).astype(np.int32)
        frags.append((data(pts), t))
    # the first fragment's elements again, rotated, through a fragment that holds exact copies of its nodes
    frags.append((data(base), np.roll(t0[:200], 1, axis=1)))
    frags.append((np.zeros((0, nc)), np.zeros((0, 3), np.int32)))
    return frags, data


# ------------------------------------------------------------------------------------------------- the recorded reference output
def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc_ref.npz")


def load_golden(path=None):
    """tests/golden/mc_ref.npz -> {name: dict(iso, sha, inputs (list of arrays, or None where only the digest is kept),
    per_fab [(verts, keys, elts)], merged (nodes, elts) or None)}: what the reference's compiled code returned"""
    g = np.load(path or golden_path())
    out = {}
    for k in (str(s) for s in g["names"]):
        dim, nc = int(g[k + "_dim"]), int(g[k + "_nc"])
        nv, ne = g[k + "_nv"].astype(np.int64), g[k + "_ne"].astype(np.int64)
        V, K, T = g[k + "_V"].reshape(-1, nc), g[k + "_K"].astype(np.int32).reshape(-1, 2 * dim), g[k + "_T"].astype(np.int32).reshape(-1, dim)
        ov, oe = np.concatenate([[0], np.cumsum(nv)]), np.concatenate([[0], np.cumsum(ne)])
        per_fab = [(V[ov[q]:ov[q + 1]], K[ov[q]:ov[q + 1]], T[oe[q]:oe[q + 1]]) for q in range(len(nv))]
        merged = None
        if k + "_msrc" in g.files:  # node i of the merge is, bit for bit, vertex msrc[i] of the fragments laid end to end (checked when recorded)
            fv = np.concatenate([v for v, _ in fragments(per_fab)] + [np.zeros((0, nc))])
            merged = (fv[g[k + "_msrc"].astype(np.int64)], g[k + "_melts"].astype(np.int32).reshape(-1, dim))
        n_in, imap = int(g[k + "_nin"]), g[k + "_inmap"].astype(np.int64)
        out[k] = dict(name=k, dim=dim, nc=nc, iso=float(g[k + "_iso"]), sha=str(g[k + "_sha"]), per_fab=per_fab, merged=merged,
                      inputs=[g[f"{k}_in{q}"] for q in imap] if n_in else None)
    return out


def assert_same_surface(got, want, what=""):
    """(verts, keys, elts) or (nodes, elts) of `got` against `want`: the same counts, keys and connectivity equal entry by entry
    (order included), floating-point data equal as int64 views -- bit for bit, a NaN or a signed zero included"""
    assert len(got) == len(want), f"{what}: {len(got)} arrays against {len(want)}"
    fl_g, fl_w = np.ascontiguousarray(got[0], dtype=np.float64), np.ascontiguousarray(want[0], dtype=np.float64)
    assert fl_g.shape == fl_w.shape, f"{what}: {fl_g.shape[0]} vertices of {fl_g.shape[1:]} components, the reference has {fl_w.shape[0]} of {fl_w.shape[1:]}"
    for n, (a, b) in enumerate(zip(got[1:], want[1:])):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype.kind == "i" and b.dtype.kind == "i", f"{what}: integer arrays expected"
        label = "connectivity" if n == len(got) - 2 else "edge keys / vertex order"
        assert a.shape == b.shape, f"{what}: {label}: shape {a.shape}, the reference has {b.shape}"
        if not np.array_equal(a, b):
            q = int(np.argwhere((a != b).any(axis=1))[0, 0])
            raise AssertionError(f"{what}: {label} differ, first at row {q}: {a[q].tolist()} against the reference's {b[q].tolist()}")
    if not np.array_equal(fl_g.view(np.int64), fl_w.view(np.int64)):
        q = int(np.argwhere((fl_g.view(np.int64) != fl_w.view(np.int64)).any(axis=1))[0, 0])
        raise AssertionError(f"{what}: vertex data not bit-identical, first at vertex {q}: {fl_g[q].tolist()!r} against the reference's {fl_w[q].tolist()!r}")
