"""do_smooth (curvature.cpp:328-406): what pins the oracle's composite implicit-diffusion solve, since AMReX's
MLABecLaplacian/MLMG cannot be run here (parity unpinned):
  * on one periodic level sin/cos modes are eigenfunctions of the 7-point operator -> exact discrete solution;
  * the composite operator conserves the integral (refluxed fluxes telescope) -> sum_uncovered vol*(A x - x) = 0
    for ANY x, across coarse-fine interfaces, with Neumann walls;
  * the solver reaches the reference's tolerance (1e-12) and the covered coarse cells hold child averages;
  * on the case matrix of smooth_cases.py (L-shaped levels, concave coarse-fine corners, walls, periodic faces, four levels, 2-D) the
    operator is consistent with the PDE: constants, linear and quadratic fields, conservation, second-order convergence to a
    manufactured solution (second half of this file)."""
import numpy as np
import pytest

import smooth_cases as sc
from peleanalysis_amd.hierarchy import Hierarchy, MultiFab, Level, _occupancy, chop_box, nested_hierarchy, fill_analytic, field_flame


def test_single_level_periodic_eigenmode(oracle):
    n = 16
    lv = Level(chop_box((0, 0, 0), (n - 1,) * 3, 8), (0, 0, 0), (n - 1,) * 3, (1, 1, 1), (0, 0, 0), (1, 1, 1))
    rhs = MultiFab(lv, 1, 0)
    kx, ky, kz = 2, 1, 3
    f = lambda x, y, z: 0.5 + 0.25 * np.sin(2 * np.pi * kx * x) * np.cos(2 * np.pi * ky * y) * np.sin(2 * np.pi * kz * z + 0.3)
    fill_analytic(rhs, 0, f)
    dt, h = 3e-3, 1.0 / n
    sol, it, res = oracle.smooth_solve([lv], [rhs], 0, dt, (0, 0, 0), MultiFab, tol=1e-14)
    assert 0 < it < 60 and res <= 1e-14
    lam = sum((2 - 2 * np.cos(2 * np.pi * k * h)) / h ** 2 for k in (kx, ky, kz))
    for b in range(lv.nboxes):
        want = 0.5 + (rhs.valid(b)[0] - 0.5) / (1 + dt * lam)  # constant mode: eigenvalue 0
        assert np.abs(sol[0].valid(b)[0] - want).max() < 1e-13


def _composite_sum(levels, mfs, masks):
    tot = 0.0
    for lv, m, k in zip(levels, mfs, masks):
        vol = float(np.prod(lv.dx))
        for b in range(lv.nboxes):
            tot += vol * float((m.valid(b)[0] * k.valid(b)[0]).sum())
    return tot


def test_composite_operator_conserves_the_integral(oracle):
    H = nested_hierarchy(16, 3, 8, is_per=(1, 1, 0))
    rng = np.random.default_rng(3)
    x = []
    for lv in H.levels:
        m = MultiFab(lv, 1, 1)
        for b in range(lv.nboxes):
            m.valid(b)[0] = rng.random(m.valid(b)[0].shape)
        x.append(m)
    bc = oracle.bc_from_flags((1, 1, 0))
    dt = 2e-3
    y, mask = oracle.smooth_apply(H.levels, x, dt, bc, MultiFab)
    sx, sy = _composite_sum(H.levels, x, mask), _composite_sum(H.levels, y, mask)
    assert abs(sx) > 0.1 and abs(sy - sx) < 1e-13 * abs(sx)
    # the mask really excludes cells: level 0 has 1/8 of its cells covered
    assert abs(sum(float(mask[0].valid(b)[0].sum()) for b in range(H.levels[0].nboxes)) - 16 ** 3 * 7 / 8) < 0.5
    # without the reflux the integral is NOT conserved (the test can fail)
    L = oracle.lib()
    y2 = [MultiFab(lv, 1, 1) for lv in H.levels]
    for l, lv in enumerate(H.levels):
        L.orc_smooth_apply_level(oracle._p(oracle._mf(x[l])), 0, oracle._p(oracle._mf(y2[l])), 0, oracle.C.c_double(dt))
    assert abs(_composite_sum(H.levels, y2, mask) - sx) > 1e-9 * abs(sx)


def test_composite_solve_reaches_tolerance(oracle):
    H = nested_hierarchy(16, 3, 8, is_per=(1, 1, 0))
    rhs = []
    for lv in H.levels:
        m = MultiFab(lv, 1, 0)
        fill_analytic(m, 0, lambda x, y, z: (field_flame(x, y, z, 0) - 300.0) / 1700.0)
        rhs.append(m)
    bc = oracle.bc_from_flags((1, 1, 0))
    dt = 5e-4  # dt/dx^2 = 0.13 / 0.5 / 2 on the three levels
    sol, it, res = oracle.smooth_solve(H.levels, rhs, 0, dt, bc, MultiFab, tol=1e-12)
    assert 0 < it < 100 and res <= 1e-12
    # independent residual check with the composite operator
    x = [MultiFab(lv, 1, 1, s.data.copy()) for lv, s in zip(H.levels, sol)]
    y, mask = oracle.smooth_apply(H.levels, x, dt, bc, MultiFab)
    r = max(float(np.abs((y[l].valid(b)[0] - rhs[l].valid(b)[0]) * mask[l].valid(b)[0]).max()) for l, lv in enumerate(H.levels) for b in range(lv.nboxes))
    assert r <= 2e-12
    # smoothing: bounded by the data, integral conserved, covered coarse cells = child averages
    assert all(s.valid_concat(0).min() >= -1e-12 and s.valid_concat(0).max() <= 1 + 1e-12 for s in sol)
    assert abs(_composite_sum(H.levels, sol, mask) - _composite_sum(H.levels, rhs, mask)) < 1e-12
    c0 = sol[0]
    fine = {tuple(H.levels[1].boxes[b, :3]): sol[1].valid(b)[0] for b in range(H.levels[1].nboxes)}
    lo1 = H.levels[1].boxes[:, :3].min(axis=0)
    for b in range(H.levels[0].nboxes):
        B = H.levels[0].boxes[b]
        v = c0.valid(b)[0]
        for (i, j, k) in [(B[0], B[1], B[2]), (B[3], B[4], B[5])]:
            if mask[0].valid(b)[0][k - B[2], j - B[1], i - B[0]] == 0.0:
                f = 2 * np.array([i, j, k])
                fb = [q for q in range(H.levels[1].nboxes) if np.all(H.levels[1].boxes[q, :3] <= f) and np.all(f + 1 <= H.levels[1].boxes[q, 3:])][0]
                FB = H.levels[1].boxes[fb]
                blk = sol[1].valid(fb)[0][f[2] - FB[2]:f[2] - FB[2] + 2, f[1] - FB[1]:f[1] - FB[1] + 2, f[0] - FB[0]:f[0] - FB[0] + 2]
                assert abs(v[k - B[2], j - B[1], i - B[0]] - blk.mean()) < 1e-15


def _hier2d(per):
    per3 = np.array([per[0], per[1], 0])
    l0 = Level(chop_box((0, 0, 0), (31, 31, 0), 16), (0, 0, 0), (31, 31, 0), per3, np.zeros(3), np.ones(3))
    l1 = Level(chop_box((16, 16, 0), (47, 47, 0), 16), (0, 0, 0), (63, 63, 0), per3, np.zeros(3), np.ones(3))
    return Hierarchy([l0, l1], 2)


def test_2d_single_level_periodic_eigenmode(oracle):
    """the AMREX_SPACEDIM == 2 build: one plane of cells, z a Neumann wall -> the operator is the 5-point one and a 2-D
    Fourier mode is its eigenfunction with the 2-D eigenvalue (no z term)"""
    n = 32
    lv = Level(chop_box((0, 0, 0), (n - 1, n - 1, 0), 16), (0, 0, 0), (n - 1, n - 1, 0), (1, 1, 0), (0, 0, 0), (1, 1, 1))
    rhs = MultiFab(lv, 1, 0)
    kx, ky = 3, 2
    fill_analytic(rhs, 0, lambda x, y, z: 0.5 + 0.25 * np.sin(2 * np.pi * kx * x + 0.1) * np.cos(2 * np.pi * ky * y) + 0 * z)
    dt, h = 1e-3, 1.0 / n
    sol, it, res = oracle.smooth_solve([lv], [rhs], 0, dt, oracle.bc_from_flags((1, 1, 0)), MultiFab, tol=1e-14)
    assert 0 < it < 60 and res <= 1e-14
    lam = sum((2 - 2 * np.cos(2 * np.pi * k * h)) / h ** 2 for k in (kx, ky))
    for b in range(lv.nboxes):
        want = 0.5 + (rhs.valid(b)[0] - 0.5) / (1 + dt * lam)
        assert np.abs(sol[0].valid(b)[0] - want).max() < 1e-13


def test_2d_composite_conserves_and_averages(oracle):
    """2-D hierarchy (refined in x and y only): covered cells are the 2 x 2 child blocks, the refluxed operator conserves
    the integral for any x, and after the solve the covered coarse cells hold the mean of their FOUR children"""
    for per in ((1, 0), (0, 0)):
        H = _hier2d(per)
        rng = np.random.default_rng(5)
        x = []
        for lv in H.levels:
            m = MultiFab(lv, 1, 1)
            for b in range(lv.nboxes):
                m.valid(b)[0] = rng.random(m.valid(b)[0].shape)
            x.append(m)
        bc = oracle.bc_from_flags((per[0], per[1], 0))
        dt = 4e-4
        y, mask = oracle.smooth_apply(H.levels, x, dt, bc, MultiFab)
        ncov = 32 * 32 - sum(float(mask[0].valid(b)[0].sum()) for b in range(H.levels[0].nboxes))
        assert abs(ncov - 16 * 16) < 0.5  # 32 x 32 fine cells cover 16 x 16 coarse ones (ratio 1 in z)
        sx, sy = _composite_sum(H.levels, x, mask), _composite_sum(H.levels, y, mask)
        assert abs(sx) > 0.1 and abs(sy - sx) < 1e-13 * abs(sx)
        rhs = []
        for lv in H.levels:
            m = MultiFab(lv, 1, 0)
            fill_analytic(m, 0, lambda x, y, z: 0.5 * (1.0 + np.tanh((np.hypot(x - 0.5, (y - 0.5) / 0.8) - 0.27) / 0.06)) + 0 * z)
            rhs.append(m)
        sol, it, res = oracle.smooth_solve(H.levels, rhs, 0, dt, bc, MultiFab, tol=1e-13)
        assert 0 < it < 100 and res <= 1e-13
        assert abs(_composite_sum(H.levels, sol, mask) - _composite_sum(H.levels, rhs, mask)) < 1e-12
        xs = [MultiFab(lv, 1, 1, s.data.copy()) for lv, s in zip(H.levels, sol)]
        ys, _ = oracle.smooth_apply(H.levels, xs, dt, bc, MultiFab)
        r = max(float(np.abs((ys[l].valid(b)[0] - rhs[l].valid(b)[0]) * mask[l].valid(b)[0]).max()) for l, lv in enumerate(H.levels) for b in range(lv.nboxes))
        assert r <= 2e-12
        fine = np.zeros((64, 64))
        for b in range(H.levels[1].nboxes):
            B = H.levels[1].boxes[b]
            fine[B[1]:B[4] + 1, B[0]:B[3] + 1] = sol[1].valid(b)[0][0]
        for b in range(H.levels[0].nboxes):
            B = H.levels[0].boxes[b]
            v, k = sol[0].valid(b)[0][0], mask[0].valid(b)[0][0]
            for j in range(B[1], B[4] + 1):
                for i in range(B[0], B[3] + 1):
                    if k[j - B[1], i - B[0]] == 0.0:
                        assert abs(v[j - B[1], i - B[0]] - fine[2 * j:2 * j + 2, 2 * i:2 * i + 2].mean()) < 1e-15


# ---------------------------------------------------------------- the operator against the PDE, on the case matrix (smooth_cases.py)
# Consistency pins that are not the oracle itself: constants and linear fields are reproduced (any wrong interpolation weight, reflux
# factor or average fails them), quadratics are reproduced where the coarse-fine interpolation keeps its order, the integral is
# conserved on every hierarchy, and the solve converges to a manufactured solution of the PDE at second order under refinement.
OP_DT = 2e-3  # dt / dx^2 = 0.5 on a 16-cell level 0, 8 on a 64-cell level 2: every level's stencil and the reflux carry weight
OP_CASES = list(sc.CASES) + ["nested3"]


def _op_case(name):
    if name == "nested3":  # the hierarchy of the three pins above
        return nested_hierarchy(16, 3, 8, is_per=(1, 1, 0)), (1, 1, 0), (1, 1, 0)
    return sc.build(name)


def _apply_dense(oracle, H, fn_or_mfs, bc3, dt=OP_DT):
    """(x, A x) over every level's whole domain for a field given at cell centres, and the uncovered-cell masks"""
    x0 = sc.fill(H, fn_or_mfs) if callable(fn_or_mfs) else fn_or_mfs
    x = sc.with_ghosts(H, x0)
    y, _ = oracle.smooth_apply(H.levels, x, dt, oracle.bc_from_flags(bc3), MultiFab)
    return [sc.dense(lv, m) for lv, m in zip(H.levels, x0)], [sc.dense(lv, m) for lv, m in zip(H.levels, y)], sc.uncovered(H)


def _interior(H, l, width=2):
    """cells of level l at least `width` cells from every domain face (the refined directions of a one-plane hierarchy)"""
    n = H.levels[l].domhi - H.levels[l].domlo + 1
    m = np.zeros((int(n[2]), int(n[1]), int(n[0])), bool)
    w = width
    if sc.is_planar(H):
        m[:, w:-w, w:-w] = True
    else:
        m[w:-w, w:-w, w:-w] = True
    return m


@pytest.mark.parametrize("name", OP_CASES)
def test_operator_reproduces_constants(oracle, name):
    """A c = c on EVERY uncovered cell, walls included, to 8 ulp of c"""
    H, per, bc3 = _op_case(name)
    c = 0.7
    x, y, unc = _apply_dense(oracle, H, lambda xx, yy, zz: c + 0 * (xx + yy + zz), bc3)
    worst = max(float(np.abs(y[l] - c)[unc[l]].max()) for l in range(H.nlev))
    print(f"{name}: max |A c - c| = {worst:.3e}")
    assert worst <= 8 * np.spacing(c), worst


@pytest.mark.parametrize("name", OP_CASES)
def test_operator_reproduces_linear_fields(oracle, name):
    """A x = x for a linear x on the uncovered cells at least 2 cells from every domain face (periodic faces too: the field is not
    periodic); the wall layer itself differs by > 1e-2, so the mask really excludes something"""
    H, per, bc3 = _op_case(name)
    x, y, unc = _apply_dense(oracle, H, lambda xx, yy, zz: 0.3 + 0.5 * xx - 0.2 * yy + 0.4 * zz, bc3)
    worst = max(float(np.abs(y[l] - x[l])[unc[l] & _interior(H, l)].max(initial=0.0)) for l in range(H.nlev))
    wall = max(float(np.abs(y[l] - x[l])[unc[l] & ~_interior(H, l, 1)].max(initial=0.0)) for l in range(H.nlev))
    print(f"{name}: max |A x - x| interior {worst:.3e}, wall layer {wall:.3e}")
    assert worst <= 1e-13, worst
    assert wall > 1e-2, wall


QUAD = (0.2, 0.3, -0.25, 0.15, 0.1, -0.2, 0.05, 0.12, -0.07, 0.09)


def _quad(xx, yy, zz):
    a, b, c, d, e, f, g, h, p, q = QUAD
    return a + b * xx * xx + c * yy * yy + d * zz * zz + e * xx * yy + f * yy * zz + g * xx * zz + h * xx + p * yy + q * zz


def _quad_dev(oracle, H, bc3):
    lap = 2.0 * (QUAD[1] + QUAD[2] + (0.0 if sc.is_planar(H) else QUAD[3]))
    x, y, unc = _apply_dense(oracle, H, _quad, bc3)
    return [np.where(unc[l], np.abs(y[l] - (x[l] - OP_DT * lap)), 0.0) for l in range(H.nlev)], unc


def test_operator_reproduces_quadratics_on_the_nested_hierarchy(oracle):
    """A x = x - dt Lap x for a quadratic x (the 7-point Laplacian, the quadratic coarse-fine interpolation and the averaged fine
    fluxes are all exact for it) on the convex nested hierarchy, away from the domain faces"""
    H, per, bc3 = _op_case("nested3")
    dev, unc = _quad_dev(oracle, H, bc3)
    worst = max(float(dev[l][_interior(H, l)].max()) for l in range(H.nlev))
    print(f"nested3: max |A x - (x - dt Lap x)| = {worst:.3e}")
    assert worst <= 1e-13, worst


def _dilate(m, w, planar):
    out = m.copy()
    for ax in ((1, 2) if planar else (0, 1, 2)):
        acc = out.copy()
        for s in range(1, w + 1):
            acc |= np.roll(out, s, axis=ax) | np.roll(out, -s, axis=ax)  # wraps: lands within w cells of a domain face, allowed anyway
        out = acc
    return out


def _concave(H, unc):
    """per level: uncovered cells that have covered neighbours of the SAME level in two or more directions (the coarse cells in a
    concave coarse-fine edge or corner)"""
    planar = sc.is_planar(H)
    out = []
    for l, lv in enumerate(H.levels):
        cov = _occupancy(lv) & ~unc[l]
        ndir = np.zeros(cov.shape, int)
        for ax in ((1, 2) if planar else (0, 1, 2)):
            lo, hi = np.roll(cov, 1, axis=ax), np.roll(cov, -1, axis=ax)
            per = bool(lv.is_per[2 - ax])
            if not per:  # nothing beyond a wall
                sl = [slice(None)] * 3
                sl[ax] = 0
                lo[tuple(sl)] = False
                sl[ax] = -1
                hi[tuple(sl)] = False
            ndir += (lo | hi)
        out.append(unc[l] & (ndir >= 2))
    return out


def _defect_elsewhere(H, dev, unc):
    """[(level, (i, j, k))] of the cells whose defect exceeds 1e-13 and that lie neither within 2 cells (of their own level) of a
    concave coarse-fine edge nor within 2 cells of a domain face"""
    planar = sc.is_planar(H)
    K = _concave(H, unc)
    assert any(k.any() for k in K), "the case has no concave coarse-fine edge"
    where = []
    for l in range(H.nlev):
        near = _dilate(K[l], 2, planar)
        if l > 0:  # the fine cells next to the coarse corner cell's footprint
            up = K[l - 1].repeat(2, axis=1).repeat(2, axis=2)
            if not planar:
                up = up.repeat(2, axis=0)
            near |= _dilate(up, 2, planar)
        if l + 1 < H.nlev:  # the coarse cells next to a corner cell of the finer level
            f = K[l + 1]
            dn = np.any([f[a::(1 if planar else 2), b::2, c::2] for a in ((0,) if planar else (0, 1)) for b in (0, 1) for c in (0, 1)], axis=0)
            near |= _dilate(dn, 2, planar)
        bad = (dev[l] > 1e-13) & _interior(H, l) & ~near
        print(f"  level {l}: {int((dev[l] > 1e-13).sum())} deviating cells, max {float(dev[l].max()):.2e}; {int(bad.sum())} of them elsewhere, max {float(dev[l][bad].max(initial=0.0)):.2e}")
        where += [(l, tuple(int(v) for v in c[::-1])) for c in np.argwhere(bad)]
    return where


L_SHAPED = ["hand-000", "hand-110", "hand-101", "union4", "union9", "planar_L-00", "planar_L-10", "planar_L-01"]


@pytest.mark.parametrize("name", L_SHAPED)
def test_quadratic_defect_sits_at_concave_corners(oracle, name):
    """On L-shaped regions the coarse-fine interpolation drops an order where its stencil cannot be centred (defects of 1e-6 .. 1e-4 away
    from the walls on the 3-D cases; none at all, 3e-15, on planar_L: a 2-D concave corner keeps the order).  With ONE coarse-fine
    interface -- planar_L, and the first two levels of every 3-D case -- every cell whose A x departs from x - dt Lap x lies within 2 cells (of its own level) of a concave
    coarse-fine edge or of a domain face: asserted.
    With the third level in place the localisation does NOT hold on the oracle as it stands, so it is recorded, not asserted: hand has 149
    further cells (18 on level 0, 131 on level 1; defect <= 3.6e-6), union4 22, union9 4 (<= 5.2e-6; union14 has no concave edge).  They are the
    level-1 cells on a coarse-fine face whose ghost cell's normal stencil (max order 4: three interior cells) reaches a cell
    that level 2 covers -- the nesting buffer is 2 cells -- and the level-0 cells those faces reflux into: a covered cell holds its
    children's average, which differs from the quadratic's centre value by h^2 / 16 * (sum of the second derivatives' halves).  None of them
    is there without level 2 (the two-level assertion), and the nested hierarchy (buffer of 4 cells) has none."""
    H, per, bc3 = _op_case(name)
    if H.nlev > 2:
        dev3, unc3 = _quad_dev(oracle, H, bc3)
        print(f"{name}, three levels (recorded):")
        _defect_elsewhere(H, dev3, unc3)
        H = Hierarchy(H.levels[:2], 2)
    dev, unc = _quad_dev(oracle, H, bc3)
    print(f"{name}, one coarse-fine interface:")
    where = _defect_elsewhere(H, dev, unc)
    print(f"  largest defect away from the domain faces: {max(float(d[_interior(H, l)].max()) for l, d in enumerate(dev)):.2e}")
    assert not where, where[:8]


@pytest.mark.parametrize("name", OP_CASES)
def test_composite_operator_conserves_the_integral_on_every_case(oracle, name):
    """sum over uncovered cells of vol (A x - x) = 0 for a random x: the refluxed fluxes telescope at every coarse-fine face, concave
    corners, walls and periodic faces included"""
    H, per, bc3 = _op_case(name)
    rng = np.random.default_rng(3)
    x = []
    for lv in H.levels:
        m = MultiFab(lv, 1, 1)
        for b in range(lv.nboxes):
            m.valid(b)[0] = rng.random(m.valid(b)[0].shape)
        x.append(m)
    y, mask = oracle.smooth_apply(H.levels, x, OP_DT, oracle.bc_from_flags(bc3), MultiFab)
    sx, sy = _composite_sum(H.levels, x, mask), _composite_sum(H.levels, y, mask)
    print(f"{name}: |sum vol (A x - x)| / |sum vol x| = {abs(sy - sx) / abs(sx):.3e}")
    assert abs(sx) > 0.1 and abs(sy - sx) < 1e-13 * abs(sx)


def _manufactured_error(oracle, H, per, bc3, dt):
    phi, rhs_fn = sc.manufactured(H, per, dt)
    rhs = sc.fill(H, rhs_fn)
    sol, it, res = oracle.smooth_solve(H.levels, rhs, 0, dt, oracle.bc_from_flags(bc3), MultiFab, tol=1e-12, maxiter=2000)
    assert it > 0 and res <= 1e-12, (it, res)
    return sc.max_uncovered(H, sol, fn=phi)


@pytest.mark.parametrize("name,dt", [("hand-000", 2.0 / 64 ** 2), ("hand-110", 2.0 / 64 ** 2), ("planar_L-00", 4e-4), ("planar_L-10", 4e-4)])
def test_composite_solve_converges_to_the_manufactured_solution(oracle, name, dt):
    """phi = 0.5 + 0.3 prod cos(pi k x / L) solves (I - dt Lap) phi = rhs exactly (Neumann walls, periodic faces): the composite solve's
    error over the uncovered cells falls by >= 2.8 when every index is doubled at fixed dt (a first-order scheme gives 2, a coarse-fine
    treatment that is inconsistent with the PDE about 1; the solve's tolerance, 1e-12, is far below the errors), and the refined levels
    do not cost accuracy: the composite error is at most twice that of level 0 solved alone"""
    H, per, bc3 = sc.build(name)
    e1 = _manufactured_error(oracle, H, per, bc3, dt)
    e2 = _manufactured_error(oracle, sc.refine(H), per, bc3, dt)
    e0 = _manufactured_error(oracle, Hierarchy(H.levels[:1], 2), per, bc3, dt)
    print(f"{name}: error {e1:.3e}, refined {e2:.3e}, ratio {e1 / e2:.2f}; level 0 alone {e0:.3e} ({e1 / e0:.2f} x)")
    assert e1 / e2 >= 2.8, (e1, e2)
    assert e1 <= 2.0 * e0, (e1, e0)
