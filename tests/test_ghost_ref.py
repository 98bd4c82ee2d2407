"""CPU tier of the ghost-fill tests: the dense numpy reference (tests/ghost_ref.py) and the oracle (oracle/pa_oracle.c), written from
different structures -- one array per level against box-by-box loops -- give the same bits on every cell a call may write and leave
every other double alone, on every case of tests/ghost_cases.py; every case reaches the branch it was written for; and a few facts
that need neither of the two."""
import numpy as np
import pytest

import ghost_cases as GC
import ghost_ref as GR
from avgplt_ref import interp_dense
from util import SENT_REF, bits_equal

FILL = [c.name for c in GC.fill_cases()]
BC = [c.name for c in GC.bc_cases()]


def _oracle_mode(oracle, case, mfs, mode):
    for l, mf in enumerate(mfs):
        for call in GC.mode_calls(case, mode, l):
            if call == "fb":
                oracle.fill_boundary(mf, case.comp, case.ncomp, case.ngs[l])
            elif call == "fp":
                assert oracle.fillpatch_two_levels(mf, mfs[l - 1], case.comp, case.ncomp, case.ngs[l], case.ratio, case.interp) == 0, "not properly nested"
            else:
                oracle.foextrap(mf, case.comp, case.ncomp, case.ngs[l])


def _first_diff(got, want):
    for b in range(got.level.nboxes):
        g, w = got.fab(b), want.fab(b)
        bad = np.argwhere(g.view(np.int64) != w.view(np.int64))
        if len(bad):
            c, k, j, i = bad[0]
            return f"box {b} {got.level.boxes[b]}: {len(bad)} cells differ, first comp {c} at FAB index (i,j,k)=({i},{j},{k}): got {g[c, k, j, i]!r} want {w[c, k, j, i]!r}"
    return "padding between components differs"


@pytest.mark.parametrize("name", FILL)
def test_reference_equals_oracle_on_every_cell_a_call_may_write(oracle, name):
    """each entry point alone and the three-call sequence: the oracle's multifab (ghost cells and padding prefilled with a sentinel) equals,
    bit for bit and over the WHOLE buffer, the reference's -- so the values agree and the oracle left every other double untouched"""
    case = GC.fill_case(name)
    init = GC.case_data(case, SENT_REF)
    _, BR = GC.case_ref(name)
    for mode in ("fb", "fp", "fo", "seq"):
        want, n = GC.expected(case, init, mode)
        got = [m.copy() for m in init]
        _oracle_mode(oracle, case, got, mode)
        for l in range(case.nlev):
            assert bits_equal(got[l].data, want[l].data), f"{name} {mode} level {l}: {_first_diff(got[l], want[l])}"
        if mode == "seq":
            assert n > 0
            # no compared cell is NaN, and after the whole sequence every ghost cell within ng holds the dense value
            for l in range(case.nlev):
                for b, B in enumerate(BR[l]):
                    m = (B.layer > 0) & (B.layer <= case.ngs[l]) & ((B.cls < 2) | bool(case.foextrap))
                    for c in case.comps:
                        assert np.isfinite(B.exp[c][m]).all(), f"{name} level {l} box {b}: NaN in the reference (not properly nested)"
                        assert bits_equal(want[l].fab(b)[c][m], B.exp[c][m])


@pytest.mark.parametrize("name", FILL)
def test_every_case_reaches_its_branch(name):
    case = GC.fill_case(name)
    GC.check_expect(case)
    if case.interp == 1 and case.nlev > 1:
        R, BR = GC.case_ref(name)
        zero = lim = free = 0
        for l in range(1, case.nlev):
            z, m, f = GR.limiter_branches(R[l], BR[l], case.comps, case.ngs[l])
            zero, lim, free = zero + z, lim + m, free + f
        if case.two_slopes:
            # no parent can be limited here: with the x slope always 0 (lower and upper neighbour are the same cell) two slopes remain,
            # each at most twice its smaller one-sided difference b_d, so dumax <= (2 b_1 + 2 b_2) / 4 <= max(b_1, b_2) <= u0 - umin
            # (and likewise umax - u0) at ratio 2: the common factor stays 1 whatever the data
            assert lim == 0 and all((R[1].keep[c]["sl"][0] == 0.0).all() for c in case.comps)
            lim = 1
        assert zero > 0 and lim > 0 and free > 0, f"{name}: parents with all slopes zero {zero}, factor below 1 {lim}, slopes and factor 1 {free}"


def test_matrix_covers_the_arguments():
    """the argument values the matrix promises, somewhere in it"""
    C = GC.fill_cases()
    assert {(c.alloc, ng) for c in C for ng in c.ngs} >= {(4, 1), (4, 2), (4, 4)}
    assert {(c.nc, c.comp, c.ncomp) for c in C} >= {(4, 0, 4), (4, 1, 2), (4, 3, 1)}
    assert {c.interp for c in C} == {0, 1} and {c.foextrap for c in C} == {0, 1} and {c.ratio for c in C} == {2, 4}
    B = GC.bc_cases()
    assert {v for c in B for v in c.bc} == {0, 1, 2} and all({c.bc[d] for c in B} == {0, 1, 2} for d in range(3))
    assert {c.only_dir for c in B} == {-1, 0, 1, 2} and {c.alloc for c in B} == {1, 2} and any(c.no_coarse for c in B)
    thick = set()
    for c in B:
        assert c.nc == 3 and c.comp == 2 and c.ccomp == 0
        n = c.levels[1].boxes[:, 3:] - c.levels[1].boxes[:, :3] + 1
        thick |= set(int(v) for v in n.ravel())
        faces = [int(a) * int(b) for row in n for a, b in ((row[0], row[1]), (row[0], row[2]), (row[1], row[2]))]
        assert min(faces) < 256 < max(faces)
    assert thick >= {1, 2, 3, 4}


# ----------------------------------------------------------------------------- facts that need neither oracle nor reference
@pytest.mark.parametrize("name", ["d_uniform", "g_ratio4_interp1", "i_three_124", "f_lshape"])
def test_constant_field_gives_the_constant(oracle, name):
    case = GC.fill_case(name)
    mfs = GC.case_data(case, SENT_REF)
    for mf in mfs:
        for b in range(mf.level.nboxes):
            mf.valid(b)[...] = -3.7
    _oracle_mode(oracle, case, mfs, "seq")
    _, BR = GC.case_ref(name)
    for l, mf in enumerate(mfs):
        for b, B in enumerate(BR[l]):
            m = (B.layer > 0) & (B.layer <= case.ngs[l]) & ((B.cls < 2) | bool(case.foextrap))
            for c in case.comps:
                assert (mf.fab(b)[c][m] == -3.7).all()


@pytest.mark.parametrize("ratio", [2, 4])
@pytest.mark.parametrize("is_per", [(0, 0, 0), (1, 0, 1)])
def test_children_average_to_the_parent(ratio, is_per):
    """cell-conservative: the offsets of the ratio^3 children of a parent cancel in pairs, so their exact sum is ratio^3 parents; every
    child is three rounded additions onto the parent, the sum ratio^3 - 1 more, each within eps / 2 of a partial sum no larger than
    ratio^3 max|child|: the mean is within ratio^3 eps max|child| of the parent.  Piecewise constant: the parent's bits."""
    rng = np.random.default_rng(3)
    c = rng.uniform(-1.0, 1.0, size=(5, 6, 7)) * 10.0 ** rng.integers(-3, 3, size=(5, 6, 7))
    f = interp_dense(c, ratio, is_per, 1)
    ch = f.reshape(5, ratio, 6, ratio, 7, ratio)
    mean = ch.sum(axis=(1, 3, 5)) / ratio ** 3
    bound = ratio ** 3 * np.finfo(np.float64).eps * np.abs(ch).max(axis=(1, 3, 5))
    assert (np.abs(mean - c) <= bound).all()
    p = interp_dense(c, ratio, is_per, 0).reshape(5, ratio, 6, ratio, 7, ratio)
    assert (p.view(np.int64) == c.view(np.int64)[:, None, :, None, :, None]).all()


@pytest.mark.parametrize("name", ["b_interp0", "e_negative_pc", "g_ratio4_interp0"])
def test_piecewise_constant_ghost_cells_hold_the_parents_bits(oracle, name):
    """interp_type 0 through the oracle: every coarse-fine ghost cell is a copy of the coarse cell floor(q / ratio), looked up by plain
    indexing of the coarse level's dense array"""
    case = GC.fill_case(name)
    mfs = GC.case_data(case, SENT_REF)
    _oracle_mode(oracle, case, mfs, "fp")
    R, BR = GC.case_ref(name)
    lv, cl = case.levels[1], case.levels[0]
    cn = cl.domhi.astype(np.int64) - cl.domlo + 1
    seen = 0
    for b, B in enumerate(BR[1]):
        kz, jy, ix = np.nonzero(GR.write_mask(B, "fp", case.ngs[1]))
        q = np.stack([ix, jy, kz], axis=1) + (lv.boxes[b, :3].astype(np.int64) - B.G)
        pc = (np.floor_divide(q, case.ratio) - cl.domlo) % cn
        for c in case.comps:
            assert bits_equal(mfs[1].fab(b)[c][kz, jy, ix], R[0].D[c][pc[:, 2], pc[:, 1], pc[:, 0]])
        seen += len(kz)
    assert seen > 0


# ----------------------------------------------------------------------------- applyBC
@pytest.mark.parametrize("name", BC)
def test_apply_bc_walls_and_classes_equal_the_oracle(oracle, name):
    """the oracle writes +interior / -interior into the face ghost cells beyond a wall, SOMETHING into the coarse-fine ones (nothing,
    and counts them, without a coarse multifab) and leaves every other double alone: edges, corners, second layers, other components,
    the faces of other directions under only_dir"""
    case = GC.bc_case(name)
    init = GC.bc_data(case, SENT_REF)
    _, BR = GC.bc_ref(name)
    for l in range(len(case.levels)):
        got = init[l].copy()
        crse = None if (l == 0 or case.no_coarse) else init[l - 1]
        nbad = oracle.lib().orc_apply_bc(oracle._p(oracle._mf(got)), case.comp, oracle._p(oracle._mf(crse)), case.ccomp, oracle._bc(case.bc), case.ratio, case.only_dir)
        want = init[l].copy()
        ncf = nwall = 0
        for b, B in enumerate(BR[l]):
            cf, wall = GR.apply_bc(want.fab(b), case.comp, B, case.bc, case.only_dir)
            g = got.fab(b)[case.comp]
            written = g.view(np.uint64)[cf] != np.uint64(SENT_REF)
            assert written.all() if crse is not None else not written.any(), f"{name} level {l} box {b}"
            want.fab(b)[case.comp][cf] = g[cf]
            ncf += int(cf.sum())
            nwall += int(wall.sum())
        assert bits_equal(got.data, want.data), f"{name} level {l}: {_first_diff(got, want)}"
        assert nbad == (ncf if crse is None else 0)
        if l:
            assert ncf > 0 and (nwall > 0 or not any(b in (1, 2) for d, b in enumerate(case.bc) if case.only_dir in (-1, d)))
        else:
            assert ncf == 0
