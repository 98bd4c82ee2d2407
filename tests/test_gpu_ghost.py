"""GPU tier of the ghost-fill tests: pa_fill_boundary, pa_fillpatch_two_levels, pa_foextrap, pa_fill_ghosts_hierarchy and pa_apply_bc
against the dense numpy reference of tests/ghost_ref.py on the matrix of tests/ghost_cases.py (the CPU tier, test_ghost_ref.py, holds
that reference to the oracle and every case to its branch).  Every multifab starts as SENT_GPU in every double but the valid cells
and is compared WHOLE, bit for bit: the cells a call may write hold the reference's bits, everything else -- layers beyond the ng
argument, other components, the padding between components, the cells of another call's class, valid cells -- is as it was.  Every
comparison is of bits or of counts, but one: the coarse-fine face ghosts of pa_apply_bc, which equal the oracle's bits, are ALSO held cell
by cell to the dense long-double reference of tests/gradcurv_ref.py within its derived bound, so they do not rest on the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import ghost_cases as GC
import ghost_ref as GR
import gradcurv_cases as GCC
import gradcurv_ref as GCR
from peleanalysis_amd import capi
from util import SENT_GPU, bits_equal, sentinel_count

pytestmark = pytest.mark.gpu

FILL = [c.name for c in GC.fill_cases()]
BC = [c.name for c in GC.bc_cases()]


def _diff(got, want, init):
    for b in range(got.level.nboxes):
        g, w = got.fab(b), want.fab(b)
        bad = np.argwhere(g.view(np.int64) != w.view(np.int64))
        if len(bad):
            c, k, j, i = bad[0]
            was = init.fab(b)[c, k, j, i]
            return (f"box {b} {got.level.boxes[b]}: {len(bad)} cells differ, first comp {c} at FAB index (i,j,k)=({i},{j},{k}): got {g[c, k, j, i]!r} "
                    f"want {w[c, k, j, i]!r} (before the call: {was!r}; {sentinel_count(g, SENT_GPU)} sentinels got, {sentinel_count(w, SENT_GPU)} wanted)")
    return "padding between components differs"


def _assert_whole(got, want, init, nstored, what):
    """the whole buffer, bit for bit; valid cells as uploaded; as many doubles changed as the reference stores (a store of the bits a
    cell already held -- foextrap alone copying a sentinel -- changes nothing on either side)"""
    assert bits_equal(got.data, want.data), f"{what}: {_diff(got, want, init)}"
    for b in range(got.level.nboxes):
        assert bits_equal(got.valid(b), init.valid(b)), f"{what}: valid cells of box {b} changed"
    changed = int(np.count_nonzero(got.data.view(np.int64) != init.data.view(np.int64)))
    assert changed == nstored, f"{what}: {changed} doubles changed, the reference stores {nstored}"


def _run_mode(ctx, case, dmf, mode):
    """the calls of a mode; returns FillBoundary's launch records (tag 3) of the mode"""
    ctx.sync()
    ctx.profile_read(3, reset=True)
    if mode == "hier":
        hm = (C.c_void_p * case.nlev)(*[d.h for d in dmf])
        hg = (C.c_int32 * case.nlev)(*case.ngs)
        ctx.check(ctx.lib.pa_fill_ghosts_hierarchy(ctx.h, case.nlev, hm, case.comp, case.ncomp, hg, case.ratio, case.interp, case.foextrap))
    else:
        for l in range(case.nlev):
            for call in GC.mode_calls(case, mode, l):
                if call == "fb":
                    ctx.check(ctx.lib.pa_fill_boundary(ctx.h, dmf[l].h, case.comp, case.ncomp, case.ngs[l]))
                elif call == "fp":
                    ctx.check(ctx.lib.pa_fillpatch_two_levels(ctx.h, dmf[l].h, dmf[l - 1].h, case.comp, case.ncomp, case.ngs[l], case.ratio, case.interp))
                else:
                    ctx.check(ctx.lib.pa_foextrap(ctx.h, dmf[l].h, case.comp, case.ncomp, case.ngs[l]))
    ctx.sync()
    assert ctx.bc_errors() == 0, f"{case.name} {mode}: coarse data missing"
    return ctx.profile_read(3, reset=True)[0]


def _stored(init, want):
    return sum(int(np.count_nonzero(w.data.view(np.int64) != i.data.view(np.int64))) for i, w in zip(init, want))


def _fill_records(case, mode, fallbacks):
    """tag-3 records: one per pa_fill_boundary call (and one for the hierarchy call's FillBoundary step); the per-cell kernel adds one per
    launch, the region form none.  Under PA_FORCE_FALLBACKS the hierarchy call is the per-level calls"""
    if mode in ("fp", "fo"):
        return 0
    if fallbacks:
        return 2 * case.nlev
    return 1 if mode == "hier" else case.nlev


@pytest.mark.parametrize("fallbacks", [0, 1], ids=["plans", "fallbacks"])
@pytest.mark.parametrize("name", FILL)
def test_fill_matrix(ctx, options, name, fallbacks):
    """each entry point alone, the three calls level by level, and pa_fill_ghosts_hierarchy, with the region / parent-list forms and,
    under PA_FORCE_FALLBACKS=1, with the per-cell kernels and the per-level path of the hierarchy call: the same bits.  Which form of
    FillBoundary ran is read off the tag-3 launch records (every level of the matrix has a region plan -- case h through the O(n^2)
    candidate search -- so without the switch no per-cell launch may show)"""
    case = GC.fill_case(name)
    options(PA_FORCE_FALLBACKS=1 if fallbacks else None)
    init = GC.case_data(case, SENT_GPU)
    dls = [capi.DevLevel(ctx, lv) for lv in case.levels]
    dmf = [capi.DevMF(ctx, dl, case.nc, case.alloc) for dl in dls]
    ctx.profile_enable(1 << 3)
    try:
        for mode in GC.MODES:
            want, n = GC.expected(case, init, mode)
            for d, m in zip(dmf, init):
                d.upload(m)
            rec = _run_mode(ctx, case, dmf, mode)
            stored = _stored(init, want)
            assert stored == n or mode == "fo"
            for l in range(case.nlev):
                _assert_whole(dmf[l].download(), want[l], init[l], _stored([init[l]], [want[l]]), f"{name} {mode} level {l}")
            assert rec == _fill_records(case, mode, fallbacks), f"{name} {mode}: {rec} FillBoundary records, expected {_fill_records(case, mode, fallbacks)}"
    finally:
        ctx.profile_enable(False)
        for d in dmf:
            d.close()
        for dl in dls:
            dl.close()


@pytest.mark.parametrize("fallbacks", [0, 1], ids=["plans", "fallbacks"])
def test_plans_are_kept_per_ghost_width_and_serve_new_data(ctx, options, fallbacks):
    """on ONE pair of levels: ng 4 (the plans are made), ng 4 again with other data (the plans are reused), ng 2 (plans of their own,
    not the ng-4 ones), and ng 4 once more -- three calls and the hierarchy call each time, each into re-uploaded multifabs"""
    options(PA_FORCE_FALLBACKS=1 if fallbacks else None)
    c4, c2 = GC.fill_case("b_interp1"), GC.fill_case("b_interp1_ng2")
    dls = [capi.DevLevel(ctx, lv) for lv in c4.levels]
    dmf = [capi.DevMF(ctx, dl, c4.nc, c4.alloc) for dl in dls]
    try:
        for case, shift in ((c4, 0), (c4, 1), (c2, 0), (c4, 0)):
            init = GC.case_data(case, SENT_GPU, shift)
            for mode in ("seq", "hier"):
                want, _ = GC.expected(case, init, mode, shift)
                for d, m in zip(dmf, init):
                    d.upload(m)
                _run_mode(ctx, case, dmf, mode)
                for l in range(case.nlev):
                    _assert_whole(dmf[l].download(), want[l], init[l], _stored([init[l]], [want[l]]), f"{case.name} data {shift} {mode} level {l}")
    finally:
        for d in dmf:
            d.close()
        for dl in dls:
            dl.close()


def test_bad_arguments_are_refused_before_any_launch(ctx):
    """ng beyond the allocated width, a component range past the end, ng larger than a periodic domain, interp_type 2, ratio 1 and 17:
    non-zero, no launch recorded, not one double changed"""
    case = GC.fill_case("b_interp1")  # fine level: 8 cells in periodic x
    a = GC.fill_case("a_ng4")         # 6 x 5 x 4, periodic
    init = GC.case_data(case, SENT_GPU)
    dls = [capi.DevLevel(ctx, lv) for lv in case.levels]
    dmf = [capi.DevMF.from_host(ctx, dl, m) for dl, m in zip(dls, init)]
    ainit = GC.random_mf(a.levels[0], 1, 5, 3, SENT_GPU)
    al = capi.DevLevel(ctx, a.levels[0])
    am = capi.DevMF.from_host(ctx, al, ainit)
    L, h, f, c = ctx.lib, ctx.h, dmf[1].h, dmf[0].h
    hm = (C.c_void_p * 2)(c, f)
    ha = (C.c_void_p * 1)(am.h)

    def ngs(*v):
        return (C.c_int32 * len(v))(*v)
    ctx.sync()
    ctx.profile_enable(1 << 3)
    ctx.profile_read(3, reset=True)
    try:
        refused = {
            "fill_boundary ng > allocated": L.pa_fill_boundary(h, f, 0, 4, 5),
            "fillpatch ng > allocated": L.pa_fillpatch_two_levels(h, f, c, 0, 4, 5, 2, 1),
            "foextrap ng > allocated": L.pa_foextrap(h, f, 0, 4, 5),
            "hierarchy ng > allocated": L.pa_fill_ghosts_hierarchy(h, 2, hm, 0, 4, ngs(4, 5), 2, 1, 1),
            "fill_boundary components": L.pa_fill_boundary(h, f, 2, 3, 4),
            "fillpatch components": L.pa_fillpatch_two_levels(h, f, c, 2, 3, 4, 2, 1),
            "foextrap components": L.pa_foextrap(h, f, 4, 1, 4),
            "hierarchy components": L.pa_fill_ghosts_hierarchy(h, 2, hm, 3, 2, ngs(4, 4), 2, 1, 1),
            "fill_boundary negative component": L.pa_fill_boundary(h, f, -1, 2, 4),
            "fill_boundary ng > periodic domain": L.pa_fill_boundary(h, am.h, 0, 1, 5),
            "hierarchy ng > periodic domain": L.pa_fill_ghosts_hierarchy(h, 1, ha, 0, 1, ngs(5), 2, 1, 1),
            "fillpatch interp 2": L.pa_fillpatch_two_levels(h, f, c, 0, 4, 4, 2, 2),
            "hierarchy interp 2": L.pa_fill_ghosts_hierarchy(h, 2, hm, 0, 4, ngs(4, 4), 2, 2, 1),
            "fillpatch ratio 1": L.pa_fillpatch_two_levels(h, f, c, 0, 4, 4, 1, 1),
            "fillpatch ratio 17": L.pa_fillpatch_two_levels(h, f, c, 0, 4, 4, 17, 1),
            "hierarchy ratio 1": L.pa_fill_ghosts_hierarchy(h, 2, hm, 0, 4, ngs(4, 4), 1, 1, 1),
            "hierarchy ratio 17": L.pa_fill_ghosts_hierarchy(h, 2, hm, 0, 4, ngs(4, 4), 17, 1, 1),
        }
        ctx.sync()
        assert all(rc != 0 for rc in refused.values()), {k: v for k, v in refused.items() if v == 0}
        assert ctx.profile_read(3, reset=True)[0] == 0
        assert ctx.bc_errors() == 0
        for d, m in zip(dmf + [am], init + [ainit]):
            assert bits_equal(d.download().data, m.data)
    finally:
        ctx.profile_enable(False)
        for d in dmf + [am]:
            d.close()
        for dl in dls + [al]:
            dl.close()


# ----------------------------------------------------------------------------- applyBC
@pytest.mark.parametrize("fallbacks", [0, 1], ids=["plans", "fallbacks"])
@pytest.mark.parametrize("name", BC)
def test_apply_bc_matrix(ctx, oracle, options, name, fallbacks):
    """pa_apply_bc on component 2 of 3 with the coarse component 0: the face ghost cells beyond a wall hold +interior / -interior (the
    reference), the coarse-fine ones the oracle's bits (its stencil is held by the polynomial known answers of
    test_oracle_known_answers.py) AND lie within the derived bound of the dense long-double reference of tests/gradcurv_ref.py, which
    shares no box arithmetic with the oracle or the library; nothing else changed: edge, corner and second-layer ghosts, the other
    components, the faces of other directions under only_dir.  Without a coarse multifab the coarse-fine face ghosts stay sentinels and
    pa_bc_errors counts them"""
    case = GC.bc_case(name)
    options(PA_FORCE_FALLBACKS=1 if fallbacks else None)
    init = GC.bc_data(case, SENT_GPU)
    _, BR = GC.bc_ref(name)
    dense, _ = GCC.bc_ref(name)
    dls = [capi.DevLevel(ctx, lv) for lv in case.levels]
    dmf = [capi.DevMF.from_host(ctx, dl, m) for dl, m in zip(dls, init)]
    st = GCC.Stat()
    try:
        for l in range(len(case.levels)):
            has_crse = l > 0 and not case.no_coarse
            ctx.sync()
            assert ctx.bc_errors() == 0
            ctx.check(ctx.lib.pa_apply_bc(ctx.h, dmf[l].h, case.comp, dmf[l - 1].h if has_crse else None, case.ccomp, capi._i3(case.bc), case.ratio, case.only_dir))
            ctx.sync()
            orc = init[l].copy()
            oracle.lib().orc_apply_bc(oracle._p(oracle._mf(orc)), case.comp, oracle._p(oracle._mf(init[l - 1] if has_crse else None)), case.ccomp, oracle._bc(case.bc),
                                      case.ratio, case.only_dir)
            want = init[l].copy()
            ncf, masks = 0, []
            for b, B in enumerate(BR[l]):
                cf, wall = GR.apply_bc(want.fab(b), case.comp, B, case.bc, case.only_dir)
                if has_crse:
                    want.fab(b)[case.comp][cf] = orc.fab(b)[case.comp][cf]
                ncf += int(cf.sum())
                masks.append((cf, wall))
            assert ctx.bc_errors() == (0 if has_crse else ncf), f"{name} level {l}"
            got = dmf[l].download()
            _assert_whole(got, want, init[l], _stored([init[l]], [want]), f"{name} level {l}")
            assert dense[l][1] == (0 if has_crse else ncf), f"{name} level {l}: the dense reference counts {dense[l][1]} cells without coarse data"
            for b, (v, e, cfm, wallm) in enumerate(dense[l][0]):
                cf, wall = masks[b]
                assert np.array_equal(GCR.ring1(cf, case.alloc), cfm) and np.array_equal(GCR.ring1(wall, case.alloc), wallm), f"{name} level {l} box {b}: the two references classify alike"
                if has_crse:
                    g = GCR.ring1(got.fab(b)[case.comp], case.alloc)
                    assert sentinel_count(g[cfm], SENT_GPU) == 0 and np.isfinite(g[cfm]).all(), f"{name} level {l} box {b}"
                    st.add(g[cfm], v[cfm], e[cfm], f"{name} level {l} box {b}: coarse-fine ghost cells against the dense reference")
        if not case.no_coarse:
            print(st.check_cap(f"GPU apply_bc {name} (coarse-fine ghosts, dense reference)"))
    finally:
        for d in dmf:
            d.close()
        for dl in dls:
            dl.close()
