"""GPU tier: the filter kernels of csrc/pa_filter.hip on the case matrix of tests/filter_cases.py, against the independent numpy
references of tests/filter_ref.py (which tests/test_filter_ref.py holds to the oracle on the same cases).  Per case and filter mode:

  launch     pa_filter_last_launch reports the launch the case was written for
  exact      the output equals tap_order bit for bit, and equals the oracle
  separable  every cell is within the a-priori rounding bound of the exact sum, against its OWN M = sum |w w w| |q|, and equals
             sep_model -- the kernel's documented operation order -- bit for bit
  sentinels  no sentinel left in a compared cell; nothing written outside the valid boxes or the component range
and, for the separable kernel, one dense field gives the same bits however it is cut into boxes."""
import ctypes as C

import numpy as np
import pytest

import filter_cases as FC
import filter_ref as R
from peleanalysis_amd import capi
from util import SENT_GPU, assert_no_sentinel, assert_untouched, ref_out, sentinel_count, sentinel_out

pytestmark = pytest.mark.gpu

_oracle_cache = {}


def last_launch(ctx):
    info = (C.c_int32 * 8)()
    ctx.check(ctx.lib.pa_filter_last_launch(ctx.h, info))
    return tuple(info)


def _wc(w):
    return (C.c_double * len(w))(*w)


def _oracle_out(oracle, case):
    if case.id not in _oracle_cache:
        w = FC.weights(case.wname, case.ng)[1]
        oo = ref_out(FC.level(case), FC.NCOMP)
        src = FC.input_mf(case).copy()
        oracle.lib().orc_apply_filter(C.byref(oracle._mf(src)), C.byref(oracle._mf(oo)), FC.COMPS[0], len(FC.COMPS), case.ng, _wc(w))
        _oracle_cache[case.id] = oo
    return _oracle_cache[case.id]


def _assert_only_written(got, scomp, ncomp, what):
    """the valid cells of components scomp .. scomp + ncomp - 1 hold no sentinel; every other double of the multifab -- ghost cells,
    the other components, the padding between components -- still holds SENT_GPU"""
    comps = list(range(scomp, scomp + ncomp))
    assert_no_sentinel(got, comps, what)
    assert_untouched(got, [c for c in range(got.ncomp) if c not in comps], what)
    written = got.data.size - sentinel_count(got.data, SENT_GPU)
    assert written == ncomp * got.level.ncells, f"{what}: {written} doubles written, the valid cells of {ncomp} components are {ncomp * got.level.ncells}"


def _check_values(oracle, case, mode, got, scomp, ncomp, what):
    sep = (case.sep if mode == "separable" else case.exa)[0] == 1
    ng = case.ng
    for b in range(got.level.nboxes):
        for c in range(scomp, scomp + ncomp):
            g, tag = got.valid(b)[c], f"{what} box {b} comp {c}"
            if sep:
                tot, mag = FC.ref_exact(case)[b][c]
                FC.assert_bound(g, tot, mag, ng, f"{tag}: kernel against the exact sum")
                FC.assert_bits(g, FC.ref_model(case)[b][c], f"{tag}: kernel against sep_model")
            else:
                FC.assert_bits(g, FC.ref_tap(case)[b][c], f"{tag}: kernel against tap_order")
                if case.dim == 3:
                    FC.assert_bits(g, _oracle_out(oracle, case).valid(b)[c], f"{tag}: kernel against the oracle")


def _variants(case):
    """(entry, ghost layers of the output, scomp, ncomp)"""
    if not case.variants:
        return [("level", 0, 0, 2)]
    entries = ("level", "fab") if len(case.boxes) == 1 else ("level",)
    return [(e, og, sc, nc) for e in entries for og in (0, 1) for sc, nc in FC.RANGES]


def _run_case(ctx, oracle, mode, case):
    lv, w = FC.level(case), FC.weights(case.wname, case.ng)[1]
    want_info = case.sep if mode == "separable" else case.exa
    with capi.DevLevel(ctx, lv) as dl, capi.DevMF.from_host(ctx, dl, FC.input_mf(case)) as di:
        for entry, og, scomp, ncomp in _variants(case):
            what = f"{case.id} [{mode}, {entry} entry, output ng {og}, comps {scomp}..{scomp + ncomp - 1}]"
            with sentinel_out(ctx, dl, FC.NCOMP, og) as do:
                if case.dim == 2:
                    ctx.check(ctx.lib.pa_boxfilter_level2d(ctx.h, di.h, do.h, scomp, ncomp, case.ng, _wc(w)))
                elif entry == "level":
                    ctx.check(ctx.lib.pa_boxfilter_level(ctx.h, di.h, do.h, scomp, ncomp, case.ng, _wc(w)))
                else:
                    ctx.check(ctx.lib.pa_boxfilter_fab(ctx.h, capi.box_of(lv, 0), di.fab(0), do.fab(0), scomp, ncomp, case.ng, _wc(w)))
                ctx.sync()
                info = last_launch(ctx)
                got = do.download()
            print(f"launch {what}: {info}")
            assert info == want_info, f"{what}: launch {info}, the case is written for {want_info}"
            _assert_only_written(got, scomp, ncomp, what)
            _check_values(oracle, case, mode, got, scomp, ncomp, what)


@pytest.mark.parametrize("case", FC.CASES, ids=[c.id for c in FC.CASES])
def test_filter_case(ctx, oracle, filter_mode, case):
    _run_case(ctx, oracle, filter_mode, case)


@pytest.mark.parametrize("case", FC.CASES_2D, ids=[c.id for c in FC.CASES_2D])
def test_filter_case_2d(ctx, oracle, filter_mode, case):
    """k_boxfilter2d (the same kernel in either mode) against the 2-D tap_order, m outer and l inner"""
    _run_case(ctx, oracle, filter_mode, case)


def test_filter_hierarchy_entry_with_a_width_per_level(ctx, oracle, filter_mode):
    """pa_boxfilter_hierarchy: two levels, ng 3 on the first and ng 2 on the second, each held to its own case's references; the
    launch record is the last level's"""
    cases = [next(c for c in FC.CASES if c.id == cid) for cid in ("b67x18x5-ng3-box", "mixed3-ng2-box")]
    ws = [FC.weights(c.wname, c.ng)[1] for c in cases]
    own = []
    try:
        dls = [capi.DevLevel(ctx, FC.level(c)) for c in cases]
        own += dls
        din = [capi.DevMF.from_host(ctx, dl, FC.input_mf(c)) for dl, c in zip(dls, cases)]
        own += din
        dout = [sentinel_out(ctx, dl, FC.NCOMP) for dl in dls]
        own += dout
        wcs = [_wc(w) for w in ws]
        pw = (C.POINTER(C.c_double) * 2)(*[C.cast(a, C.POINTER(C.c_double)) for a in wcs])
        ctx.check(ctx.lib.pa_boxfilter_hierarchy(ctx.h, 2, capi._handles(din), capi._handles(dout), 1, 2, (C.c_int32 * 2)(*[c.ng for c in cases]), pw))
        ctx.sync()
        info = last_launch(ctx)
        assert info == (cases[1].sep if filter_mode == "separable" else cases[1].exa), info
        for c, d in zip(cases, dout):
            got = d.download()
            _assert_only_written(got, 1, 2, f"hierarchy call, {c.id}")
            _check_values(oracle, c, filter_mode, got, 1, 2, f"hierarchy call, {c.id} [{filter_mode}]")
    finally:
        for m in reversed(own):  # multifabs before their levels
            m.close()


@pytest.mark.parametrize("ng", FC.INVARIANCE_NG)
def test_separable_filter_does_not_depend_on_the_tiling(ctx, options, ng):
    """one ghost-filled dense field of 67 x 18 x 11 cells filtered as one box and as a ragged chop (boxes 23 / 22 / 22 wide, 9 rows,
    6 / 5 planes), each through pa_boxfilter_level and box by box through pa_boxfilter_fab: every launch separable, every cell the
    same bits whichever launch made it -- and those of sep_model"""
    options(PA_FILTER_EXACT=None)
    nx, ny, nz = FC.INVARIANCE_DOMAIN
    g = ng + 1
    w = FC.weights("box", ng)[1]
    dense = FC.dense_field(f"invariance-{ng}", (0, 0, 0), (nx - 1, ny - 1, nz - 1), g)
    want = R.sep_model(np.ascontiguousarray(dense[0]), g, ng, w)
    for boxes in ([(0, 0, 0, nx - 1, ny - 1, nz - 1)], FC.chop_box((0, 0, 0), (nx - 1, ny - 1, nz - 1), FC.INVARIANCE_CHOP)):
        lv = FC.level_of(boxes)
        src = FC.cut_input(lv, dense, (-g, -g, -g), g)
        with capi.DevLevel(ctx, lv) as dl, capi.DevMF.from_host(ctx, dl, src) as di:
            for entry in ("level", "fab"):
                with sentinel_out(ctx, dl, FC.NCOMP) as do:
                    if entry == "level":
                        ctx.check(ctx.lib.pa_boxfilter_level(ctx.h, di.h, do.h, 0, 1, ng, _wc(w)))
                        assert last_launch(ctx)[0] == 1, last_launch(ctx)
                    else:
                        for b in range(lv.nboxes):
                            ctx.check(ctx.lib.pa_boxfilter_fab(ctx.h, capi.box_of(lv, b), di.fab(b), do.fab(b), 0, 1, ng, _wc(w)))
                            assert last_launch(ctx)[0] == 1, (b, last_launch(ctx))
                    ctx.sync()
                    got = do.download()
                what = f"ng {ng}, {lv.nboxes} boxes, {entry} entry"
                _assert_only_written(got, 0, 1, what)
                for b in range(lv.nboxes):
                    lo, hi = lv.boxes[b, :3], lv.boxes[b, 3:]
                    FC.assert_bits(got.valid(b)[0], want[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1], f"{what}: box {b} against the one dense result")


def test_last_launch_starts_empty_and_checks_its_arguments(ctx):
    c2 = capi.Context(0)
    try:
        assert last_launch(c2) == (0,) * 8
        assert c2.lib.pa_filter_last_launch(c2.h, None) != 0 and c2.lib.pa_filter_last_launch(None, (C.c_int32 * 8)()) != 0
    finally:
        c2.close()
