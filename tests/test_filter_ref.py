"""CPU tier: the independent numpy references of tests/filter_ref.py on every case of tests/filter_cases.py.

  tap_order   equals the oracle's orc_apply_filter bit for bit: the sum IS ((w_l w_m) w_n) q, n outermost, l innermost
  sep_model   (the separable kernel's documented operation order) is within the a-priori bound of the exact sum in every cell,
              and does not depend on how the cells are cut into boxes
and the references fail when they should, each time by the assertion meant for it.  The GPU tier
(tests/test_gpu_filter_shapes.py) then holds the kernels to these references."""
import ctypes as C

import numpy as np
import pytest

import filter_cases as FC
import filter_ref as R
from util import ref_out

IDS = [c.id for c in FC.CASES]


def _oracle_filter(oracle, case, w=None):
    """orc_apply_filter on the case's level, components COMPS: the oracle's output multifab"""
    lv, mf = FC.level(case), FC.input_mf(case)
    w = FC.weights(case.wname, case.ng)[1] if w is None else w
    oo = ref_out(lv, FC.NCOMP)
    src = mf.copy()  # the shared input is read-only
    oracle.lib().orc_apply_filter(C.byref(oracle._mf(src)), C.byref(oracle._mf(oo)), FC.COMPS[0], len(FC.COMPS), case.ng, (C.c_double * len(w))(*w))
    return oo


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_tap_order_is_the_oracle_bit_for_bit(oracle, case):
    oo = _oracle_filter(oracle, case)
    want = FC.ref_tap(case)
    for b in range(oo.level.nboxes):
        for c in FC.COMPS:
            assert np.isfinite(want[b][c]).all(), f"{case.id}: the reference read the NaN layer (box {b} comp {c})"
            FC.assert_bits(want[b][c], oo.valid(b)[c], f"{case.id} box {b} comp {c}: tap_order against orc_apply_filter")


@pytest.mark.parametrize("case", FC.CASES, ids=IDS)
def test_sep_model_within_bound_and_tiling_independent(case):
    tot_mag, model = FC.ref_exact(case), FC.ref_model(case)
    lv, g, ng = FC.level(case), case.ng_have, case.ng
    w = FC.weights(case.wname, ng)[1]
    dense = FC.dense(case)
    for b in range(lv.nboxes):
        for c in FC.COMPS:
            tot, mag = tot_mag[b][c]
            assert np.isfinite(model[b][c]).all() and (mag > 0).all()
            FC.assert_bound(model[b][c], tot, mag, ng, f"{case.id} box {b} comp {c}: sep_model against the exact sum")
    # the same cells as part of a larger box: the whole bounding box grown by one cell, out of the dense field (ng ghost layers left)
    big = {c: R.sep_model(np.ascontiguousarray(dense[c]), ng, ng, w) for c in FC.COMPS}
    for b in range(lv.nboxes):
        o = lv.boxes[b, :3] - lv.domlo + 1
        nz, ny, nx = lv.box_shape(b)
        for c in FC.COMPS:
            FC.assert_bits(model[b][c], big[c][o[2]:o[2] + nz, o[1]:o[1] + ny, o[0]:o[0] + nx], f"{case.id} box {b} comp {c}: sep_model of the box against the larger box")


def test_weights_are_the_oracles(oracle):
    for ng in (1, 2, 3, 4, 5, 6, 7, 8):
        ong, ow = oracle.box_filter_weights(2 * ng)
        n, w = FC.weights("box", ng)
        assert (n, ong) == (ng, ng) and np.array_equal(w.view(np.int64), ow.view(np.int64))
    for wname, ftype in FC.FILTER_TYPE.items():
        ong, ow = oracle.filter_weights(ftype, 4)
        n, w = FC.weights(wname, ong)
        assert n == ong and np.array_equal(w.view(np.int64), ow.view(np.int64)), wname
    n, w = FC.weights("tri", 4)
    assert n == 4 and w.sum() == 1.0 and np.array_equal(w, w[::-1]) and w[2] != w[1]  # symmetric, no box weights


def test_matrix_reaches_what_it_is_for():
    """the launches the suite never ran before this matrix, by the numbers the cases expect of pa_filter_last_launch"""
    sep = {c.id: c.sep for c in FC.CASES}
    exa = {c.id: c.exa for c in FC.CASES}
    for ng in (3, 6, 8):
        assert any(s[:3] == (1, ng, 1024) for s in sep.values()), f"1024 threads at ng {ng}"
        assert any(s[0] == 1 and s[1] == ng and s[6] > 1 for s in sep.values()), f"several z segments at ng {ng}"
    assert any(s[0] == 1 and s[4] > 1 and c.maxn[1] % s[3] for c in FC.CASES for s in [c.sep]), "a last y strip shorter than TY"
    assert any(s[0] == 1 and c.maxn[0] % 2 for c in FC.CASES for s in [c.sep]), "odd nx"
    assert sum(s[7] for s in sep.values()) >= 5 and all(s[0] != 1 for s in sep.values() if s[7]), "refused by the shape rule"
    assert {e[0] for e in exa.values()} == {2, 3, 4} and all(e[7] == 0 for e in exa.values())
    assert any(e[0] == 2 and e[6] == 3 for e in exa.values()), "streaming kernel, 3 z segments"
    assert any(e[:2] == (3, 4) for e in exa.values()), "LDS tile kernel at ng 4"
    assert max(int(np.prod(c.maxn)) for c in FC.CASES) < 75000 and all(c.sep[0] == 5 for c in FC.CASES_2D)


# ------------------------------------------------------------------------------------- the references fail when they should
def _case(cid):
    return next(c for c in FC.CASES if c.id == cid)


def test_wrong_end_weight_fails(oracle):
    """the end weights of the box filter not halved: tap_order no longer equals the oracle"""
    case = _case("b33x9x9-ng2-box")
    oo = _oracle_filter(oracle, case)
    w = FC.weights("box", 2)[1].copy()
    w[0] = w[-1] = w[1]
    got = R.tap_order(np.ascontiguousarray(FC.input_mf(case).fab(0)[0]), case.ng_have, 2, w)
    with pytest.raises(AssertionError, match="cells differ bit for bit"):
        FC.assert_bits(got, oo.valid(0)[0], "wrong end weight")


def test_swapped_loop_order_fails(oracle):
    """l outermost and n innermost: the same terms in another order are another double in most cells"""
    case = _case("b33x9x9-ng2-box")
    oo = _oracle_filter(oracle, case)
    f = np.ascontiguousarray(FC.input_mf(case).fab(0)[0])
    w = FC.weights("box", 2)[1]
    got = R.tap_order(f, case.ng_have, 2, w, order="lmn")
    assert rel_err_arrays(got, oo.valid(0)[0]) < 1e-14  # the same sum ...
    with pytest.raises(AssertionError, match="cells differ bit for bit"):  # ... not the same bits
        FC.assert_bits(got, oo.valid(0)[0], "swapped loop order")
    FC.assert_bits(R.tap_order(f, case.ng_have, 2, w), oo.valid(0)[0], "the intended order")


def rel_err_arrays(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def test_two_ulp_at_a_small_valued_cell_fails_the_bound():
    """2 ulp of the field's L-infinity added to the cell with the smallest M: 1e-12 * L-infinity (util.assert_filter_parity's
    bar) does not see it, the per-cell bound does"""
    case = _case("b33x9x9-ng1-box")
    tot, mag = FC.ref_exact(case)[0][0]
    got = FC.ref_model(case)[0][0].copy()
    FC.assert_bound(got, tot, mag, 1, "unperturbed")
    linf = float(np.abs(got).max())
    k, j, i = np.unravel_index(np.argmin(mag), mag.shape)
    assert float(mag[k, j, i]) < 1e-3 * linf, "the case has no small-valued cell"
    want = got.copy()
    got[k, j, i] += 2.0 * np.spacing(linf)
    assert np.abs(got - want).max() <= 1e-12 * linf
    with pytest.raises(AssertionError, match="outside the rounding bound"):
        FC.assert_bound(got, tot, mag, 1, "2 ulp of L-infinity at the smallest cell")
    # 2 ulp of a cell's OWN value where nothing has cancelled is within the bound: it is a rounding bound, not a bit comparison
    got = want.copy()
    ratio = np.abs(want) / mag.astype(np.float64)
    k, j, i = np.unravel_index(np.argmax(ratio), ratio.shape)  # |sum| ~ M: 2 ulp = at most 4 u |sum| <= 10 u M
    got[k, j, i] += 2.0 * np.spacing(got[k, j, i])
    FC.assert_bound(got, tot, mag, 1, "2 ulp of a cell without cancellation")
