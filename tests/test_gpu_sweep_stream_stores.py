"""The marching kernels' output stores are streaming stores (`global_store_dwordx2 ... nt`: pa_fused_march3.h, pa_fused_march3n.h,
pa_grad_march.h): the 8-store burst of the fused sweep, the G-output sweeps' stores of G and the gradient sweep's 4 stores.  The
values, the addresses and the order of the stores are what they were, so every output is the oracle's, bit for bit, on

    two_level   coarse boxes of 64 x 26 x 8 and 64 x 27 x 8 (8-row tiles: last tiles of 2 and 3 rows, one x tile) under a fine box of
                64 x 64 x 16 that straddles them (13-row tiles, a last tile of 12 rows)
    tall_1row   one box of 64 x 53 x 8: 13-row tiles with a last tile of ONE row
    periodic    one periodic box of 128 x 39 x 6: two x tiles by five row tiles, halo rows and columns shared both ways
    narrow      three nested levels of 32^3 boxes: the narrow-box kernel

through pa_gradcurv_run (without and with the threshold clip), pa_grad_run and pa_curvature_run with do_gauss (the stores of G).
Outputs start as NaN sentinels.  A pass repeated onto the SAME outputs, with nothing re-poisoned in between, must give the same
bits again: a streaming store must not leave an older line behind for a later reader."""
import numpy as np
import pytest

from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, field_flame, nested_hierarchy
from util import assert_valid_bits_equal, bits_equal, make_states, ref_out, sentinel_out

pytestmark = pytest.mark.gpu

THR = 0.05
NC = [(4, 2), (5, 3), (6, 4), (7, 1)]  # pa_gradcurv_run's N, K <- the oracle's curvature components
NAMES = ["two_level", "tall_1row", "periodic", "narrow"]


def _hierarchy(name):
    z3, o3 = np.zeros(3), np.ones(3)
    if name == "two_level":
        per = (1, 1, 0)
        l0 = Level(np.array([[0, 0, 0, 63, 25, 7], [0, 26, 0, 63, 52, 7]], np.int32), (0, 0, 0), (63, 52, 7), per, z3, o3)
        # coarse cells 16..47 x 10..41 x 0..7: across the seam of the two coarse boxes at j = 26, wall to wall in z
        l1 = Level(np.array([[32, 20, 0, 95, 83, 15]], np.int32), (0, 0, 0), (127, 105, 15), per, z3, o3)
        return Hierarchy([l0, l1], 2), per
    if name == "tall_1row":
        per = (1, 1, 0)
        return Hierarchy([Level(np.array([[0, 0, 0, 63, 52, 7]], np.int32), (0, 0, 0), (63, 52, 7), per, z3, o3)], 2), per
    if name == "periodic":
        per = (1, 1, 1)
        return Hierarchy([Level(np.array([[0, 0, 0, 127, 38, 5]], np.int32), (0, 0, 0), (127, 38, 5), per, z3, o3)], 2), per
    per = (1, 1, 0)
    return nested_hierarchy(64, 3, 32, is_per=per), per


_CASES = {}


def _case(oracle, name):
    """hierarchy, states and the oracle's outputs: computed once per hierarchy, shared by the tests, never modified"""
    if name not in _CASES:
        H, per = _hierarchy(name)
        states = make_states(H, 1, 2, field_flame, seed=1501)
        bc = capi.bc_from_flags(per)
        og = [ref_out(lv, 4) for lv in H.levels]
        oracle.grad_pipeline(H.levels, [s.copy() for s in states], 0, bc, og, 0, multipass=False)
        oc = [ref_out(lv, 5) for lv in H.levels]
        oracle.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, oc, 0, MultiFab)
        oct_ = [ref_out(lv, 5) for lv in H.levels]
        oracle.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, oct_, 0, MultiFab, threshold=THR)
        okg = [ref_out(lv, 6) for lv in H.levels]
        oracle.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, okg, 0, MultiFab, threshold=THR, do_gauss=True)
        _CASES[name] = (H, states, bc, og, oc, oct_, okg)
    return _CASES[name]


def _dev(ctx, H, states):
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    return dls, [capi.DevMF.from_host(ctx, dl, s) for dl, s in zip(dls, states)]


@pytest.mark.parametrize("name", NAMES)
def test_gradcurv_run_matches_oracle(ctx, oracle, name):
    H, states, bc, og, oc, oct_, _ = _case(oracle, name)
    dls, dst = _dev(ctx, H, states)
    work = [capi.DevMF(ctx, dl, 1, 2) for dl in dls]
    for thr, ocx in ((None, oc), (THR, oct_)):
        dout = [sentinel_out(ctx, dl, 8) for dl in dls]
        capi.gradcurv_run(ctx, dst, 0, bc, capi.curv_params(threshold=thr, fused=True), work, dout, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        kn = ctx.lib.pa_sweep_kernel_name(ctx.h).decode()
        assert "k_gradcurv_march3" in kn, kn  # a marching sweep ran, not the pass-by-pass kernels
        assert ("march3n" in kn) == (name == "narrow"), kn
        for l in range(H.nlev):
            got = dout[l].download()
            assert_valid_bits_equal(got, og[l], [(c, c) for c in range(4)], f"{name}: pa_gradcurv_run thr {thr}, grad level {l}")
            assert_valid_bits_equal(got, ocx[l], NC, f"{name}: pa_gradcurv_run thr {thr}, curv level {l}")


@pytest.mark.parametrize("name", NAMES)
def test_grad_run_matches_oracle(ctx, oracle, name):
    H, states, bc, og = _case(oracle, name)[:4]
    dls, dst = _dev(ctx, H, states)
    d4 = [sentinel_out(ctx, dl, 4) for dl in dls]
    capi.grad_run(ctx, dst, 0, bc, d4, 0)
    ctx.sync()
    for l in range(H.nlev):
        assert_valid_bits_equal(d4[l].download(), og[l], [(c, c) for c in range(4)], f"{name}: pa_grad_run level {l}")


@pytest.mark.parametrize("name", NAMES)
def test_curvature_run_do_gauss_matches_oracle(ctx, oracle, name):
    H, states, bc = _case(oracle, name)[:3]
    okg = _case(oracle, name)[6]
    dls, dst = _dev(ctx, H, states)
    d6 = [sentinel_out(ctx, dl, 6) for dl in dls]
    capi.curvature_run(ctx, dst, 0, bc, capi.curv_params(threshold=THR, fused=True, do_gauss=True), d6, 0)
    ctx.sync()
    assert ctx.bc_errors() == 0
    for l in range(H.nlev):
        assert_valid_bits_equal(d6[l].download(), okg[l], [(c, c) for c in range(6)], f"{name}: pa_curvature_run do_gauss level {l}")


def test_second_pass_onto_the_same_outputs_gives_the_same_bits(ctx, oracle):
    """two_level (both tile heights, a coarse-fine boundary): every pass twice onto one set of outputs, nothing re-poisoned"""
    H, states, bc, og, oc, _, okg = _case(oracle, "two_level")
    dls, dst = _dev(ctx, H, states)
    work = [capi.DevMF(ctx, dl, 1, 2) for dl in dls]
    d8 = [sentinel_out(ctx, dl, 8) for dl in dls]
    d4 = [sentinel_out(ctx, dl, 4) for dl in dls]
    d6 = [sentinel_out(ctx, dl, 6) for dl in dls]
    first = None
    for rep in range(2):
        capi.gradcurv_run(ctx, dst, 0, bc, capi.curv_params(fused=True), work, d8, 0)
        capi.grad_run(ctx, dst, 0, bc, d4, 0)
        capi.curvature_run(ctx, dst, 0, bc, capi.curv_params(threshold=THR, fused=True, do_gauss=True), d6, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        got = [[d[l].download() for l in range(H.nlev)] for d in (d8, d4, d6)]
        for l in range(H.nlev):
            assert_valid_bits_equal(got[0][l], og[l], [(c, c) for c in range(4)], f"pass {rep}: pa_gradcurv_run grad level {l}")
            assert_valid_bits_equal(got[0][l], oc[l], NC, f"pass {rep}: pa_gradcurv_run curv level {l}")
            assert_valid_bits_equal(got[1][l], og[l], [(c, c) for c in range(4)], f"pass {rep}: pa_grad_run level {l}")
            assert_valid_bits_equal(got[2][l], okg[l], [(c, c) for c in range(6)], f"pass {rep}: pa_curvature_run do_gauss level {l}")
        if first is None:
            first = got
        else:  # the whole allocation, padding and all: the second pass changed no bit anywhere
            for a, b in zip(first, got):
                for l in range(H.nlev):
                    assert bits_equal(a[l].data, b[l].data), f"level {l}: the second pass left other bits than the first"
