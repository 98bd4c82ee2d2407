"""The fused sweep's z segments at the lengths where its peeled prologue takes another path (pa_fused_march3.h, pa_fused_march3n.h):
an output row runs three store-free warm-up steps, then ONE peeled group of three storing steps, then the loop, then up to two
remainder steps.  A segment of n planes has n + 2 steps:

    n = 3  warm-up + remainder (2)          n = 6  ... + peeled group + remainder (2)
    n = 4  warm-up + peeled group           n = 7  first loop trip
    n = 5  ... + remainder (1)              n = 8  first loop trip + remainder (1)

and nz = 73 / 74 are cut by the launcher's model into eight segments of 9 planes and a last one of 1 / 2 planes (the warm-up with
nothing to store before the epilogue; the warm-up plus one remainder step).  One box per level of 64 x 52 (tiles of 13 rows),
64 x 16 (8 rows) and 32 x 16 cells (the narrow-box kernel), with a wall in z (special z faces: the compact ghost arrays), periodic
in z, and as a fine level inside a coarse one (coarse-fine z faces); through pa_gradcurv_run without and with a threshold,
pa_curvature_run without and with do_gauss, and (the periodic box) pa_gradcurv_fab.  Everything against the oracle bit for bit,
outputs starting as NaN sentinels: a plane the kernel no longer stores shows up as "never written by the kernel"."""
import numpy as np
import pytest

from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, field_flame
from util import assert_valid_bits_equal, make_states, ref_out, sentinel_out

pytestmark = pytest.mark.gpu

THR = 0.05
NZS = [3, 4, 5, 6, 7, 8, 73, 74]
SHAPES = [(64, 52), (64, 16), (32, 16)]
KINDS = ["wall_z", "periodic_z", "fine_level"]
NC = [(4, 2), (5, 3), (6, 4), (7, 1)]  # pa_gradcurv_run's N, K <- the oracle's curvature components


def _hierarchy(nx, ny, nz, kind):
    z3, o3 = np.zeros(3), np.ones(3)
    if kind != "fine_level":
        per = (1, 1, 0) if kind == "wall_z" else (1, 1, 1)
        hi = (nx - 1, ny - 1, nz - 1)
        return Hierarchy([Level(np.array([[0, 0, 0, *hi]], np.int32), (0, 0, 0), hi, per, z3, o3)], 2), per
    per = (1, 1, 0)
    # the fine box starts 8 coarse cells inside the coarse one in every direction and ends at least 4 coarse cells before its far side
    chi = (nx // 2 + 15, ny // 2 + 15, (nz + 1) // 2 + 15)
    l0 = Level(np.array([[0, 0, 0, *chi]], np.int32), (0, 0, 0), chi, per, z3, o3)
    fhi = tuple(2 * c + 1 for c in chi)
    l1 = Level(np.array([[16, 16, 16, 16 + nx - 1, 16 + ny - 1, 16 + nz - 1]], np.int32), (0, 0, 0), fhi, per, z3, o3)
    return Hierarchy([l0, l1], 2), per


def _oracle_outputs(oracle, H, states, bc):
    og = [ref_out(lv, 4) for lv in H.levels]
    oracle.grad_pipeline(H.levels, [s.copy() for s in states], 0, bc, og, 0, multipass=False)
    oc = [ref_out(lv, 5) for lv in H.levels]
    oracle.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, oc, 0, MultiFab)
    oct_ = [ref_out(lv, 5) for lv in H.levels]
    oracle.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, oct_, 0, MultiFab, threshold=THR)
    okg = [ref_out(lv, 6) for lv in H.levels]
    oracle.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, okg, 0, MultiFab, threshold=THR, do_gauss=True)
    return og, oc, oct_, okg


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nz", NZS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_short_segments_match_oracle(ctx, oracle, nx, ny, nz, kind):
    H, per = _hierarchy(nx, ny, nz, kind)
    what = f"{nx}x{ny}x{nz} {kind}"
    states = make_states(H, 1, 2, field_flame, seed=101 + nz)
    bc = capi.bc_from_flags(per)
    og, oc, oct_, okg = _oracle_outputs(oracle, H, states, bc)
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    dst = [capi.DevMF.from_host(ctx, dl, s) for dl, s in zip(dls, states)]
    work = [capi.DevMF(ctx, dl, 1, 2) for dl in dls]

    # pa_gradcurv_run: the fused pass, without and with the threshold clip
    for thr, ocx in ((None, oc), (THR, oct_)):
        dout = [sentinel_out(ctx, dl, 8) for dl in dls]
        capi.gradcurv_run(ctx, dst, 0, bc, capi.curv_params(threshold=thr, fused=True), work, dout, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        kn = ctx.lib.pa_sweep_kernel_name(ctx.h).decode()
        assert "k_gradcurv_march3" in kn, kn  # a marching sweep ran, not the pass-by-pass kernels
        assert ("march3n" in kn) == (nx <= 32), kn  # (the coarse box of the fine-level case is 48 or 32 cells wide: the same kernel family)
        for l in range(H.nlev):
            got = dout[l].download()
            assert_valid_bits_equal(got, og[l], [(c, c) for c in range(4)], f"{what}: pa_gradcurv_run thr {thr}, grad level {l}")
            assert_valid_bits_equal(got, ocx[l], NC, f"{what}: pa_gradcurv_run thr {thr}, curv level {l}")

    # pa_curvature_run: the G-output sweeps, without do_gauss and with it (+ the clip)
    d5 = [sentinel_out(ctx, dl, 5) for dl in dls]
    capi.curvature_run(ctx, dst, 0, bc, capi.curv_params(fused=True), d5, 0)
    ctx.sync()
    assert ctx.bc_errors() == 0
    for l in range(H.nlev):
        assert_valid_bits_equal(d5[l].download(), oc[l], [(c, c) for c in range(5)], f"{what}: pa_curvature_run level {l}")
    d6 = [sentinel_out(ctx, dl, 6) for dl in dls]
    capi.curvature_run(ctx, dst, 0, bc, capi.curv_params(threshold=THR, fused=True, do_gauss=True), d6, 0)
    ctx.sync()
    assert ctx.bc_errors() == 0
    for l in range(H.nlev):
        assert_valid_bits_equal(d6[l].download(), okg[l], [(c, c) for c in range(6)], f"{what}: pa_curvature_run do_gauss level {l}")

    # pa_gradcurv_fab (per FAB, ghost cells as they are): the periodic box, whose filled ghost cells are the level's own data
    if kind == "periodic_z":
        lv = H.levels[0]
        st = states[0].copy()
        oracle.fill_boundary(st, 0, 1, 2)
        pmin, pmax = oracle.minmax(states[0], 0)
        dphi = capi.DevMF.from_host(ctx, dls[0], st)
        dxinv = capi._d3(1.0 / lv.dx)
        for thr, ocx in ((-1.0, oc), (THR, oct_)):
            dfo = sentinel_out(ctx, dls[0], 8)
            ctx.check(ctx.lib.pa_gradcurv_fab(ctx.h, capi.box_of(lv, 0), dphi.fab(0), 0, pmin, pmax, dxinv, thr, dfo.fab(0), 0))
            ctx.sync()
            got = dfo.download()
            assert_valid_bits_equal(got, og[0], [(c, c) for c in range(4)], f"{what}: pa_gradcurv_fab thr {thr}, grad")
            assert_valid_bits_equal(got, ocx[0], NC, f"{what}: pa_gradcurv_fab thr {thr}, curv")
