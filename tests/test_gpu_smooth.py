"""GPU parity: do_smooth (curvature.cpp:328-406) -- pa_smooth_solve vs the oracle's composite solve.
An iterative solve to a tolerance: GPU and oracle run the same algorithm with different summation
orders, so the comparison is to a stated tolerance: 1e-12 absolute on a field in [0,1] (= north_star's 1e-12 relative
to the field's scale) with both sides iterated to a residual of 1e-14 (cond(I - dt Lap) ~ 25 here), plus the
solver-independent checks (exact discrete eigenmode, residual of the GPU
solution under the ORACLE's operator)."""
import numpy as np
import pytest

from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import MultiFab, Level, chop_box, nested_hierarchy, fill_analytic, field_flame
from util import assert_no_sentinel, assert_untouched, ref_out, sentinel_out

pytestmark = pytest.mark.gpu


def _solve_gpu(ctx, levels, rhs, dt, bc, tol):
    dls = [capi.DevLevel(ctx, lv) for lv in levels]
    drhs = [capi.DevMF.from_host(ctx, dl, r) for dl, r in zip(dls, rhs)]
    dsol = [sentinel_out(ctx, dl, 1) for dl in dls]
    it, res = capi.smooth_solve(ctx, drhs, 0, dsol, 0, dt, bc, tol=tol, maxiter=200)
    return _written([d.download() for d in dsol]), it, res


def _written(sol):
    """the solution multifabs started as SENT_GPU: every valid cell was stored, with a finite value (the comparisons that follow are to a
    tolerance, which a NaN would fail only by the accident of `<=`)"""
    for l, m in enumerate(sol):
        assert_no_sentinel(m, [0], f"pa_smooth_solve, level {l}")
        assert np.isfinite(m.valid_concat(0)).all(), f"pa_smooth_solve, level {l}: non-finite values"
    return sol


def test_smooth_single_level_eigenmode(ctx):
    n = 32
    lv = Level(chop_box((0, 0, 0), (n - 1,) * 3, 16), (0, 0, 0), (n - 1,) * 3, (1, 1, 1), (0, 0, 0), (1, 1, 1))
    rhs = MultiFab(lv, 1, 0)
    kx, ky, kz = 3, 1, 2
    fill_analytic(rhs, 0, lambda x, y, z: 0.5 + 0.25 * np.sin(2 * np.pi * kx * x) * np.cos(2 * np.pi * ky * y) * np.sin(2 * np.pi * kz * z + 0.3))
    dt, h = 2e-3, 1.0 / n
    sol, it, res = _solve_gpu(ctx, [lv], [rhs], dt, (0, 0, 0), 1e-14)
    assert 0 < it < 60 and res <= 1e-14
    lam = sum((2 - 2 * np.cos(2 * np.pi * k * h)) / h ** 2 for k in (kx, ky, kz))
    for b in range(lv.nboxes):
        assert np.abs(sol[0].valid(b)[0] - (0.5 + (rhs.valid(b)[0] - 0.5) / (1 + dt * lam))).max() < 1e-13


@pytest.mark.parametrize("per", [(1, 1, 0), (0, 0, 0)])
def test_smooth_composite_matches_oracle(ctx, oracle, per):
    H = nested_hierarchy(16, 3, 8, is_per=per)
    rhs = []
    for lv in H.levels:
        m = MultiFab(lv, 1, 0)
        fill_analytic(m, 0, lambda x, y, z: (field_flame(x, y, z, 0) - 300.0) / 1700.0)
        rhs.append(m)
    bc = capi.bc_from_flags(per)
    dt = 5e-4
    want, oit, ores = oracle.smooth_solve(H.levels, rhs, 0, dt, bc, MultiFab, tol=1e-14)
    got, it, res = _solve_gpu(ctx, H.levels, rhs, dt, bc, 1e-14)
    assert 0 < it < 100 and res <= 1e-14 and abs(it - oit) <= 3
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            assert np.abs(got[l].valid(b)[0] - want[l].valid(b)[0]).max() <= 1e-12, (l, b)
    # the GPU solution under the oracle's composite operator
    x = [MultiFab(lv, 1, 1) for lv in H.levels]
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            x[l].valid(b)[0] = got[l].valid(b)[0]
    y, mask = oracle.smooth_apply(H.levels, x, dt, bc, MultiFab)
    r = max(float(np.abs((y[l].valid(b)[0] - rhs[l].valid(b)[0]) * mask[l].valid(b)[0]).max()) for l, lv in enumerate(H.levels) for b in range(lv.nboxes))
    assert r <= 1e-12


@pytest.mark.parametrize("per,sym", [((1, 1, 0), (0, 0, 0)), ((0, 1, 0), (1, 0, 1))])
def test_curvature_run_with_smoothing(ctx, oracle, per, sym):
    """the tool path: Progress stays unsmoothed, SmoothedProgress feeds the curvature (idprogvar, :408).  With sym_dir set
    the gradient operators see reflect_odd walls but the smoothing operator stays Neumann (curvature.cpp:348-357)."""
    from util import make_states
    H = nested_hierarchy(16, 3, 8, is_per=per)
    states = make_states(H, 1, 2, field_flame, seed=41)
    bc = capi.bc_from_flags(per, sym)
    dt = 1e-3
    oout = [ref_out(lv, 18) for lv in H.levels]
    oracle.curvature_pipeline(H.levels, [s.copy() for s in states], 0, bc, oout, 0, MultiFab, do_smooth=True, smoothing_time=dt, smooth_tol=1e-14)
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    dst = [capi.DevMF.from_host(ctx, dl, s) for dl, s in zip(dls, states)]
    dout = [sentinel_out(ctx, dl, 18) for dl in dls]
    capi.curvature_run(ctx, dst, 0, bc, capi.curv_params(fused=False, do_smooth=True, smoothing_time=dt), dout, 0)
    ctx.sync()
    assert ctx.lib.pa_curvature_last_path(ctx.h) == 0
    # the same solve feeding the exact-normal pipeline (fused=True: the smoothed field as a progress source of range [0, 1], which the
    # sweeps' (x - pmin) * invdenom leaves bit for bit): every output, options included, equals the pass-by-pass path's bits
    st4 = make_states(H, 4, 2, field_flame, seed=41)
    dst4 = [capi.DevMF.from_host(ctx, dl, s) for dl, s in zip(dls, st4)]
    both = []
    for fused in (False, True):
        o = [sentinel_out(ctx, dl, 18) for dl in dls]
        capi.curvature_run(ctx, dst4, 0, bc, capi.curv_params(threshold=0.04, fused=fused, do_smooth=True, smoothing_time=dt, do_gauss=True, do_strain=True,
                                                             strain_tensor=True, do_velnormal=True, vel_comp=1), o, 0)
        ctx.sync()
        assert ctx.lib.pa_curvature_last_path(ctx.h) == (1 if fused else 0)
        both.append([m.download() for m in o])
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            assert np.array_equal(both[0][l].valid(b).view(np.int64), both[1][l].valid(b).view(np.int64)), f"do_smooth + options: fast path != pass by pass, level {l} box {b}"
        for m in (both[0][l], both[1][l]):  # equal bits are no proof that either path stored them
            assert_no_sentinel(m, range(18), f"do_smooth + options, level {l}")
    for l, lv in enumerate(H.levels):
        g = dout[l].download()
        assert_no_sentinel(g, [0, 1, 2, 3, 4, 17], f"do_smooth, level {l} (kernel output)")
        assert_no_sentinel(oout[l], [0, 1, 2, 3, 4, 17], f"do_smooth, level {l} (oracle output)")
        assert_untouched(g, range(6, 17), f"do_smooth without options: their components, level {l}")
        for b in range(lv.nboxes):
            gv, wv = g.valid(b), oout[l].valid(b)
            assert np.array_equal(gv[0].view(np.int64), wv[0].view(np.int64)), "Progress (unsmoothed) must stay bit-identical"
            assert np.abs(gv[17] - wv[17]).max() <= 1e-12, "SmoothedProgress"
            assert not np.array_equal(gv[17], gv[0])
            # Downstream fields.  n = -G / |G| and K = 0.5 div n amplify a difference eps in the smoothed field by 1 / |G|; the
            # tolerance is DERIVED from the measured eps, not chosen.  Cells whose stencil stays inside the box (no ghost cell):
            #   G_d = 0.5 dxinv_d (c[+1] - c[-1])            =>  |dG_d| <= dxinv_d eps,  ||dG||_2 <= eps S,  S = sqrt(sum dxinv_d^2)
            #   n = G / |G|:  |a/|a| - b/|b|| <= 2 |a - b| / max(|a|, |b|)   =>  ||dn||_inf <= 2 eps S / |G|
            #   K = 0.5 sum_d 0.5 dxinv_d (n_d[+1] - n_d[-1])                =>  |dK| <= 0.5 (sum_d dxinv_d) max_neighbours ||dn||_inf
            # (+ a few ulp of the fields' own rounding).  Where |G| <= 1e-14 the reference clamps it: not compared.
            eps = float(np.abs(gv[17] - wv[17]).max())
            dxinv = 1.0 / np.asarray(lv.dx)
            S, S1 = float(np.sqrt((dxinv ** 2).sum())), float(dxinv.sum())
            cs = wv[17]
            Gz, Gy, Gx = [0.5 * dxinv[d] * (np.roll(cs, -1, axis=2 - d) - np.roll(cs, 1, axis=2 - d)) for d in (2, 1, 0)]
            Gm = np.sqrt(Gx ** 2 + Gy ** 2 + Gz ** 2)
            inner = np.zeros(cs.shape, bool)
            inner[1:-1, 1:-1, 1:-1] = True  # np.roll wrapped at the box faces: those cells use ghost data, not bounded here
            ok = inner & (Gm > 1e-6)
            dn_bound = np.where(ok, 2.0 * eps * S / np.maximum(Gm - eps * S, 1e-300) + 8e-16, np.inf)
            for c in (2, 3, 4):
                d = np.abs(gv[c] - wv[c])
                assert np.all(d[ok] <= dn_bound[ok]), (l, b, c, float((d[ok] / dn_bound[ok]).max()))
            nb = dn_bound.copy()  # the bound of a cell's six neighbours and its own
            for ax in range(3):
                nb = np.maximum(nb, np.maximum(np.roll(dn_bound, 1, axis=ax), np.roll(dn_bound, -1, axis=ax)))
            inner2 = np.zeros(cs.shape, bool)
            inner2[2:-2, 2:-2, 2:-2] = True
            okk = inner2 & np.isfinite(nb)
            dk = np.abs(gv[1] - wv[1])
            kb = 0.5 * S1 * nb + 1e-13 * max(1.0, float(np.abs(wv[1]).max()))
            assert np.all(dk[okk] <= kb[okk]), (l, b, float((dk[okk] / kb[okk]).max()))
    # EVERY cell (box faces with their coarse-fine / wall ghost data, the flat parts of the profile), without a tolerance: the
    # downstream fields are a function f of the smoothed field, and f on the HIP path is the reference's f BIT FOR BIT -- the ORACLE's
    # smoothed field handed to the HIP pipeline as a progress variable of range [0, 1] ((c - 0.0) * 1.0 = c exactly) gives the
    # oracle's normals and curvature in every cell.  What separates the two runs above is therefore the solve's eps alone
    # (<= 1e-12, iterative on both sides -- MLMG's in the reference), amplified by the conditioning of f: the bounds above.
    sm = []
    for l, lv in enumerate(H.levels):
        m = MultiFab(lv, 1, 2)
        for b in range(lv.nboxes):
            m.valid(b)[0] = oout[l].valid(b)[17]
        sm.append(m)
    dsm = [capi.DevMF.from_host(ctx, dl, m) for dl, m in zip(dls, sm)]
    for fused in (False, True):
        o = [sentinel_out(ctx, dl, 18) for dl in dls]
        capi.curvature_run(ctx, dsm, 0, bc, capi.curv_params(prog_min=0.0, prog_max=1.0, fused=fused), o, 0)
        ctx.sync()
        for l, lv in enumerate(H.levels):
            g = o[l].download()
            for b in range(lv.nboxes):
                gv, wv = g.valid(b), oout[l].valid(b)
                assert np.array_equal(gv[0].view(np.int64), wv[17].view(np.int64))
                for c in (1, 2, 3, 4):
                    assert np.array_equal(gv[c].view(np.int64), wv[c].view(np.int64)), f"f(oracle's smoothed field), fused={fused}: level {l} box {b} comp {c}"


def _hier2d(per):
    from peleanalysis_amd.hierarchy import Hierarchy
    per3 = np.array([per[0], per[1], 0])
    l0 = Level(chop_box((0, 0, 0), (31, 31, 0), 16), (0, 0, 0), (31, 31, 0), per3, np.zeros(3), np.ones(3))
    l1 = Level(chop_box((16, 16, 0), (47, 47, 0), 16), (0, 0, 0), (63, 63, 0), per3, np.zeros(3), np.ones(3))
    return Hierarchy([l0, l1], 2)


@pytest.mark.parametrize("per", [(1, 0), (0, 0)])
def test_smooth_2d_composite_matches_oracle(ctx, oracle, per):
    """the AMREX_SPACEDIM == 2 build of do_smooth: one plane of cells per level, refined in x and y only (covered blocks
    of 2 x 2, two fine faces per coarse face in the reflux), z a Neumann wall"""
    H = _hier2d(per)
    rhs = []
    for lv in H.levels:
        m = MultiFab(lv, 1, 0)
        fill_analytic(m, 0, lambda x, y, z: 0.5 * (1.0 + np.tanh((np.hypot(x - 0.5, (y - 0.5) / 0.8) - 0.27) / 0.06)) + 0 * z)
        rhs.append(m)
    bc = capi.bc_from_flags((per[0], per[1], 0))
    dt = 4e-4
    want, oit, ores = oracle.smooth_solve(H.levels, rhs, 0, dt, bc, MultiFab, tol=1e-14)
    got, it, res = _solve_gpu(ctx, H.levels, rhs, dt, bc, 1e-14)
    assert 0 < it < 100 and res <= 1e-14 and abs(it - oit) <= 3
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            assert np.abs(got[l].valid(b)[0] - want[l].valid(b)[0]).max() <= 1e-12, (l, b)
    x = [MultiFab(lv, 1, 1) for lv in H.levels]
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            x[l].valid(b)[0] = got[l].valid(b)[0]
    y, mask = oracle.smooth_apply(H.levels, x, dt, bc, MultiFab)
    r = max(float(np.abs((y[l].valid(b)[0] - rhs[l].valid(b)[0]) * mask[l].valid(b)[0]).max()) for l, lv in enumerate(H.levels) for b in range(lv.nboxes))
    assert r <= 1e-12


def test_smooth_2d_single_level_eigenmode(ctx):
    n = 64
    lv = Level(chop_box((0, 0, 0), (n - 1, n - 1, 0), 32), (0, 0, 0), (n - 1, n - 1, 0), (1, 1, 0), (0, 0, 0), (1, 1, 1))
    rhs = MultiFab(lv, 1, 0)
    kx, ky = 3, 5
    fill_analytic(rhs, 0, lambda x, y, z: 0.5 + 0.25 * np.sin(2 * np.pi * kx * x + 0.1) * np.cos(2 * np.pi * ky * y) + 0 * z)
    dt, h = 5e-4, 1.0 / n
    sol, it, res = _solve_gpu(ctx, [lv], [rhs], dt, capi.bc_from_flags((1, 1, 0)), 1e-14)
    assert 0 < it < 60 and res <= 1e-14
    lam = sum((2 - 2 * np.cos(2 * np.pi * k * h)) / h ** 2 for k in (kx, ky))
    for b in range(lv.nboxes):
        assert np.abs(sol[0].valid(b)[0] - (0.5 + (rhs.valid(b)[0] - 0.5) / (1 + dt * lam))).max() < 1e-13


def test_smooth_and_stream_reject_bad_input(ctx):
    """host-side shape checks before any kernel runs: misaligned fine boxes, component ranges, ghost widths"""
    import ctypes as C
    from peleanalysis_amd.hierarchy import Hierarchy
    l0 = Level(chop_box((0, 0, 0), (15, 15, 15), 8), (0, 0, 0), (15, 15, 15), (1, 1, 1), (0, 0, 0), (1, 1, 1))
    l1 = Level(np.array([[9, 8, 8, 18, 23, 23]], dtype=np.int32), (0, 0, 0), (31, 31, 31), (1, 1, 1), (0, 0, 0), (1, 1, 1))  # odd lo: not ratio-aligned
    dls = [capi.DevLevel(ctx, l0), capi.DevLevel(ctx, l1)]
    rhs = [capi.DevMF(ctx, dl, 1, 0) for dl in dls]  # inputs of calls that are refused before any launch: never read
    sol = [capi.DevMF(ctx, dl, 1, 0) for dl in dls]  # never written
    with pytest.raises(capi.PaError, match="aligned"):
        capi.smooth_solve(ctx, rhs, 0, sol, 0, 1e-3, (0, 0, 0))
    with pytest.raises(capi.PaError, match="component"):
        capi.smooth_solve(ctx, rhs[:1], 3, sol[:1], 0, 1e-3, (0, 0, 0))
    v = [capi.DevMF(ctx, dls[0], 3, 0)]  # input (refused): no ghost layers
    with pytest.raises(capi.PaError, match="nGrow"):
        capi.stream_trace(ctx, v, 0, np.array([[0.5, 0.5, 0.5]]), 5, 0.01)
    v = [capi.DevMF(ctx, dls[0], 2, 2)]  # too few components
    with pytest.raises(capi.PaError, match="component"):
        capi.stream_trace(ctx, v, 0, np.array([[0.5, 0.5, 0.5]]), 5, 0.01)
    pos, nred = capi.stream_trace(ctx, [capi.DevMF(ctx, dls[0], 3, 2)], 0, np.zeros((0, 3)), 5, 0.01)  # no seeds: nothing to do
    assert pos.shape == (0, 5, 3) and nred == 0


@pytest.mark.parametrize("per,base,box", [((1, 1, 0), 16, 8), ((0, 0, 0), 32, 16), ((1, 1, 0), 12, 6)])  # 6-cell boxes: level 0 cannot be coarsened, more steps on it
def test_smooth_multigrid_preconditioner(ctx, oracle, per, base, box, monkeypatch):
    """a STIFF smoothing step (dt / dx^2 = 100 on the finest level: what smoothing_time = 1e-7 is for a plotfile in physical units):
    BiCGStab with the V-cycle preconditioner (default there; PA_SMOOTH_MG=1) reaches the tolerance in a fraction of the iterations of the
    unpreconditioned solve (PA_SMOOTH_MG=0), both fields agree with each other and with the oracle's unpreconditioned solve to the
    solve's tolerance times the condition number, and the preconditioned field has a small residual under the ORACLE's operator"""
    H = nested_hierarchy(base, 3, box, is_per=per)
    rhs = []
    for lv in H.levels:
        m = MultiFab(lv, 1, 0)
        fill_analytic(m, 0, lambda x, y, z: (field_flame(x, y, z, 0) - 300.0) / 1700.0)
        rhs.append(m)
    bc = capi.bc_from_flags(per)
    nf = base * 4
    dt = 100.0 / nf ** 2
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    drhs = [capi.DevMF.from_host(ctx, dl, r) for dl, r in zip(dls, rhs)]
    out = {}
    for mg in ("0", "1", ""):
        if mg:
            monkeypatch.setenv("PA_SMOOTH_MG", mg)
        else:
            monkeypatch.delenv("PA_SMOOTH_MG")
        capi.reload_options()
        dsol = [sentinel_out(ctx, dl, 1) for dl in dls]
        it, res = capi.smooth_solve(ctx, drhs, 0, dsol, 0, dt, bc, tol=1e-13, maxiter=2000)
        assert res <= 1e-13
        out[mg] = (_written([d.download() for d in dsol]), it)
    assert out["1"][1] == out[""][1], "dt / dx^2 = 100: the preconditioner is the default"
    # pa_curvature_run iterates to 1e-14 (and accepts 1e-12): the preconditioned recurrence gets there too, in a handful of iterations
    dsol = [sentinel_out(ctx, dl, 1) for dl in dls]
    it14, res14 = capi.smooth_solve(ctx, drhs, 0, dsol, 0, dt, bc, tol=1e-14, maxiter=100)
    assert res14 <= 1e-14 and it14 <= out["1"][1] + 6, (it14, res14)
    assert out["1"][1] * 3 <= out["0"][1], f"iterations: preconditioned {out['1'][1]}, plain {out['0'][1]}"
    want, oit, ores = oracle.smooth_solve(H.levels, rhs, 0, dt, bc, MultiFab, tol=1e-13, maxiter=2000)
    assert ores <= 1e-13
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            assert np.abs(out["1"][0][l].valid(b)[0] - out["0"][0][l].valid(b)[0]).max() <= 1e-10, (l, b)
            assert np.abs(out["1"][0][l].valid(b)[0] - want[l].valid(b)[0]).max() <= 1e-10, (l, b)
    x = [MultiFab(lv, 1, 1) for lv in H.levels]
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            x[l].valid(b)[0] = out["1"][0][l].valid(b)[0]
    y, mask = oracle.smooth_apply(H.levels, x, dt, bc, MultiFab)
    r = max(float(np.abs((y[l].valid(b)[0] - rhs[l].valid(b)[0]) * mask[l].valid(b)[0]).max()) for l, lv in enumerate(H.levels) for b in range(lv.nboxes))
    assert r <= 1e-11


@pytest.mark.parametrize("base", [80, 46])
@pytest.mark.parametrize("dtq", [2.0, 20.0])  # dt / dx^2 on the finest level: the plain iteration / the multigrid-preconditioned one
def test_smooth_wide_boxes_marching_kernels(ctx, oracle, dtq, base, monkeypatch):
    """boxes wider than a wavefront row and taller than a z chunk (every other smoothing test has boxes of <= 16 cells: two rows of 32
    lanes, one chunk): 80-cell boxes = a full 64-cell tile + a partly filled one, two chunks of planes;
    46-cell boxes = one partly filled tile in x and a last tile of rows that is partly outside the box.
    The z-marching stencil kernels (k_smooth_march) give the SAME BITS as the cell-per-thread kernels (PA_SMOOTH_MARCH=0) whatever
    the chunk length, and the field agrees with the oracle's solve"""
    H = nested_hierarchy(base, 2, base, is_per=(1, 0, 0))
    rhs = []
    for lv in H.levels:
        m = MultiFab(lv, 1, 0)
        fill_analytic(m, 0, lambda x, y, z: (field_flame(x, y, z, 0) - 300.0) / 1700.0)
        rhs.append(m)
    bc = capi.bc_from_flags((1, 0, 0))
    dt = dtq / (2.0 * base) ** 2
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    drhs = [capi.DevMF.from_host(ctx, dl, r) for dl, r in zip(dls, rhs)]
    out = {}
    variants = (("0", "64"), ("1", "64"))
    for march, kz in variants:
        monkeypatch.setenv("PA_SMOOTH_MARCH", march)
        capi.reload_options()
        dsol = [sentinel_out(ctx, dl, 1) for dl in dls]
        it, res = capi.smooth_solve(ctx, drhs, 0, dsol, 0, dt, bc, tol=1e-13, maxiter=500)
        assert res <= 1e-13
        out[(march, kz)] = (_written([d.download() for d in dsol]), it, res)
    monkeypatch.delenv("PA_SMOOTH_MARCH")
    capi.reload_options()
    ref = out[variants[0]]
    for key in variants[1:]:
        assert out[key][1] == ref[1] and out[key][2] == ref[2], (key, out[key][1:], ref[1:])
        for l, lv in enumerate(H.levels):
            for b in range(lv.nboxes):
                assert np.array_equal(out[key][0][l].valid(b)[0], ref[0][l].valid(b)[0]), (key, l, b)
    if base > 64 and dtq > 8:
        return  # (the oracle's unpreconditioned solve of the stiff case takes half a minute at this size: compared on the smaller hierarchy)
    want, oit, ores = oracle.smooth_solve(H.levels, rhs, 0, dt, bc, MultiFab, tol=1e-13, maxiter=2000)
    assert ores <= 1e-13
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            assert np.abs(ref[0][l].valid(b)[0] - want[l].valid(b)[0]).max() <= 1e-10, (l, b)


# ---------------------------------------------------------------- the one-rank solve on the case matrix (smooth_cases.py)
# General BoxArrays through k_smooth_avgdown + k_smooth_reflux + the masked k_smooth_march: L-shaped regions, concave coarse-fine
# corners (a coarse cell refluxed from two or three sides), fine boxes on walls and through periodic faces, partly covered faces,
# 4-wide and 2-thin boxes, four levels, the 2-D build.  Right-hand sides from smooth_cases.manufactured, so the analytic solution of
# the PDE is known as well.  Tolerances are the file's: solve tolerance x condition number (1 + 12 q), see the docstring on top.
import smooth_cases as sc  # noqa: E402

MATRIX = list(sc.CASES) + ["march_shapes"]
Q_TOL = {2.0: (1e-14, 1e-12, 1e-12), 100.0: (1e-13, 1e-10, 1e-11)}  # q = dt / dx^2 (finest): solve tolerance, field bound, residual bound
_cache = {}


def _case(name):
    if name == "march_shapes":
        return sc.march_shapes(), (1, 0, 0), (1, 0, 0)
    return sc.build(name)


def _oracle_case(oracle, name, q):
    """hierarchy, right-hand side, the oracle's solve and its error against the analytic solution: computed once, shared, not modified"""
    key = (name, q)
    if key not in _cache:
        H, per, bc3 = _case(name)
        dt = q * sc.finest_dx2(H)
        phi, rhs_fn = sc.manufactured(H, per, dt)
        rhs = sc.fill(H, rhs_fn)
        bc = capi.bc_from_flags(bc3)
        want, oit, ores = oracle.smooth_solve(H.levels, rhs, 0, dt, bc, MultiFab, tol=Q_TOL[q][0], maxiter=2000)
        assert oit > 0 and ores <= Q_TOL[q][0], (oit, ores)
        _cache[key] = dict(H=H, bc=bc, dt=dt, phi=phi, rhs=rhs, want=want, oit=oit, oerr=sc.max_uncovered(H, want, fn=phi))
    return _cache[key]


def _solve(ctx, H, rhs, dt, bc, tol, maxiter=2000):
    """every call builds its own DevLevels and DevMFs"""
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    drhs = [capi.DevMF.from_host(ctx, dl, r) for dl, r in zip(dls, rhs)]
    dsol = [sentinel_out(ctx, dl, 1) for dl in dls]
    it, res = capi.smooth_solve(ctx, drhs, 0, dsol, 0, dt, bc, tol=tol, maxiter=maxiter)
    return _written([d.download() for d in dsol]), it, res


@pytest.mark.parametrize("q", [2.0, 100.0])  # the plain iteration / the V-cycle-preconditioned one (the default above q = 8)
@pytest.mark.parametrize("name", MATRIX)
def test_smooth_matrix_matches_oracle(ctx, oracle, name, q):
    """one-rank pa_smooth_solve on every case: against the oracle's solve, under the oracle's operator, against the analytic solution
    (no worse than 1.01 x the oracle's own error), conservation to the bound the returned residual implies, covered cells = child
    means, and a constant right-hand side"""
    tol, fbound, rbound = Q_TOL[q]
    c = _oracle_case(oracle, name, q)
    H, bc, dt, rhs, want = c["H"], c["bc"], c["dt"], c["rhs"], c["want"]
    got, it, res = _solve(ctx, H, rhs, dt, bc, tol)
    assert it > 0 and res <= tol, (it, res)
    # against the oracle's solve
    d = max(float(np.abs(got[l].valid(b)[0] - want[l].valid(b)[0]).max()) for l, lv in enumerate(H.levels) for b in range(lv.nboxes))
    # the GPU field under the ORACLE's operator
    y, mask = oracle.smooth_apply(H.levels, sc.with_ghosts(H, got), dt, bc, MultiFab)
    r = max(float(np.abs((y[l].valid(b)[0] - rhs[l].valid(b)[0]) * mask[l].valid(b)[0]).max()) for l, lv in enumerate(H.levels) for b in range(lv.nboxes))
    # against the analytic solution of the PDE
    err = sc.max_uncovered(H, got, fn=c["phi"])
    # conservation: sum vol A x = sum vol x over the uncovered cells, so |sum vol (sol - rhs)| = |sum vol (A sol - rhs)| + rounding
    # <= V_domain * (res * ||rhs||_inf) + 64 ulp * sum vol |sol|
    cons = asum = 0.0
    for l, lv in enumerate(H.levels):
        vol = float(np.prod(lv.dx))
        for b in range(lv.nboxes):
            m = mask[l].valid(b)[0]
            cons += vol * float(((got[l].valid(b)[0] - rhs[l].valid(b)[0]) * m).sum())
            asum += vol * float((np.abs(got[l].valid(b)[0]) * m).sum())
    lv0 = H.levels[0]
    rmax = max(float(np.abs(m.valid_concat(0)).max()) for m in rhs)
    cbound = float(np.prod(lv0.prob_hi - lv0.prob_lo)) * res * rmax + 64 * np.finfo(float).eps * asum
    print(f"{name} q={q:g}: {it} iterations (oracle {c['oit']}), res {res:.2e}; |gpu - oracle| {d:.2e}, residual under the oracle's operator {r:.2e}, "
          f"error {err:.3e} (oracle {c['oerr']:.3e}), conservation {abs(cons):.2e} (bound {cbound:.2e})")
    assert d <= fbound, d
    assert r <= rbound, r
    assert err <= 1.01 * c["oerr"], (err, c["oerr"])
    assert abs(cons) <= cbound, (cons, cbound)
    # covered coarse cells: the mean of their 8 (4) children, summed as k_smooth_avgdown sums them
    planar = sc.is_planar(H)
    for l in range(H.nlev - 1):
        cd, fd = sc.dense(H.levels[l], got[l]), sc.dense(H.levels[l + 1], got[l + 1])
        s = np.zeros_like(cd)
        for kk in range(1 if planar else 2):
            for jj in range(2):
                for ii in range(2):
                    s = s + fd[kk::(1 if planar else 2), jj::2, ii::2]
        s *= 0.25 if planar else 0.125
        cov = ~np.isnan(s)
        assert cov.any() and not np.isnan(cd[cov]).any()
        assert np.all(np.abs(cd[cov] - s[cov]) <= 2 * np.spacing(np.abs(s[cov]))), (l, float(np.abs(cd[cov] - s[cov]).max()))
    # a constant right-hand side comes back
    const = []
    for lv in H.levels:
        const.append(MultiFab(lv, 1, 0, fill=0.7))
    gc, itc, resc = _solve(ctx, H, const, dt, bc, tol)
    dc = max(float(np.abs(m.valid_concat(0) - 0.7).max()) for m in gc)
    assert dc <= 1e-12, dc


def _noisy_rhs(name, q):
    """the manufactured right-hand side plus seeded noise: every mode of the operator is in it"""
    H, per, bc3 = _case(name)
    dt = q * sc.finest_dx2(H)
    rhs = sc.fill(H, sc.manufactured(H, per, dt)[1])
    rng = np.random.default_rng(23)
    for m in rhs:
        for b in range(m.level.nboxes):
            v = m.valid(b)[0]
            v += 0.05 * rng.uniform(-1, 1, size=v.shape)
    return H, capi.bc_from_flags(bc3), dt, rhs


@pytest.mark.parametrize("q", [2.0, 20.0])  # the Jacobi modes of the marching kernel run in the V-cycle of q = 20
@pytest.mark.parametrize("name", ["hand-110", "union9", "march_shapes"])
def test_smooth_kernel_variants_same_bits_on_the_matrix(ctx, name, q, options):
    """k_smooth_march against the cell-per-thread kernels (PA_SMOOTH_MARCH=0) on boxes 33, 65, 2 and 32 cells wide with 9, 2 and 11
    rows and 66 planes, and on masked irregular levels: the same iteration count and the same bits"""
    H, bc, dt, rhs = _noisy_rhs(name, q)
    out = {}
    for march in ("0", None):
        options(PA_SMOOTH_MARCH=march)
        out[march] = _solve(ctx, H, rhs, dt, bc, 1e-13)
        assert out[march][2] <= 1e-13
    assert out["0"][1] == out[None][1] and out["0"][2] == out[None][2], (out["0"][1:], out[None][1:])
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            assert np.array_equal(out["0"][0][l].valid(b)[0], out[None][0][l].valid(b)[0]), (l, b, lv.boxes[b])


@pytest.mark.parametrize("name", ["hand-000", "union4", "union9", "union14"])
def test_smooth_preconditioner_on_irregular_levels(ctx, name, options):
    """q = 100 on level-0 boxes 8 and 10 (7, 6) cells wide: the coarsening below level 0 stops after no or one step, the coarsest
    problem of the V-cycle is still stiff and gets the ~3 sqrt(cond) Jacobi steps (`nub`'s stiff branch).  Preconditioned and plain
    solves agree to tolerance x condition number, the preconditioner is the default and needs fewer iterations (no ratio asserted:
    the factor 3 of test_smooth_multigrid_preconditioner was measured on the nested hierarchy; the counts are in DESIGN.md section 3)"""
    H, per, bc3 = _case(name)
    dt = 100.0 * sc.finest_dx2(H)
    rhs = sc.fill(H, sc.manufactured(H, per, dt)[1])
    bc = capi.bc_from_flags(bc3)
    out = {}
    for mg in ("0", "1", None):
        options(PA_SMOOTH_MG=mg)
        out[mg] = _solve(ctx, H, rhs, dt, bc, 1e-13)
        assert out[mg][2] <= 1e-13
    counts = f"{name}: preconditioned {out['1'][1]}, plain {out['0'][1]} iterations"
    print(counts)
    assert out[None][1] == out["1"][1], "dt / dx^2 = 100: the preconditioner is the default"
    for l, lv in enumerate(H.levels):
        for b in range(lv.nboxes):
            assert np.abs(out["1"][0][l].valid(b)[0] - out["0"][0][l].valid(b)[0]).max() <= 1e-10, (l, b)
            assert np.array_equal(out["1"][0][l].valid(b)[0], out[None][0][l].valid(b)[0]), (l, b)
    assert out["1"][1] < out["0"][1], counts


@pytest.mark.parametrize("q", [2.0, 100.0])
@pytest.mark.parametrize("name", ["hand-110", "planar_L-10"])
def test_smooth_is_reproducible_on_concave_hierarchies(ctx, name, q):
    """in a concave coarse-fine corner a coarse cell takes reflux corrections from two or three faces: their summation order is
    fixed (face order 0..5, as k_smooth_reflux_apply), so three solves on fresh multifabs give the same iteration count and bits"""
    H, bc, dt, rhs = _noisy_rhs(name, q)
    runs = [_solve(ctx, H, rhs, dt, bc, 1e-13) for _ in range(3)]
    for got, it, res in runs[1:]:
        assert (it, res) == (runs[0][1], runs[0][2]), ((it, res), runs[0][1:])
        for l, lv in enumerate(H.levels):
            for b in range(lv.nboxes):
                assert np.array_equal(got[l].valid(b)[0], runs[0][0][l].valid(b)[0]), (l, b)
