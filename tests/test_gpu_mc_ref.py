"""GPU tier: the marching-cubes, marching-squares and merge kernels against the output of the REFERENCE's own compiled code
(Src/isosurface.cpp, Edge through Element), recorded in tests/golden/mc_ref.npz over the case matrix of tests/mc_cases.py --
directly, not through the oracle's restatement; every comparison bit for bit (vertices as int64 views, edge keys, vertex order
and connectivity entry by entry).  Reads the fixture and the case matrix only: no reference tree, no oracle/_ref."""
import ctypes as C

import numpy as np
import pytest

import mc_cases as M
from peleanalysis_amd import capi

pytestmark = pytest.mark.gpu

FAB_CASES = ["all_cubes", "near_iso", "exact_1090", "masked_edges"]
HIER_CASES = ["amr_r2_periodic_ng1", "amr_r2_periodic_ng2", "amr_r4", "amr3"]
SQUARE_CASES = ["squares_all", "squares_amr_per0", "squares_amr_per1"]
MERGE_CASES = ["amr_r2_periodic_ng1", "amr_r2_periodic_ng2", "amr_r4", "amr3"]


@pytest.fixture(scope="module")
def gold():
    return M.load_golden()


@pytest.fixture(scope="module")
def matrix(oracle):
    """the cases, built once and left unchanged (the oracle only fills ghost cells here; no expected value comes from it)"""
    return {c["name"]: c for c in M.cases(oracle)}


def _case(matrix, gold, name):
    c, g = matrix[name], gold[name]
    if g["inputs"] is not None and "H" not in c:  # a single-FAB case whose inputs the fixture holds: run on exactly those
        arrs = [np.ascontiguousarray(a, dtype=np.float64 if a.dtype.kind == "f" else np.int64) for a in g["inputs"]]
        c = dict(c, fabs=[dict(fb, state=arrs[6 * q], mask=arrs[6 * q + 1], lo=arrs[6 * q + 2], hi=arrs[6 * q + 3], llo=arrs[6 * q + 4], lhi=arrs[6 * q + 5])
                          for q, fb in enumerate(c["fabs"])])
    assert g["sha"] == M.input_digest(c), f"{name}: the inputs built on this machine are not the ones the fixture was recorded for"
    assert len(g["per_fab"]) == len(c["fabs"]) and g["iso"] == c["iso"]
    return c, g


def test_matrix_covers_every_case(gold):
    assert set(FAB_CASES + HIER_CASES + SQUARE_CASES) == set(gold)
    assert {k for k, g in gold.items() if g["merged"] is not None and g["dim"] == 3} == set(MERGE_CASES)


@pytest.mark.parametrize("name", FAB_CASES)
def test_fab_entry_points_match_reference(ctx, matrix, gold, name):
    """pa_mc_count_fab / pa_mc_emit_fab on every run of the single-FAB cases: all 256 cube indices; values within 1e-15 of the iso
    value on either side of it; exact hits at 1090; a masked point, a masked slab flush with the loop box, a loop box one cell
    thick, an empty loop box"""
    c, g = _case(matrix, gold, name)
    nc, iso = c["nc"], c["iso"]
    ntri = 0
    for fb, want in zip(c["fabs"], g["per_fab"]):
        what = f"{name} run {fb['box']}"
        ts, tm = capi.DevBuf.from_numpy(ctx, fb["state"]), capi.DevBuf.from_numpy(ctx, fb["mask"])
        fs, fm, bx = capi.PaFab(), capi.PaFab(), capi.PaBox()
        fs.p, fs.ncomp, fs.nstride = ts.ptr, nc, 0
        fm.p, fm.ncomp, fm.nstride = tm.ptr, 1, 0
        for d in range(3):
            fs.lo[d] = fm.lo[d] = int(fb["lo"][d]); fs.hi[d] = fm.hi[d] = int(fb["hi"][d])
            bx.lo[d], bx.hi[d] = int(fb["llo"][d]), int(fb["lhi"][d])
        nv, nt = C.c_int64(-1), C.c_int64(-1)
        ctx.check(ctx.lib.pa_mc_count_fab(ctx.h, bx, fs, fm, c["isocomp"], iso, C.byref(nv), C.byref(nt)))
        assert (nv.value, nt.value) == (len(want[0]), len(want[2])), f"{what}: counts differ from the reference's"
        tv, tk, tt = capi.DevBuf(ctx, max(nv.value, 1) * nc * 8), capi.DevBuf(ctx, max(nv.value, 1) * 6 * 4), capi.DevBuf(ctx, max(nt.value, 1) * 3 * 4)
        ctx.check(ctx.lib.pa_mc_emit_fab(ctx.h, bx, fs, fm, c["isocomp"], iso, tv.ptr, tk.ptr, tt.ptr, nv.value, nt.value))
        got = (tv.to_numpy(np.float64, (max(nv.value, 1), nc))[:nv.value], tk.to_numpy(np.int32, (max(nv.value, 1), 6))[:nv.value],
               tt.to_numpy(np.int32, (max(nt.value, 1), 3))[:nt.value])
        M.assert_same_surface(got, want, what)
        ntri += nt.value
    assert ntri > 500


def _box_array(loops):
    arr = (capi.PaBox * max(len(loops), 1))()
    for b in range(len(loops)):
        for d in range(3):
            arr[b].lo[d], arr[b].hi[d] = int(loops[b, d]), int(loops[b, 3 + d])
    return arr


def _level_fine(ctx, dst, fine, ratio, loops, isocomp, iso, nc, squares=False):
    """pa_mc_level_fine / pa_msq_level_fine with the case's refinement ratio -> per-box [(verts, keys, elts)]"""
    nb = len(loops)
    nv, nt = (C.c_int64 * nb)(), (C.c_int64 * nb)()
    pv, pk, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    fn = ctx.lib.pa_msq_level_fine if squares else ctx.lib.pa_mc_level_fine
    ctx.check(fn(ctx.h, dst.h, fine.h if fine is not None else None, int(ratio), _box_array(loops), isocomp, iso, nv, nt, C.byref(pv), C.byref(pk), C.byref(pt)))
    tv, tt = int(sum(nv[:nb])), int(sum(nt[:nb]))
    try:
        V = np.empty((tv, nc)); K = np.empty((tv, 6), np.int32); T = np.empty((tt, 3), np.int32)
        if tv:
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, V.ctypes.data_as(C.c_void_p), pv, V.nbytes))
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, K.ctypes.data_as(C.c_void_p), pk, K.nbytes))
        if tt:
            ctx.check(ctx.lib.pa_memcpy_d2h(ctx.h, T.ctypes.data_as(C.c_void_p), pt, T.nbytes))
    finally:
        if pv.value:
            ctx.lib.pa_device_free(ctx.h, pv)
    out, ov, ot = [], 0, 0
    for b in range(nb):
        out.append((V[ov:ov + nv[b]], K[ov:ov + nv[b]], T[ot:ot + nt[b]]))
        ov += nv[b]; ot += nt[b]
    return out


class _Device:
    """the levels and states of a hierarchy case on the device; closed when the test is done"""

    def __init__(self, ctx, c):
        self.dls = [capi.DevLevel(ctx, lv) for lv in c["H"].levels]
        self.dst = [capi.DevMF.from_host(ctx, dl, s) for dl, s in zip(self.dls, c["states"])]
        self.own = []

    def mask(self, ctx, c, l):
        dm = capi.DevMF(ctx, self.dls[l], 1, c["ng"])
        self.own.append(dm)
        ctx.check(ctx.lib.pa_iso_mask_level(ctx.h, dm.h, 0, self.dls[l + 1].h if l + 1 < len(self.dls) else None, c["ratio"]))
        return dm

    def close(self):
        for m in self.own + self.dst:
            m.close()
        for dl in reversed(self.dls):
            dl.close()


def _per_level(c, g):
    """the recorded per-FAB outputs, level by level in box order"""
    out = [[] for _ in c["H"].levels]
    for fb, want in zip(c["fabs"], g["per_fab"]):
        assert fb["box"] == len(out[fb["level"]])
        out[fb["level"]].append(want)
    return out


@pytest.mark.parametrize("cells", ["slab", "fallbacks"])
@pytest.mark.parametrize("name", HIER_CASES)
def test_level_and_hierarchy_entry_points_match_reference(ctx, options, matrix, gold, name, cells):
    """pa_iso_mask_level + pa_mc_level, pa_mc_level_fine (one call per level) and pa_mc_hierarchy_fine (one call) with the case's
    refinement ratio (amr_r4: 4), on the slab form of the cell pass and, with PA_FORCE_FALLBACKS=1, on its first form: per FAB
    what the reference's Polygonise loop returned -- base 24^3 with the fine level flush with a periodic face and 1 or 2 ghost
    layers, ratio 4, three levels"""
    if cells == "fallbacks":
        options(PA_FORCE_FALLBACKS=1)
    c, g = _case(matrix, gold, name)
    want = _per_level(c, g)
    H, nc, iso, ic, ratio = c["H"], c["nc"], c["iso"], c["isocomp"], c["ratio"]
    dev = _Device(ctx, c)
    try:
        ntri = 0
        for l, lv in enumerate(H.levels):
            dm = dev.mask(ctx, c, l)
            ctx.sync()
            gm = dm.download()
            for b in range(lv.nboxes):
                assert np.array_equal(gm.fab(b)[0], c["fabs"][sum(x.nboxes for x in H.levels[:l]) + b]["mask"]), f"{name} level {l} box {b}: fine-covered mask differs"
            got = capi.mc_level(ctx, dev.dst[l], dm, c["loops"][l], ic, iso)  # takes the mask as it is: the ratio went into pa_iso_mask_level
            fine = _level_fine(ctx, dev.dst[l], dev.dls[l + 1] if l + 1 < H.nlev else None, ratio, c["loops"][l], ic, iso, nc)
            for b in range(lv.nboxes):
                M.assert_same_surface(got[b], want[l][b], f"{name} ({cells}) pa_mc_level level {l} box {b}")
                M.assert_same_surface(fine[b], want[l][b], f"{name} ({cells}) pa_mc_level_fine level {l} box {b}")
                ntri += len(want[l][b][2])
        hier = capi.mc_hierarchy(ctx, dev.dst, [1] * (H.nlev - 1) + [0], c["loops"], ic, iso, ratio=ratio)
        for l, lv in enumerate(H.levels):
            for b in range(lv.nboxes):
                M.assert_same_surface(hier[l][b], want[l][b], f"{name} ({cells}) pa_mc_hierarchy_fine level {l} box {b}")
        assert ntri > 1000 and all(sum(len(w[2]) for w in wl) > 0 for wl in want)
    finally:
        dev.close()


@pytest.mark.parametrize("cells", ["slab", "fallbacks"])
@pytest.mark.parametrize("name", SQUARE_CASES)
def test_marching_squares_entry_points_match_reference(ctx, options, matrix, gold, name, cells):
    """pa_msq_level (mask multifab) and pa_msq_level_fine on the 2-D cases, against the reference's Segmentise built with
    AMREX_SPACEDIM == 2: all 16 square cases with both saddles; a two-level hierarchy, walls and a periodic direction"""
    if cells == "fallbacks":
        options(PA_FORCE_FALLBACKS=1)
    c, g = _case(matrix, gold, name)
    want = _per_level(c, g)
    H, nc, iso, ic = c["H"], c["nc"], c["iso"], c["isocomp"]
    dev = _Device(ctx, c)
    try:
        nseg = 0
        for l, lv in enumerate(H.levels):
            dm = dev.mask(ctx, c, l)
            ctx.sync()
            got = capi.mc_level(ctx, dev.dst[l], dm, c["loops"][l], ic, iso, squares=True)
            fine = _level_fine(ctx, dev.dst[l], dev.dls[l + 1] if l + 1 < H.nlev else None, c["ratio"], c["loops"][l], ic, iso, nc, squares=True)
            for b in range(lv.nboxes):
                for (gv, gk, gt), entry in ((got[b], "pa_msq_level"), (fine[b], "pa_msq_level_fine")):
                    what = f"{name} ({cells}) {entry} level {l} box {b}"
                    assert (gk[:, [2, 5]] == 0).all() and (gt[:, 2] == -1).all(), f"{what}: the unused key / segment columns"
                    M.assert_same_surface((gv, np.ascontiguousarray(gk[:, [0, 1, 3, 4]]), np.ascontiguousarray(gt[:, :2])), want[l][b], what)
                nseg += len(want[l][b][2])
        assert nseg > 60
    finally:
        dev.close()


@pytest.mark.parametrize("name", MERGE_CASES)
def test_device_merge_matches_reference(ctx, gold, name):
    """pa_iso_merge on the reference's own per-FAB fragments, level-then-box order: the nodes and elements of the reference's
    std::set<Node> / std::set<Element>.  Every case of the matrix is defined in the reference, so a hand-back (None) fails."""
    g = gold[name]
    frags = M.fragments(g["per_fab"])
    got = capi.iso_merge(ctx, frags, g["nc"])
    assert got is not None, f"{name}: the device merge handed the surface back"
    M.assert_same_surface(got, g["merged"], f"{name}: pa_iso_merge")
    assert len(got[0]) < sum(len(v) for v, _ in frags)
