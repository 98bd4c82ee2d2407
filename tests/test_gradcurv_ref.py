"""CPU tier of the grad -> curvature reference tests: the dense long-double reference of tests/gradcurv_ref.py against the ORACLE
(orc_apply_bc, grad_pipeline, curvature_pipeline with and without its options) on the whole matrix of tests/gradcurv_cases.py, cell by cell within the reference's
own derived bound; the branches the matrix reaches; the polynomial known answers on the reference itself; and negative controls:
mistakes planted in the reference that the comparison must see at more than 1000 times the bound.  The GPU tier
(test_gpu_gradcurv_ref.py) runs the kernels through the same comparison.

Smallest |shift| / bound over the negative controls (the table is printed with -s): 7.0e+11 (unclipped coarse normals on `narrow`; the
others lie between 1.5e+14 and 1.8e+16.  A cell whose bound is zero -- a wall ghost, a clipped cell -- is rated against one unit
roundoff of its value).  The controls of the options (GaussianCurvature, StrainRate, ROST, VelFlameNormal): smallest 1.3e+12 (coarse-fine
ghost cells of G from the coarser level's normalised normal, on `tall`), the others between 4.9e+13 and 9.8e+15.  A transposed adjugate
is not among them: it is no mistake (test_transposed_adjugate_is_no_mistake); `adj_unsigned_minors` stands where it was meant to."""
import collections

import numpy as np
import pytest

import gradcurv_cases as GCC
import gradcurv_ref as GCR
from gradcurv_cases import Stat
from peleanalysis_amd.hierarchy import Level, MultiFab, cell_centers, chop_box, fill_analytic
from util import ref_out

LD = np.longdouble
BC = [c.name for c in GCC.bc_cases()]
PIPE = [c.name for c in GCC.pipe_cases()]
_ORC = {}


# ----------------------------------------------------------------------------- oracle results, computed once
def orc_bc(oracle, name):
    """per level the multifab after orc_apply_bc and the count it returned"""
    if ("bc", name) not in _ORC:
        case = GCC.bc_case(name)
        init = GCC.bc_data(case, None)
        out = []
        for l in range(len(case.levels)):
            has_crse = l > 0 and not case.no_coarse
            m = init[l].copy()
            nbad = oracle.lib().orc_apply_bc(oracle._p(oracle._mf(m)), case.comp, oracle._p(oracle._mf(init[l - 1] if has_crse else None)), case.ccomp, oracle._bc(case.bc),
                                             case.ratio, case.only_dir)
            out.append((m, nbad))
        _ORC[("bc", name)] = out
    return _ORC[("bc", name)]


def orc_grad(oracle, name):
    if ("grad", name) not in _ORC:
        case = GCC.pipe_case(name)
        og = [ref_out(lv, 4) for lv in case.levels]
        oracle.grad_pipeline(case.levels, GCC.pipe_states(name, 1), 0, case.bc, og, 0, multipass=True)
        _ORC[("grad", name)] = og
    return _ORC[("grad", name)]


def orc_curv(oracle, name, thr):
    if ("curv", name, thr) not in _ORC:
        case = GCC.pipe_case(name)
        oc = [ref_out(lv, 5) for lv in case.levels]
        oracle.curvature_pipeline(case.levels, GCC.pipe_states(name, 2), 0, case.bc, oc, 0, MultiFab, threshold=thr)
        _ORC[("curv", name, thr)] = oc
    return _ORC[("curv", name, thr)]


def orc_opts(oracle, name, thr):
    """all 17 components: the core and every option, the velocity at components 1..3"""
    if ("opts", name, thr) not in _ORC:
        case = GCC.pipe_case(name)
        oo = [ref_out(lv, 17) for lv in case.levels]
        oracle.curvature_pipeline(case.levels, GCC.pipe_states(name, 2, ncomp=4), 0, case.bc, oo, 0, MultiFab, threshold=thr, do_gauss=True, do_strain=True, strain_tensor=True,
                                  do_velnormal=True, vel_comp=1)
        _ORC[("opts", name, thr)] = oo
    return _ORC[("opts", name, thr)]


def _thr(case, clip):
    return case.threshold if clip else None


# ----------------------------------------------------------------------------- the matrix against the oracle
@pytest.mark.parametrize("name", BC)
def test_apply_bc_oracle_within_bound(oracle, name):
    """every face ghost cell orc_apply_bc writes: the wall ones equal the reference's (bound 0), the coarse-fine ones lie within the bound;
    the cells without coarse data are counted alike"""
    case = GCC.bc_case(name)
    ref, _ = GCC.bc_ref(name)
    st = Stat()
    for l, (m, nbad) in enumerate(orc_bc(oracle, name)):
        boxes, nmiss = ref[l]
        assert nbad == nmiss, f"{name} level {l}: the oracle counts {nbad} cells without coarse data, the reference {nmiss}"
        for b, (v, e, cfm, wallm) in enumerate(boxes):
            got = GCR.ring1(m.fab(b)[case.comp], case.alloc)
            mask = wallm | (cfm if not (l and case.no_coarse) else False)
            st.add(got[mask], v[mask], e[mask], f"{name} level {l} box {b}")
    if not case.no_coarse:
        print(st.check_cap(f"apply_bc {name}"))


@pytest.mark.parametrize("name", PIPE)
def test_grad_oracle_within_bound(oracle, name):
    case = GCC.pipe_case(name)
    g, ref = GCC.grad_ref(name)
    og = orc_grad(oracle, name)
    for c in range(4):
        st = Stat()
        for l, lv in enumerate(case.levels):
            for b in range(lv.nboxes):
                st.add(og[l].valid(b)[c], ref.valid(l, b, g[l][c].v), ref.valid(l, b, g[l][c].e), f"{name} grad comp {c} level {l} box {b}")
        print(st.check_cap(f"grad {name} comp {c}"))


@pytest.mark.parametrize("clip", [False, True], ids=["nothr", "thr"])
@pytest.mark.parametrize("name", PIPE)
def test_curvature_oracle_within_bound(oracle, name, clip):
    """Progress bit for bit, FlameNormal x 3 and MeanCurvature within the bound, clipped cells exactly zero; |grad c| far from the 1e-14
    branch wherever a normal is formed; the threshold clips between 5 % and 95 % of the cells"""
    case = GCC.pipe_case(name)
    thr = _thr(case, clip)
    out, ref = GCC.curv_ref(name, thr)
    oc = orc_curv(oracle, name, thr)
    assert ref.min_normgrad > 1e-3, f"{name}: |grad c| comes down to {ref.min_normgrad}"
    ncell = sum(lv.ncells for lv in case.levels)
    nclip = sum(int(o["clip"].sum()) for o in out)
    assert (0.05 * ncell < nclip < 0.95 * ncell) if clip else nclip == 0
    for what, k, f in (("K", 1, lambda o: o["K"]), ("n0", 2, lambda o: o["n"][0]), ("n1", 3, lambda o: o["n"][1]), ("n2", 4, lambda o: o["n"][2])):
        st = Stat()
        for l, lv in enumerate(case.levels):
            for b in range(lv.nboxes):
                got = oc[l].valid(b)
                if what == "K":
                    assert np.array_equal(got[0].view(np.int64), ref.valid(l, b, out[l]["c"]).view(np.int64)), f"{name} Progress level {l} box {b}"
                m = ref.valid(l, b, out[l]["clip"])
                assert (got[k][m] == 0.0).all(), f"{name} {what} level {l} box {b}: clipped cells are not zero"
                st.add(got[k], ref.valid(l, b, f(out[l]).v), ref.valid(l, b, f(out[l]).e), f"{name} {what} level {l} box {b}")
        print(st.check_cap(f"curvature {name} thr {thr} {what}"))


@pytest.mark.parametrize("clip", [False, True], ids=["nothr", "thr"])
@pytest.mark.parametrize("name", PIPE)
def test_options_oracle_within_bound(oracle, name, clip):
    """GaussianCurvature, StrainRate, VelFlameNormal and the nine ROST components within the bound; clipped GaussianCurvature and
    VelFlameNormal exactly zero; StrainRate is not clipped (more than nine in ten of the clipped cells hold a reference value that lies
    beyond twice the comparison's tolerance from zero, and the oracle's is not zero there); the five core components of the same call
    within theirs"""
    case = GCC.pipe_case(name)
    thr = _thr(case, clip)
    core, ref = GCC.curv_ref(name, thr)
    out, _ = GCC.opts_ref(name, thr)
    oo = orc_opts(oracle, name, thr)
    nclip, nfar = sum(int(o["clip"].sum()) for o in core), 0
    for k in range(5, 17):
        st = Stat()
        for l, lv in enumerate(case.levels):
            f = GCC.opt_field(out[l], k)
            for b in range(lv.nboxes):
                got = oo[l].valid(b)[k]
                m = ref.valid(l, b, core[l]["clip"])
                if k in (5, 7):
                    assert (got[m] == 0.0).all(), f"{name} {GCC.OPT_NAMES[k - 5]} level {l} box {b}: clipped cells are not zero"
                    assert (ref.valid(l, b, f.v)[m] == 0).all() and (ref.valid(l, b, f.e)[m] == 0).all()
                if k == 6:  # a clipped cell whose reference value lies beyond its bound from zero: the comparison below tells a zero from it
                    far = np.abs(ref.valid(l, b, f.v)[m]) > 4 * ref.valid(l, b, f.e)[m]
                    assert (got[m][far] != 0.0).all(), f"{name} StrainRate level {l} box {b}: clipped"
                    nfar += int(far.sum())
                st.add(got, ref.valid(l, b, f.v), ref.valid(l, b, f.e), f"{name} {GCC.OPT_NAMES[k - 5]} level {l} box {b}")
        print(st.check_cap(f"options {name} thr {thr} {GCC.OPT_NAMES[k - 5]}"))
    assert nfar > 0.9 * nclip if clip else nclip == 0, f"{name}: {nfar} of {nclip} clipped cells hold a StrainRate that a zero would miss"
    for what, k, f in (("K", 1, lambda o: o["K"]), ("n0", 2, lambda o: o["n"][0]), ("n1", 3, lambda o: o["n"][1]), ("n2", 4, lambda o: o["n"][2])):
        st = Stat()
        for l, lv in enumerate(case.levels):
            for b in range(lv.nboxes):
                got = oo[l].valid(b)
                assert np.array_equal(got[0].view(np.int64), ref.valid(l, b, core[l]["c"]).view(np.int64)), f"{name} Progress level {l} box {b}"
                st.add(got[k], ref.valid(l, b, f(core[l]).v), ref.valid(l, b, f(core[l]).e), f"{name} {what} with options level {l} box {b}")
        st.check_cap(f"options {name} thr {thr} {what}")


# ----------------------------------------------------------------------------- branches
def test_branch_coverage():
    """over the matrix every branch of the stencil selection, of the cross term, of the normal order and the clip is reached; each case
    reaches what it was added for"""
    total = collections.Counter()
    per = {}
    for name in BC:
        per[name] = GCC.bc_ref(name)[1].counts
        total.update(per[name])
    for name in PIPE:
        case = GCC.pipe_case(name)
        cnt = GCC.curv_ref(name, case.threshold)[1].counts
        total.update(cnt)
        for k in case.expect:
            assert cnt[k] > 0, f"pipeline case {name} does not reach {k}"
    for k in GCR.COUNT_KEYS:
        assert total[k] > 0, f"the matrix never reaches {k}"
    deep = GCC.curv_ref("deep", None)[1]
    assert len(deep.levels) == 5 and not all(R.whole for R in deep.R), "deep: five levels, the finer ones on windows"
    for t, nx in ((1, "nx2"), (2, "nx3"), (3, "nx4"), (4, "nx4")):
        for name in BC:
            if name.startswith(f"t{t}_"):
                assert per[name][nx] > 0, (name, nx)
    assert per["slots"]["st1"] > 0 and per["slots"]["st2"] > 0 and per["slots"]["nx3"] > 0
    for name in ("geo_d", "geo_f"):
        assert per[name]["st3o"] > 0 and per[name]["cross_off"] > 0, name
    assert sum(per["no_coarse"].values()) == 0 and GCC.bc_ref("no_coarse")[0][1][1] > 0
    for name in ("geo_c", "geo_e", "geo_g_ratio4"):
        assert per[name]["st3c"] > 0 and per[name]["cross_on"] > 0, name


def test_general_case_is_not_convex():
    """the `general` pipeline case: a box face that is partly covered by a neighbour and partly coarse-fine, and a coarse-fine ghost cell
    with a fine box on one side in a tangential direction (the concave corner: one-sided or shortened stencils, cross term off)"""
    ref = GCC.curv_ref("general", None)[1]
    part = False
    for B in ref.B[1]:
        for d, side, g, i in GCR.GR.bc_faces(B):
            k = B.cls[g]
            part |= bool((k == 0).any() and (k == 1).any())
    assert part
    assert ref.counts["st3o"] + ref.counts["st2"] > 0 and ref.counts["cross_off"] > 0


# ----------------------------------------------------------------------------- known answers on the reference itself
def _two_level(ncrse, clo, chi, box=None):
    clo, chi = np.asarray(clo), np.asarray(chi)
    L0 = Level(chop_box((0, 0, 0), (ncrse - 1,) * 3, box or ncrse), (0, 0, 0), (ncrse - 1,) * 3, (0, 0, 0), (0., 0., 0.), (1., 1., 1.))
    L1 = Level(chop_box(2 * clo, 2 * chi + 1, box or 2 * ncrse), (0, 0, 0), (2 * ncrse - 1,) * 3, (0, 0, 0), (0., 0., 0.), (1., 1., 1.))
    return [L0, L1]


@pytest.mark.parametrize("d", [0, 1, 2])
def test_reference_cf_ghost_exact_for_normal_cubic_plus_tangential_quadratic(d):
    """the reference's coarse-fine ghost value is exact for f = cubic(normal) + quadratic(tangential, mixed term included): every
    coarse-fine ghost cell behind the faces of the fine region holds f(ghost centre) to the rounding of the float64 inputs"""
    levels = _two_level(16, (4, 4, 4), (11, 11, 11), box=8)
    t0, t1 = [a for a in range(3) if a != d]

    def f(x, y, z):
        X = (x, y, z)
        n, a, b = X[d], X[t0], X[t1]
        return 1.0 + 0.7 * n - 1.3 * n * n + 2.1 * n ** 3 + 0.4 * a - 0.9 * b + 1.7 * a * a - 0.6 * b * b + 2.3 * a * b + 0 * x * y * z
    c, s = MultiFab(levels[0], 1, 1), MultiFab(levels[1], 1, 1)
    fill_analytic(c, 0, f)
    fill_analytic(s, 0, f)
    boxes, nmiss, _ = GCR.apply_bc(levels, 1, s, 0, c, 0, (1, 1, 1), only_dir=d)
    assert nmiss == 0
    nchecked = 0
    for b, (v, e, cfm, _) in enumerate(boxes):
        x, y, z = cell_centers(levels[1], b, 1)
        want = f(x, y, z)
        assert np.abs(v[cfm] - want[cfm]).max() < 5e-14 if cfm.any() else True, (d, b)
        nchecked += int(cfm.sum())
    assert nchecked == 2 * 16 * 16


def test_reference_cf_cross_term_only_when_all_four_diagonals_are_coarse_fine():
    """fine region flush with the z wall, f = y z on the x faces: in the first fine z pair the cross term is off (a diagonal position lies
    beyond the wall) and the one-sided z stencil is exact for a field linear in z, so the ghost value misses exactly yy zz H^2 times the
    normal cubic's weight 16/35 of the boundary value; everywhere else it is exact"""
    levels = _two_level(16, (4, 4, 0), (11, 11, 7))
    f = lambda x, y, z: y * z + 0 * x
    c, s = MultiFab(levels[0], 1, 1), MultiFab(levels[1], 1, 1)
    fill_analytic(c, 0, f)
    fill_analytic(s, 0, f)
    boxes, nmiss, ref = GCR.apply_bc(levels, 1, s, 0, c, 0, (1, 1, 1), only_dir=0)
    assert nmiss == 0 and ref.counts["cross_off"] == 2 * 2 * 16 and ref.counts["st3o"] == 2 * 2 * 16
    v, e, cfm, _ = boxes[0]
    x, y, z = cell_centers(levels[1], 0, 1)
    want = f(x, y, z)
    H = 1.0 / 16
    for xs in (0, -1):
        assert cfm[1:-1, 1:-1, xs].all()
        err = (v[1:-1, 1:-1, xs] - want[1:-1, 1:-1, xs]).astype(np.float64)
        assert np.abs(err[2:, :]).max() < 1e-15
        yy = np.where(np.arange(8, 24) % 2 == 0, -0.25, 0.25)[None, :]
        zz = np.array([-0.25, 0.25])[:, None]
        assert np.abs(err[:2, :] + (16.0 / 35.0) * yy * zz * H * H).max() < 1e-15


def test_reference_options_known_answer_quadratic_c_linear_u():
    """one level without a periodic direction, s a quadratic polynomial, u linear: centred differences are exact for both, so in cells at
    least two away from every wall G is the analytic gradient, H the analytic (constant) Hessian and grad u the analytic (constant,
    NOT symmetric) matrix -- ROST q = 3 d + m is told from 3 m + d in every cell --, and Kg is the closed form G^T adj(H) G / |G|^4 of the
    progress variable c = (s - pmin) / (pmax - pmin).  Tolerance: the inputs are float64 roundings of the polynomials (relative 2^-53 of
    values below 8); a difference multiplies that by dxinv = 16, the second one again: below 1e-12 on G, 2e-11 on H against entries
    of the size of 1, and Kg (cubic in them, of the size of 1) is asked to 1e-9"""
    n = 16
    L0 = Level(chop_box((0, 0, 0), (n - 1,) * 3, n), (0, 0, 0), (n - 1,) * 3, (0, 0, 0), (0., 0., 0.), (1., 1., 1.))
    Hs = np.array([[1.4, 0.5, -0.3], [0.5, -0.8, 0.6], [-0.3, 0.6, 1.1]])   # the Hessian of s
    g0 = np.array([2.0, 1.5, 2.5])                                          # its gradient at the origin: no zero of grad s in the unit cube
    A = np.array([[0.7, -0.4, 0.3], [0.2, 1.1, -0.5], [-0.6, 0.8, 0.4]])    # d u_d / d x_m
    u0 = np.array([0.3, -0.2, 0.5])

    def s(x, y, z):
        X = (x, y, z)
        return 1.0 + sum(g0[d] * X[d] for d in range(3)) + 0.5 * sum(Hs[d][m] * X[d] * X[m] for d in range(3) for m in range(3))
    mf = MultiFab(L0, 4, 2)
    mf.data[...] = np.nan
    fill_analytic(mf, 0, s)
    for d in range(3):
        fill_analytic(mf, 1 + d, lambda x, y, z, d=d: u0[d] + A[d][0] * x + A[d][1] * y + A[d][2] * z)
    ref = GCR.Ref([L0])
    core = ref.curvature([mf], 0, (1, 1, 1))
    out = ref.options([mf], 0, 1, (1, 1, 1), core=core)[0]
    inv = 1.0 / (core[0]["pmax"] - core[0]["pmin"])
    x, y, z = cell_centers(L0, 0, 0)
    X = np.broadcast_arrays(x, y, z, np.zeros((n, n, n)))[:3]
    G = [inv * (g0[d] + sum(Hs[d][m] * X[m] for m in range(3))) for d in range(3)]
    H = inv * Hs
    adj = np.linalg.det(H) * np.linalg.inv(H)     # symmetric: the adjugate's index order does not enter here
    gn2 = G[0] ** 2 + G[1] ** 2 + G[2] ** 2
    kg = sum(G[i] * adj[i][j] * G[j] for i in range(3) for j in range(3)) / gn2 ** 2
    i = (slice(2, -2),) * 3
    assert np.abs(kg[i]).max() > 0.1
    assert np.abs(out["Kg"].v[i].astype(np.float64) - kg[i]).max() < 1e-9
    for d in range(3):
        for m in range(3):
            assert np.abs(out["ROST"][3 * d + m].v[i].astype(np.float64) - A[d][m]).max() < 1e-11, (d, m)
    assert np.abs(out["SR"].v[i].astype(np.float64) - np.trace(A)).max() < 1e-11
    vn = -sum((u0[d] + sum(A[d][m] * X[m] for m in range(3))) * G[d] for d in range(3)) / np.sqrt(gn2)
    assert np.abs(out["VN"].v[i].astype(np.float64) - vn[i]).max() < 1e-11
    for k in range(5, 17):  # and the reference's own bound is finite and small there
        assert float(GCC.opt_field(out, k).e[i].max()) < 1e-10


# ----------------------------------------------------------------------------- negative controls
def _shift_bc(oracle, name, plant):
    """largest |planted reference - oracle| / bound over the face ghost cells of an applyBC case; a cell whose bound is zero (a wall
    ghost) is rated against one unit roundoff of its value"""
    case = GCC.bc_case(name)
    ref, _ = GCC.bc_ref(name, plant)
    good, _ = GCC.bc_ref(name)
    worst = 0.0
    for l, (m, _) in enumerate(orc_bc(oracle, name)):
        for b, (v, e, cfm, wallm) in enumerate(ref[l][0]):
            got = GCR.ring1(m.fab(b)[case.comp], case.alloc)
            mask = (cfm | wallm) & np.isfinite(v)
            bd = np.maximum(2 * good[l][0][b][1][mask], GCR.U * np.abs(got[mask]))
            if mask.any():
                worst = max(worst, float((np.abs(got[mask].astype(LD) - v[mask]) / bd).max()))
    return worst


def _shift_curv(oracle, name, plant, clip, comps):
    case = GCC.pipe_case(name)
    thr = _thr(case, clip)
    bad, ref = GCC.curv_ref(name, thr, plant)
    good, _ = GCC.curv_ref(name, thr)
    oc = orc_curv(oracle, name, thr)
    worst = 0.0
    pick = {1: lambda o: o["K"], 2: lambda o: o["n"][0], 3: lambda o: o["n"][1], 4: lambda o: o["n"][2]}
    for l, lv in enumerate(case.levels):
        for b in range(lv.nboxes):
            for k in comps:
                got = oc[l].valid(b)[k]
                v, e = ref.valid(l, b, pick[k](bad[l]).v), ref.valid(l, b, pick[k](good[l]).e)
                bd = np.maximum(2 * e, GCR.U * np.abs(got))
                nz = bd > 0
                if nz.any():
                    worst = max(worst, float((np.abs(got.astype(LD) - v)[nz] / bd[nz]).max()))
    return worst


def _shift_opts(oracle, name, plant, clip):
    """the same over the twelve option components"""
    case = GCC.pipe_case(name)
    thr = _thr(case, clip)
    bad, ref = GCC.opts_ref(name, thr, plant)
    good, _ = GCC.opts_ref(name, thr)
    oo = orc_opts(oracle, name, thr)
    worst = 0.0
    for l, lv in enumerate(case.levels):
        for b in range(lv.nboxes):
            for k in range(5, 17):
                got = oo[l].valid(b)[k]
                v, e = ref.valid(l, b, GCC.opt_field(bad[l], k).v), ref.valid(l, b, GCC.opt_field(good[l], k).e)
                bd = np.maximum(2 * e, GCR.U * np.maximum(np.abs(got), np.abs(v)))  # (a clipped cell holds 0.0: rated against the planted value)
                nz = bd > 0
                if nz.any():
                    worst = max(worst, float((np.abs(got.astype(LD) - v)[nz] / bd[nz]).max()))
    return worst


CONTROLS = [
    ("cross_off", "bc", "t4_nnn_ng1"), ("cross_on", "bc", "geo_f"), ("onesided2", "bc", "geo_d"), ("nx4", "bc", "t1_nnn_ng2"), ("nx4", "bc", "t2_pnr_ng1"),
    ("bpoint_half", "bc", "t4_nnn_ng1"), ("inside_domain", "bc", "geo_f"), ("odd_sign", "bc", "t1_rpn_ng2"),
    ("unclipped_coarse_n", "curv_thr", "narrow"), ("k_not_halved", "curv", "ragged"), ("plus_max", "curv", "ragged"),
    # the options.  Interior mixed differences commute, so the two transpositions show only next to walls and coarse-fine faces
    ("adj_unsigned_minors", "opts", "ragged"), ("adj_unsigned_minors", "opts", "tall"), ("kg_pow3", "opts", "general"), ("coarse_G_normalised", "opts", "tall"),
    ("hessian_of_n", "opts", "kgwide"), ("strain_nn", "opts", "ragged"), ("rost_transposed", "opts", "sym"), ("rost_transposed", "opts", "kgwide"),
    ("veln_unclipped_n", "opts_thr", "narrow"), ("vel_wall_even", "opts", "sym"), ("vel_wall_even", "opts", "ragged"),
]


@pytest.mark.parametrize("name", ["ragged", "tall"])
def test_transposed_adjugate_is_no_mistake(name):
    """the plant `adj_transposed` (the nine lines of :630-638 read row by row, or the Hessian's d and m exchanged: adj(H^T) = adj(H)^T) is
    NOT a negative control: G^T A^T G is the same sum of nine products as G^T A G, whether or not H is symmetric -- next to walls and
    coarse-fine faces, where the mixed differences do not commute, as well.  The transposed reference equals the plain one to the
    reference's own rounding in every cell, so no comparison can tell the two readings apart, and none has to.  The index order of the
    adjugate that does matter -- which minor carries which sign -- is the control `adj_unsigned_minors`"""
    case = GCC.pipe_case(name)
    bad, ref = GCC.opts_ref(name, None, "adj_transposed")
    good, _ = GCC.opts_ref(name, None)
    for l, lv in enumerate(case.levels):
        for b in range(lv.nboxes):
            d = np.abs(ref.valid(l, b, bad[l]["Kg"].v) - ref.valid(l, b, good[l]["Kg"].v))
            assert (d <= ref.valid(l, b, good[l]["Kg"].e)).all(), f"{name} level {l} box {b}"  # (holds where long double is float64 too)


@pytest.mark.parametrize("plant,kind,name", CONTROLS)
def test_planted_mistake_is_seen(oracle, plant, kind, name):
    """a condition on the comparison's discriminating power, not a tolerance: the planted mistake moves at least one compared cell of the
    named case by more than 1000 times that cell's bound"""
    if kind == "bc":
        r = _shift_bc(oracle, name, plant)
    elif kind.startswith("opts"):
        r = _shift_opts(oracle, name, plant, kind == "opts_thr")
    else:
        r = _shift_curv(oracle, name, plant, kind == "curv_thr", [2, 3, 4] if plant == "plus_max" else [1, 2, 3, 4])
    print(f"planted {plant} on {name}: |shift| / bound = {r:.2e}")
    assert r > 1000.0, f"{plant} on {name}: the largest shift is {r:.3g} bounds"
