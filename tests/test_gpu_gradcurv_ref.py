"""GPU tier of the grad -> curvature reference tests: pa_apply_bc, pa_grad_run, pa_curvature_run (pass by pass and fused) and
pa_gradcurv_run through the C ABI against the dense long-double reference of tests/gradcurv_ref.py on the matrix of
tests/gradcurv_cases.py (the CPU tier, test_gradcurv_ref.py, holds the oracle to the same reference and every case to its branches).
Outputs start as SENT_GPU everywhere.  Per case, in this order: no coarse data missing (pa_bc_errors); no sentinel and no non-finite
value in any compared cell, each checked on its own (a NaN fails `<=` only by accident); every compared cell within its bound
(|got - ref| <= 2 e, gradcurv_ref.py).  No cell is left out: every face ghost cell of pa_apply_bc, every valid cell of every output
component of the pipelines.  Each test prints its worst error / bound (-s).
The options of pa_curvature_run (GaussianCurvature, StrainRate, VelFlameNormal, the nine ROST components) against Ref.options on all
three implementations: pass by pass (pa_curvature_last_path 0), one options pass per level (1: k_curvopts, on `tall` with a second
z segment in both tile shapes and a grid sized by one box and decoded by another) and the Gaussian curvature inside the sweep (2:
`kgwide`); and the options one by one (the launches of k_curvopts that `every option on` never makes)."""
import numpy as np
import pytest

import gradcurv_cases as GCC
import gradcurv_ref as GCR
from gradcurv_cases import Stat
from peleanalysis_amd import capi
from util import SENT_GPU, SENT_REF, assert_untouched, bits_equal, sentinel_count, sentinel_out

pytestmark = pytest.mark.gpu

BC = [c.name for c in GCC.bc_cases()]
PIPE = [c.name for c in GCC.pipe_cases()]
# the additional switches, each at the case the matrix names for it
SWITCHES = [("narrow", "PA_FUSED2", 0), ("sym", "PA_FORCE_FALLBACKS", 1)]
RUNS = [(n, None, None) for n in PIPE] + SWITCHES
RUN_IDS = [n if k is None else f"{n}-{k}={v}" for n, k, v in RUNS]


def _clean(got, what):
    """no sentinel, nothing non-finite"""
    n = sentinel_count(got, SENT_GPU) + sentinel_count(got, SENT_REF)
    assert n == 0, f"{what}: {n} of {got.size} compared cells were never written"
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite values"


def _close(objs):
    for o in objs:
        o.close()


# ----------------------------------------------------------------------------- pa_apply_bc
@pytest.mark.parametrize("fallbacks", [0, 1], ids=["plans", "fallbacks"])
@pytest.mark.parametrize("name", BC)
def test_apply_bc_matrix(ctx, options, name, fallbacks):
    """every face ghost cell pa_apply_bc writes -- the wall ones hold the reference's bits, the coarse-fine ones lie within the bound -- and
    nothing else changed: the whole buffer equals the uploaded one with those cells replaced.  Ratio 4 with coarse data is refused
    (quirk Q11) and leaves everything as it was"""
    case = GCC.bc_case(name)
    options(PA_FORCE_FALLBACKS=1 if fallbacks else None)
    init = GCC.bc_data(case, SENT_GPU)
    ref, _ = GCC.bc_ref(name)
    dls = [capi.DevLevel(ctx, lv) for lv in case.levels]
    dmf = [capi.DevMF.from_host(ctx, dl, m) for dl, m in zip(dls, init)]
    st = Stat()
    try:
        for l in range(len(case.levels)):
            has_crse = l > 0 and not case.no_coarse
            ctx.sync()
            assert ctx.bc_errors() == 0
            rc = ctx.lib.pa_apply_bc(ctx.h, dmf[l].h, case.comp, dmf[l - 1].h if has_crse else None, case.ccomp, capi._i3(case.bc), case.ratio, case.only_dir)
            ctx.sync()
            got = dmf[l].download()
            if case.ratio != 2 and has_crse:
                assert rc != 0 and b"ratio 2" in ctx.lib.pa_last_error(ctx.h), f"{name} level {l}: ratio {case.ratio} was not refused"
                assert ctx.bc_errors() == 0 and bits_equal(got.data, init[l].data), f"{name} level {l}: a refused call changed the multifab"
                continue
            ctx.check(rc)
            boxes, nmiss = ref[l]
            assert ctx.bc_errors() == nmiss, f"{name} level {l}"
            want = init[l].copy()
            for b, (v, e, cfm, wallm) in enumerate(boxes):
                g = GCR.ring1(got.fab(b)[case.comp], case.alloc)
                w = GCR.ring1(want.fab(b)[case.comp], case.alloc)
                mask = wallm | cfm if (has_crse or l == 0) else wallm
                _clean(g[mask], f"{name} level {l} box {b}")
                assert bits_equal(g[wallm], v[wallm].astype(np.float64)), f"{name} level {l} box {b}: wall ghost cells"
                st.add(g[mask], v[mask], e[mask], f"{name} level {l} box {b}")
                w[mask] = g[mask]
            assert bits_equal(got.data, want.data), f"{name} level {l}: something else than the face ghost cells changed"
        if st.n and not case.no_coarse and case.ratio == 2:
            print(st.check_cap(f"GPU apply_bc {name} {'fallbacks' if fallbacks else 'plans'}"))
    finally:
        _close(dmf + dls)


# ----------------------------------------------------------------------------- pipelines
def _dev(ctx, name, ng, ncomp=1):
    case = GCC.pipe_case(name)
    dls = [capi.DevLevel(ctx, lv) for lv in case.levels]
    dst = [capi.DevMF.from_host(ctx, dl, s) for dl, s in zip(dls, GCC.pipe_states(name, ng, SENT_GPU, ncomp))]
    return case, dls, dst


def _check_grad(case, name, got, gcomp0, what):
    g, ref = GCC.grad_ref(name)
    for c in range(4):
        st = Stat()
        for l, lv in enumerate(case.levels):
            for b in range(lv.nboxes):
                a = got[l].valid(b)[gcomp0 + c]
                _clean(a, f"{what} grad comp {c} level {l} box {b}")
                st.add(a, ref.valid(l, b, g[l][c].v), ref.valid(l, b, g[l][c].e), f"{what} grad comp {c} level {l} box {b}")
        print(st.check_cap(f"GPU {what} grad comp {c}"))


def _check_curv(case, name, thr, got, pcomp, kcomp, ncomp0, what):
    """pcomp: Progress (None: the entry point has no such output), kcomp: MeanCurvature, ncomp0: FlameNormal"""
    out, ref = GCC.curv_ref(name, thr)
    for label, k, f in (("K", kcomp, lambda o: o["K"]), ("n0", ncomp0, lambda o: o["n"][0]), ("n1", ncomp0 + 1, lambda o: o["n"][1]), ("n2", ncomp0 + 2, lambda o: o["n"][2])):
        st = Stat()
        for l, lv in enumerate(case.levels):
            for b in range(lv.nboxes):
                a = got[l].valid(b)
                if label == "K" and pcomp is not None:
                    _clean(a[pcomp], f"{what} Progress level {l} box {b}")
                    assert bits_equal(a[pcomp], ref.valid(l, b, out[l]["c"])), f"{what} Progress level {l} box {b}"
                _clean(a[k], f"{what} {label} level {l} box {b}")
                m = ref.valid(l, b, out[l]["clip"])
                assert (a[k][m] == 0.0).all(), f"{what} {label} level {l} box {b}: clipped cells are not zero"
                st.add(a[k], ref.valid(l, b, f(out[l]).v), ref.valid(l, b, f(out[l]).e), f"{what} {label} level {l} box {b}")
        print(st.check_cap(f"GPU {what} {label}"))


def _wide_sweep_ran(ctx, name, clip, what):
    """the sweep the call launched is recorded (-s); in the `wide` case it must be a wide one -- and this call's: the name says whether it clips"""
    kn = ctx.lib.pa_sweep_kernel_name(ctx.h).decode()
    print(f"GPU {what}: sweep {kn}")
    if name == "wide":
        assert kn.startswith("k_gradcurv_march3<") or kn.startswith("k_gradcurv_march3_levels<"), f"{what}: not a wide sweep: {kn}"
        assert (",CLIP>" in kn or ",CLIP=1" in kn) == clip, f"{what}: the recorded sweep is another call's: {kn}"


@pytest.mark.parametrize("name", PIPE)
def test_grad_run(ctx, name):
    case, dls, dst = _dev(ctx, name, 1)
    dout = [sentinel_out(ctx, dl, 4) for dl in dls]
    try:
        capi.grad_run(ctx, dst, 0, case.bc, dout, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        _check_grad(case, name, [d.download() for d in dout], 0, f"pa_grad_run {name}")
    finally:
        _close(dout + dst + dls)


@pytest.mark.parametrize("clip", [False, True], ids=["nothr", "thr"])
@pytest.mark.parametrize("fused", [False, True], ids=["passes", "fused"])
@pytest.mark.parametrize("name,key,val", RUNS, ids=RUN_IDS)
def test_curvature_run(ctx, options, name, key, val, fused, clip):
    """Progress bit for bit, FlameNormal x 3 and MeanCurvature within the bound, clipped cells zero"""
    if key:
        options(**{key: val})
    case, dls, dst = _dev(ctx, name, 2)
    thr = case.threshold if clip else None
    dout = [sentinel_out(ctx, dl, 5) for dl in dls]
    what = f"pa_curvature_run {'fused' if fused else 'passes'} {name}{f' {key}={val}' if key else ''} thr {thr}"
    try:
        capi.curvature_run(ctx, dst, 0, case.bc, capi.curv_params(threshold=thr, fused=fused), dout, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        if fused:
            path = ctx.lib.pa_curvature_last_path(ctx.h)
            print(f"GPU {what}: path {path}")
            if path == 1:
                _wide_sweep_ran(ctx, name, clip, what)
            assert path == 1 or name != "wide", f"{what}: the wide case did not take the sweep"
        _check_curv(case, name, thr, [d.download() for d in dout], 0, 1, 2, what)
    finally:
        _close(dout + dst + dls)


@pytest.mark.parametrize("clip", [False, True], ids=["nothr", "thr"])
@pytest.mark.parametrize("name,key,val", RUNS, ids=RUN_IDS)
def test_gradcurv_run(ctx, options, name, key, val, clip):
    """the fused headline entry point: gx gy gz |g|, FlameNormal x 3, MeanCurvature"""
    if key:
        options(**{key: val})
    case, dls, dst = _dev(ctx, name, 2)
    thr = case.threshold if clip else None
    work = [capi.DevMF(ctx, dl, 1, 2) for dl in dls]
    dout = [sentinel_out(ctx, dl, 8) for dl in dls]
    what = f"pa_gradcurv_run {name}{f' {key}={val}' if key else ''} thr {thr}"
    try:
        capi.gradcurv_run(ctx, dst, 0, case.bc, capi.curv_params(threshold=thr, fused=True), work, dout, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        _wide_sweep_ran(ctx, name, clip, what)
        got = [d.download() for d in dout]
        _check_grad(case, name, got, 0, what)
        _check_curv(case, name, thr, got, None, 7, 4, what)
    finally:
        _close(work + dout + dst + dls)


# ----------------------------------------------------------------------------- the options of pa_curvature_run
def _check_opts(case, name, thr, got, comps, what):
    """output components `comps` (of 5..16: GaussianCurvature, StrainRate, VelFlameNormal, ROST x 9): written, finite, within the bound;
    clipped GaussianCurvature and VelFlameNormal exact zeros"""
    core, ref = GCC.curv_ref(name, thr)
    out, _ = GCC.opts_ref(name, thr)
    for k in comps:
        label = GCC.OPT_NAMES[k - 5]
        st = Stat()
        for l, lv in enumerate(case.levels):
            f = GCC.opt_field(out[l], k)
            for b in range(lv.nboxes):
                a = got[l].valid(b)[k]
                _clean(a, f"{what} {label} level {l} box {b}")
                st.add(a, ref.valid(l, b, f.v), ref.valid(l, b, f.e), f"{what} {label} level {l} box {b}")
                if k in (5, 7):
                    m = ref.valid(l, b, core[l]["clip"])
                    assert (a[m] == 0.0).all(), f"{what} {label} level {l} box {b}: clipped cells are not zero"
        print(st.check_cap(f"GPU {what} {label}"))


def _state_valid_unchanged(case, name, dst, what):
    """the call fills ghost cells of the state in place; its valid cells are the uploaded bits"""
    want = GCC.pipe_states(name, 2, SENT_GPU, 4)
    for l, lv in enumerate(case.levels):
        h = dst[l].download()
        for b in range(lv.nboxes):
            assert bits_equal(h.valid(b), want[l].valid(b)), f"{what}: valid cells of the state changed, level {l} box {b}"


PATH1 = ("narrow", "sym", "ragged", "deep", "wide", "tall")


@pytest.mark.parametrize("clip", [False, True], ids=["nothr", "thr"])
@pytest.mark.parametrize("fused", [False, True], ids=["passes", "fused"])
@pytest.mark.parametrize("name,key,val", RUNS, ids=RUN_IDS)
def test_curvature_options_run(ctx, options, name, key, val, fused, clip):
    """every option on: GaussianCurvature, StrainRate, VelFlameNormal and the nine ROST components within the bound, the five core
    components within theirs, clipped cells zero, the state's valid cells untouched; the implementation the call took: 2 (Gaussian
    curvature inside the sweep) on `kgwide`, 1 (one options pass per level) on the cases named in PATH1, 0 pass by pass"""
    if key:
        options(**{key: val})
    case, dls, dst = _dev(ctx, name, 2, 4)
    thr = case.threshold if clip else None
    dout = [sentinel_out(ctx, dl, 17) for dl in dls]
    what = f"pa_curvature_run options {'fused' if fused else 'passes'} {name}{f' {key}={val}' if key else ''} thr {thr}"
    try:
        P = capi.curv_params(threshold=thr, fused=fused, do_gauss=True, do_strain=True, strain_tensor=True, do_velnormal=True, vel_comp=1)
        capi.curvature_run(ctx, dst, 0, case.bc, P, dout, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        path = ctx.lib.pa_curvature_last_path(ctx.h)
        print(f"GPU {what}: path {path}")
        if not fused:
            assert path == 0, f"{what}: path {path}"
        elif key is None and name == "kgwide":
            assert path == 2, f"{what}: path {path}, not the Gaussian curvature inside the sweep"
        elif key is None and name in PATH1:
            assert path == 1, f"{what}: path {path}, not the options pass"
        got = [d.download() for d in dout]
        _check_opts(case, name, thr, got, range(5, 17), what)
        _check_curv(case, name, thr, got, 0, 1, 2, what)
        _state_valid_unchanged(case, name, dst, what)
    finally:
        _close(dout + dst + dls)


SUBSETS = {
    "gauss": (dict(do_gauss=True), [5]),
    "strain": (dict(do_strain=True), [6]),
    "strain_tensor": (dict(do_strain=True, strain_tensor=True), [6] + list(range(8, 17))),
    "veln": (dict(do_velnormal=True), [7]),
    "strain_veln": (dict(do_strain=True, do_velnormal=True), [6, 7]),
}


@pytest.mark.parametrize("subset", list(SUBSETS))
@pytest.mark.parametrize("name", ["tall", "wide"])
def test_curvature_option_subsets(ctx, name, subset):
    """the options one by one and in pairs, fused, with the threshold: the launches of the options pass that `all options on` never makes
    (Gaussian curvature alone; strain without the tensor; strain with it and no Gaussian curvature; the normal velocity alone; strain
    + normal velocity).  The requested components lie within the bound; every component of an option that is off still holds the
    sentinel"""
    opts, comps = SUBSETS[subset]
    case, dls, dst = _dev(ctx, name, 2, 4)
    thr = case.threshold
    dout = [sentinel_out(ctx, dl, 17) for dl in dls]
    what = f"pa_curvature_run {subset} {name} thr {thr}"
    try:
        capi.curvature_run(ctx, dst, 0, case.bc, capi.curv_params(threshold=thr, fused=True, vel_comp=1, **opts), dout, 0)
        ctx.sync()
        assert ctx.bc_errors() == 0
        path = ctx.lib.pa_curvature_last_path(ctx.h)
        assert path == 1, f"{what}: path {path}, not the options pass"
        got = [d.download() for d in dout]
        _check_opts(case, name, thr, got, comps, what)
        _check_curv(case, name, thr, got, 0, 1, 2, what)
        for l in range(len(case.levels)):
            assert_untouched(got[l], [k for k in range(5, 17) if k not in comps], f"{what} level {l}")
        _state_valid_unchanged(case, name, dst, what)
    finally:
        _close(dout + dst + dls)
