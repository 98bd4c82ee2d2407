"""GPU tier: the composite-integral kernels (peleanalysis_amd/csrc/pa_integral.hip) through the C ABI, and integral3d.ex / rmsVel3d.ex
end to end, against the numpy restatement of integral.cpp / rmsVel.cpp (tests/integral_ref.py).  Row 0 (the measure) is compared with
== to the correctly rounded exact sum; every other slot S must satisfy |S - fsum(t)| <= n 2^-53 sum|t| over the terms t the restatement
adds into it; the same input must give the same BITS on every run, for a re-tiled level, for a shuffled box order, for the uncombined
kernel and for every grouping of the variables.  Every slot of every row is compared."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import fixed192_ref as F
import integral_ref as I
import stats_ref as R
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, field_flame, nested_hierarchy, regrid_copy, retile_level
from peleanalysis_amd.plotfile import write_plotfile
from util import bits_equal, make_states

pytestmark = pytest.mark.gpu

HIERS = R.stats_hierarchies()
KIND_DIR = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0)]


def _sub(states, comps):
    out = []
    for s in states:
        m = MultiFab(s.level, len(comps), 0)
        for b in range(s.level.nboxes):
            m.valid(b)[...] = s.valid(b)[list(comps)]
        out.append(m)
    return out


def _vabs(states, comps, fl):
    """the magnitude of the finite values of every component over the levels that are integrated"""
    out = []
    for c in comps:
        m = 0.0
        for l in range(fl + 1):
            v = np.abs(states[l].valid_concat(c))
            v = v[np.isfinite(v)]
            m = max(m, float(v.max()) if len(v) else 0.0)
        out.append(m)
    return out


def gpu_integral(ctx, H, states, comps, kind, dir_=0, finest_level=None, ccomp=-1, cmin=0.0, cmax=0.0, squares=False, uncombined=False, vabs=None):
    """the level loops of integral.cpp:20-44, :79-101, :123-140 on the device -> the raw sums [rows] + shape, with the magnitudes declared at
    begin in .declared"""
    fl = H.nlev - 1 if finest_level is None else finest_level
    rr, Rl = R.ref_ratios(H), I.cum_ratios(H, fl)
    w = [I.level_weight(H.levels[l], kind, dir_) for l in range(fl + 1)]
    sub = _sub(states[:fl + 1], comps)
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels[:fl + 1]]
    vabs = [float(v) for v in (_vabs(states, comps, fl) if vabs is None else vabs)]
    with capi.IntegralAcc(ctx, len(comps), kind, dir_, I.domain_box(H, fl), squares) as acc:
        acc.begin(max(w), vabs)
        for l in (range(fl + 1) if kind == 3 else range(fl, -1, -1)):
            with capi.DevMF.from_host(ctx, dls[l], sub[l]) as mf:
                acc.add_level(mf, dls[l + 1] if l < fl else None, rr[l] if l < fl else 1, Rl[l], w[l], ccomp, cmin, cmax, uncombined=uncombined)
        out = acc.read().view(IntegralSums)
    for dl in dls:
        dl.close()
    out.declared = dict(w_max=max(w), vabs=vabs, squares=squares)
    return out


class IntegralSums(np.ndarray):
    """the array pa_integral_read fills, with the magnitudes declared at begin in .declared"""
    declared = None


def check_integral(res, got, H, what, bound=True):
    """row 0 == the correctly rounded exact sum; rows 1..: the contract's bound in every slot AND equal, bit for bit, to the big-integer model at
    the scales of the declared magnitudes (== fsum where the terms convert exactly); the IEEE rule where a term is not finite.
    bound=False (tests/test_gpu_fixed_sums.py only): inputs with terms below the quantum 2^(k-157), which the accumulator truncates by design --
    the model includes that, the bound presumes terms it can hold"""
    assert got.shape == (res["nrows"],) + res["shape"], (what, got.shape)
    ns = res["nslots"]
    s_w, s_row = F.integral_scales(**got.declared)
    F.assert_bins_match_model(np.asarray(got[0]), res["keys"], res["terms"][0], s_w, ns, f"{what} measure")
    assert np.array_equal(got[0], I.measure_exact(res, H)), f"{what}: the measure is not the correctly rounded exact sum"
    worst = 0.0
    for r in range(1, res["nrows"]):
        S = got[r].ravel().copy()
        special, k, t = I.split_nonfinite(res["keys"], res["terms"][r], ns)
        for s, v in special.items():
            assert (math.isnan(v) and math.isnan(S[s])) or S[s] == v, f"{what} row {r} slot {s}: {S[s]} where IEEE addition gives {v}"
            S[s] = 0.0
        if bound:
            worst = max(worst, R.assert_sum_bound(S, k, t, ns, f"{what} row {r}"))
        F.assert_bins_match_model(S, k, t, s_row[r - 1], ns, f"{what} row {r}")
    return worst


# ----------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name", sorted(HIERS))
@pytest.mark.parametrize("kind,dir_", KIND_DIR)
@pytest.mark.parametrize("cond", [False, True])
def test_integral_matches_the_restatement(ctx, name, kind, dir_, cond):
    H = HIERS[name]
    st = make_states(H, 3, 0, field_flame, seed=11)
    kw = dict(ccomp=2, cmin=400.0, cmax=1900.0) if cond else {}
    for fl in sorted({H.nlev - 1, max(H.nlev - 2, 0), 0}, reverse=True):
        res = I.integrate(H, st, [1, 0, 2], kind, dir_, finest_level=fl, **kw)
        assert len(res["keys"]) > 0
        got = gpu_integral(ctx, H, st, [1, 0, 2], kind, dir_, finest_level=fl, **kw)
        worst = check_integral(res, got, H, f"{name} kind={kind} dir={dir_} cond={cond} finestLevel={fl}")
        print(f"{name} kind={kind} dir={dir_} cond={cond} finestLevel={fl}: worst |S - fsum| / bound = {worst:.3f}")


@pytest.mark.parametrize("nv", [1, 4, 5, 8])
def test_every_variable_count(ctx, nv):
    H = HIERS["union"]
    st = make_states(H, 8, 0, field_flame, seed=13)
    comps = list(range(nv))
    for kind, dir_ in ((3, 0), (2, 2), (1, 0)):
        res = I.integrate(H, st, comps, kind, dir_, ccomp=nv - 1, cmin=350.0, cmax=2100.0)
        check_integral(res, gpu_integral(ctx, H, st, comps, kind, dir_, ccomp=nv - 1, cmin=350.0, cmax=2100.0), H, f"nv={nv} kind={kind}")


def test_wide_boxes_whose_rows_fill_wavefronts(ctx):
    """boxes 64 cells wide: the lanes of a wavefront share the slot (kind 3; kind 2 with dir != x; kind 1 with dir = x), their runs are
    summed in integers before one lane adds -- against the restatement, and the same bits as the uncombined kernel"""
    H = nested_hierarchy(64, 2, 64)
    assert all(((lv.boxes[:, 3] - lv.boxes[:, 0] + 1) % 64 == 0).all() for lv in H.levels)
    st = make_states(H, 4, 0, field_flame, seed=17)
    for kind, dir_ in KIND_DIR:
        for kw in ({}, dict(ccomp=3, cmin=450.0, cmax=2300.0)):
            res = I.integrate(H, st, [0, 1, 2, 3], kind, dir_, **kw)
            got = gpu_integral(ctx, H, st, [0, 1, 2, 3], kind, dir_, **kw)
            check_integral(res, got, H, f"wide boxes kind={kind} dir={dir_} {kw}")
            assert bits_equal(got, gpu_integral(ctx, H, st, [0, 1, 2, 3], kind, dir_, uncombined=True, **kw))


@pytest.mark.parametrize("nv", [1, 3, 8])
def test_squares_rows(ctx, nv):
    """the rows (v * v) * w of rmsVel.cpp:109-111, composite or -- as rmsVel uses them -- one level without a mask"""
    H = HIERS["nested"]
    st = make_states(H, 8, 0, field_flame, seed=14)
    comps = list(range(nv))
    for kind, dir_ in ((3, 0), (2, 1), (1, 2)):
        res = I.integrate(H, st, comps, kind, dir_, squares=True)
        assert res["nrows"] == 1 + 2 * nv
        check_integral(res, gpu_integral(ctx, H, st, comps, kind, dir_, squares=True), H, f"squares nv={nv} kind={kind}")
    for H2, st2, _ in I.rmsvel_cases():
        r = I.rmsvel(H2, st2)
        fl = r["level"]
        lev = H2.levels[fl]
        H1 = Hierarchy([lev], 2)
        got = gpu_integral(ctx, H1, [st2[fl]], [0, 1, 2], 3, 0, squares=True)
        assert got.shape == (7,)
        assert got[0] == math.fsum(r["terms"][0])
        for q in range(1, 7):
            R.assert_sum_bound(got[q:q + 1], r["keys"], r["terms"][q], 1, f"rmsVel sum {q}")
            F.assert_bins_match_model(np.asarray(got[q:q + 1]), r["keys"], r["terms"][q], F.integral_scales(**got.declared)[1][q - 1], 1, f"rmsVel sum {q}")


def test_nonfinite_terms_follow_ieee_addition(ctx):
    """NaN, +inf and -inf terms: sticky flags per slot and row; NaN or both infinities give NaN, one infinity gives itself, the other
    slots and rows keep their finite sums; a NaN in the condition variable fails the window"""
    H = nested_hierarchy(16, 2, 8)
    st = make_states(H, 3, 0, field_flame, seed=15)
    fine, coarse = st[1], st[0]
    fine.valid(0)[0, 1, 2, 3] = np.nan
    fine.valid(1)[0, 2, 2, 2] = np.inf
    fine.valid(2)[0, 3, 3, 3] = -np.inf
    fine.valid(3)[1, 4, 4, 4] = np.inf
    fine.valid(3)[1, 4, 4, 5] = -np.inf
    coarse.valid(0)[1, 0, 0, 0] = np.inf   # a coarse cell: the flag reaches every fine slot under it
    coarse.valid(0)[2, 1, 1, 1] = np.nan  # the condition variable
    for kind, dir_ in KIND_DIR:
        for kw in ({}, dict(ccomp=2, cmin=-1e300, cmax=1e300)):
            res = I.integrate(H, st, [0, 1, 2], kind, dir_, squares=True, **kw)
            nf = sum(int((~np.isfinite(t)).sum()) for t in res["terms"])
            assert nf >= 6
            got = gpu_integral(ctx, H, st, [0, 1, 2], kind, dir_, squares=True, **kw)
            check_integral(res, got, H, f"non-finite kind={kind} dir={dir_} {kw}")
            unc = gpu_integral(ctx, H, st, [0, 1, 2], kind, dir_, squares=True, uncombined=True, **kw)
            assert bits_equal(got, unc)
    got = gpu_integral(ctx, H, st, [0, 1, 2], 3, 0)
    assert math.isnan(got[1]) and math.isnan(got[2])  # a NaN among the terms; both infinities among the terms


def test_wide_span_component(ctx):
    """values from 1e-14 to 1 in one component: every bit of every term down to 2^-105 of the declared magnitude is kept, so the bound of
    the ordinary case holds, which implies the coarser n^2 2^-53 max|t|"""
    H = HIERS["nested"]
    st = make_states(H, 3, 0, field_flame, seed=9)
    for l, s in enumerate(st):
        rng = np.random.default_rng(40 + l)
        for b in range(s.level.nboxes):
            v = s.valid(b)
            v[1] = 10.0 ** rng.uniform(-14, 0, size=v[1].shape)
            v[2] = -(10.0 ** rng.uniform(-14, 0, size=v[1].shape)) * np.sign(rng.uniform(-1, 3, size=v[1].shape))
    for kind, dir_ in ((3, 0), (2, 0), (2, 2), (1, 1)):
        res = I.integrate(H, st, [0, 1, 2], kind, dir_, squares=True)
        got = gpu_integral(ctx, H, st, [0, 1, 2], kind, dir_, squares=True)
        check_integral(res, got, H, f"wide span kind={kind} dir={dir_}")
        for r in (2, 3):
            R.assert_sum_bound(got[r], res["keys"], res["terms"][r], res["nslots"], "wide span, coarse bound", coarse=True)


# ----------------------------------------------------------------------------- reproducibility
def _retiled(H, states, how):
    levels, out = [], []
    for l, lv in enumerate(H.levels):
        if how == "retile":
            nl = retile_level(lv, (32, 16, 32), 3)
        else:
            perm = np.random.default_rng(70 + l).permutation(lv.nboxes)
            nl = Level(lv.boxes[perm], lv.domlo, lv.domhi, lv.is_per, lv.prob_lo, lv.prob_hi)
        s = MultiFab(nl, states[l].ncomp, 0)
        regrid_copy(states[l], s)
        levels.append(nl)
        out.append(s)
    return Hierarchy(levels, H.ref_ratio), out


@pytest.mark.parametrize("name", sorted(HIERS))
def test_same_bits_on_every_run_tiling_box_order_and_kernel(ctx, name):
    H = HIERS[name]
    st = make_states(H, 4, 0, field_flame, seed=12)
    comps = [0, 1, 2, 3]
    kw = dict(ccomp=0, cmin=350.0, cmax=1800.0, squares=True)
    first = {kd: gpu_integral(ctx, H, st, comps, *kd, **kw) for kd in KIND_DIR}
    variants = [("second run", H, st, False), ("uncombined kernel", H, st, True)]
    for how in ("retile", "shuffle"):
        H2, st2 = _retiled(H, st, how)
        variants.append((how, H2, st2, False))
    for what, H2, st2, unc in variants:
        for kd in KIND_DIR:
            got = gpu_integral(ctx, H2, st2, comps, *kd, uncombined=unc, **kw)
            assert bits_equal(got, first[kd]), f"{name}, {what}, kind {kd[0]} dir {kd[1]}: the sums differ in their bits"


def test_same_bits_for_every_grouping_of_nine_variables(ctx):
    """9 variables as 8 + 1 (what integral3d does) against other groupings and against every variable on its own"""
    H = HIERS["union"]
    st = make_states(H, 9, 0, field_flame, seed=16)
    for kind, dir_ in ((3, 0), (2, 1), (1, 0)):
        def rows(groups):
            out = {}
            for g in groups:
                got = gpu_integral(ctx, H, st, g, kind, dir_)
                for q, c in enumerate(g):
                    out[c] = got[1 + q]
                out["m"] = got[0] if "m" not in out else out["m"]
                assert bits_equal(out["m"], got[0])
            return out
        a = rows([list(range(8)), [8]])
        b = rows([[0, 1, 2, 3], [4, 5, 6, 7, 8]])
        c = rows([[q] for q in range(9)])
        for q in list(range(9)) + ["m"]:
            assert bits_equal(a[q], b[q]) and bits_equal(a[q], c[q]), f"kind {kind}: variable {q} depends on its group"


# ----------------------------------------------------------------------------- error paths
def test_error_paths(ctx):
    H = nested_hierarchy(16, 2, 8)
    st = make_states(H, 3, 0, field_flame)
    dom1, dom0 = I.domain_box(H, 1), I.domain_box(H, 0)
    with pytest.raises(capi.PaError, match="kind must be 1"):
        capi.IntegralAcc(ctx, 2, 0, 0, dom1)
    with pytest.raises(capi.PaError, match="kind must be 1"):
        capi.IntegralAcc(ctx, 2, 4, 0, dom1)
    with pytest.raises(capi.PaError, match="dir must be 0, 1 or 2"):
        capi.IntegralAcc(ctx, 2, 2, 3, dom1)
    with pytest.raises(capi.PaError, match="dir must be 0, 1 or 2"):
        capi.IntegralAcc(ctx, 2, 1, -1, dom1)
    with pytest.raises(capi.PaError, match="1 to 8 variables"):
        capi.IntegralAcc(ctx, 9, 3, 0, dom1)
    with pytest.raises(capi.PaError, match="1 to 8 variables"):
        capi.IntegralAcc(ctx, 0, 3, 0, dom1)
    dl0, dl1 = capi.DevLevel(ctx, H.levels[0]), capi.DevLevel(ctx, H.levels[1])
    mf0, mf1 = capi.DevMF.from_host(ctx, dl0, st[0]), capi.DevMF.from_host(ctx, dl1, st[1])
    w = [I.level_weight(lv, 2, 0) for lv in H.levels]
    with capi.IntegralAcc(ctx, 3, 2, 0, dom1) as acc:
        with pytest.raises(capi.PaError, match="pa_integral_begin has not been called"):
            acc.add_level(mf1, None, 1, 1, w[1])
        with pytest.raises(capi.PaError, match="pa_integral_begin has not been called"):
            acc.read()
        with pytest.raises(capi.PaError, match="w_max must be positive"):
            acc.begin(0.0, [1.0] * 3)
        with pytest.raises(capi.PaError, match="magnitude of variable 1 is not finite"):
            acc.begin(w[0], [1.0, float("inf"), 1.0])
        acc.begin(w[0], [3000.0] * 3)
        with pytest.raises(capi.PaError, match="condition component must be one of the 3"):
            acc.add_level(mf1, None, 1, 1, w[1], ccomp=3, cmin=0.0, cmax=1.0)
        with pytest.raises(capi.PaError, match="is not the domain the accumulator was created for"):
            acc.add_level(mf0, dl1, 2, 1, w[0])   # level 0 with R_l = 1: its domain does not refine to the declared one
        with pytest.raises(capi.PaError, match="is not the domain the accumulator was created for"):
            acc.add_level(mf1, None, 1, 2, w[1])
        with pytest.raises(capi.PaError, match="weight must be positive"):
            acc.add_level(mf1, None, 1, 1, 2.0 * w[0])
        with pytest.raises(capi.PaError, match="must hold 3 components"):
            with capi.DevMF(ctx, dl1, 2, 0) as small:  # an input, refused for its component count before anything reads it
                acc.add_level(small, None, 1, 1, w[1])
        # a scale taken from a magnitude the data exceed: the read fails instead of returning a wrapped sum
        acc.begin(w[0], [1.0] * 3)
        acc.add_level(mf1, None, 1, 1, w[1])
        with pytest.raises(capi.PaError, match="exceeds the magnitude declared"):
            acc.read()
        # ... and the object is usable again after the next begin
        acc.begin(w[0], [3000.0] * 3)
        acc.add_level(mf1, None, 1, 1, w[1])
        acc.add_level(mf0, dl1, 2, 2, w[0])
        res = I.integrate(H, st, [0, 1, 2], 2, 0)
        got = acc.read().view(IntegralSums)
        got.declared = dict(w_max=w[0], vabs=[3000.0] * 3, squares=False)
        check_integral(res, got, H, "after a failed read")
    with capi.IntegralAcc(ctx, 1, 3, 0, dom0) as acc:  # finestLevel = 0: level 1 does not belong
        acc.begin(1.0, [3000.0])
        with pytest.raises(capi.PaError, match="is not the domain the accumulator was created for"):
            acc.add_level(mf1, None, 1, 1, 1e-3)
    for o in (mf0, mf1, dl0, dl1):
        o.close()


# ----------------------------------------------------------------------------- device memory
def test_device_memory_of_the_accumulators_comes_back(ctx):
    """the pattern of tests/test_gpu_leaks.py for pa_integral: create / add / read / destroy cycles leave the free memory of the device
    where it was after the second one"""
    torch = pytest.importorskip("torch")
    H = HIERS["nested"]
    st = make_states(H, 4, 0, field_flame)

    def cycle():
        for kd in KIND_DIR:
            gpu_integral(ctx, H, st, [0, 1, 2, 3], *kd, squares=True)
        ctx.sync()

    for _ in range(2):
        cycle()
    torch.cuda.synchronize()
    free2, _ = torch.cuda.mem_get_info(0)
    for _ in range(4):
        cycle()
    torch.cuda.synchronize()
    free6, _ = torch.cuda.mem_get_info(0)
    assert free2 - free6 <= 4 << 20, f"{(free2 - free6) / 2**20:.1f} MiB of device memory did not come back"


# ----------------------------------------------------------------------------- integral3d.ex / rmsVel3d.ex end to end
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")
NAMES = ["temp", "Y(H2)", "HeatRelease", "density"]


def _tool(exe, args, cwd):
    return subprocess.run([os.path.join(BIN, exe)] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


@pytest.fixture(scope="module")
def plotfiles(tmp_path_factory):
    d = tmp_path_factory.mktemp("integral")
    out = {}
    for name in ("nested", "union", "ratio4"):
        H = HIERS[name]
        st = make_states(H, 4, 0, field_flame, seed=21)
        p = str(d / f"plt_{name}")
        write_plotfile(p, H, st, NAMES, time=0.5)
        out[name] = (p, H, st)
    return out


def brackets(res, avg):
    """the finished array at both ends of the contract's bound: rows 1.. = fsum -+ n 2^-53 sum|t| (one step outwards for the rounding
    of the end itself), divided by the exact measure where avg asks for it.  Division by a positive number is monotone, so the tool's
    quotient of a sum inside the bound lies between the quotients of the ends."""
    ns = res["nslots"]
    m = I.measure_exact(res, None).ravel()
    lo, hi = [m], [m]
    for r in range(1, res["nrows"]):
        ex, sa, n, _ = R.fsum_by_bin(res["keys"], res["terms"][r], ns)
        d = n * R.EPS * sa
        a = np.where(d > 0, np.nextafter(ex - d, -np.inf), ex)
        b = np.where(d > 0, np.nextafter(ex + d, np.inf), ex)
        if avg:
            with np.errstate(all="ignore"):
                a, b = np.where(m > 0, a / m, a), np.where(m > 0, b / m, b)
        lo.append(a)
        hi.append(b)
    sh = (res["nrows"],) + res["shape"]
    return np.array(lo).reshape(sh), np.array(hi).reshape(sh)


def compare_tokens(got, lo, hi, what):
    """the tool's text against the restatement's writer at both ends: the same layout, and every %e token inside [fmt(lo), fmt(hi)]
    -> (tokens, of which not identical in all three)"""
    shape = lambda t: re.sub(r"[^\s]+", "#", t)
    assert shape(got) == shape(lo) == shape(hi), f"{what}: layout differs"
    n = nn = 0
    for q, (g, a, b) in enumerate(zip(got.split(), lo.split(), hi.split())):
        n += 1
        if g == a == b:
            continue
        nn += 1
        assert min(float(a), float(b)) <= float(g) <= max(float(a), float(b)), f"{what}: token {q}: {g} outside [{a}, {b}]"
    return n, nn


def check_files(outfile, kind, dir_, names, res, H, fl, avg, listing_dir):
    lo, hi = brackets(res, avg)
    want_lo = I.integral_files(outfile, kind, dir_, names, lo, H, fl)
    want_hi = I.integral_files(outfile, kind, dir_, names, hi, H, fl)
    made = sorted(os.path.join(listing_dir, f) for f in os.listdir(listing_dir) if f.startswith(os.path.basename(outfile) + "_") and os.path.isfile(os.path.join(listing_dir, f)))
    assert made == sorted(want_lo), (made, sorted(want_lo))
    ntok = 0
    for fn in want_lo:
        txt = open(fn).read()
        n, nn = compare_tokens(txt, want_lo[fn], want_hi[fn], os.path.basename(fn))
        if fn.endswith("_x.dat") or fn.endswith("_y.dat") or fn.endswith("_length.dat"):
            assert txt == want_lo[fn], f"{fn}: exact bytes"
        ntok += n
    return ntok


@pytest.mark.parametrize("name", ["nested", "union", "ratio4"])
def test_integral_tool_end_to_end(plotfiles, name):
    p, H, st = plotfiles[name]
    d = os.path.dirname(p)
    fl = H.nlev - 1
    # kind 3: one line; twice the same bytes
    res = I.integrate(H, st, [0, 3], 3)
    r = _tool("integral3d.ex", ["infile=" + p, "vars=temp density", "integralDimension=3"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout == I.integral_stdout(p, ["temp", "density"], 3, H.nlev)
    out3 = I.outfile_name(p, 3, 0)
    assert check_files(out3, 3, 0, ["temp", "density"], res, H, fl, 0, d) == 3
    txt = open(out3 + "_allVars.dat").read()
    assert not txt.endswith("\n")
    assert _tool("integral3d.ex", ["infile=" + p, "vars=temp density", "integralDimension=3"], d).returncode == 0 and open(out3 + "_allVars.dat").read() == txt
    os.remove(out3 + "_allVars.dat")
    # kind 2, every direction, the planar average conditioned on a window
    for d1, d2 in ((1, 2), (2, 0), (1, 0)):
        dir_ = 3 - d1 - d2
        res = I.integrate(H, st, [0, 1, 2], 2, dir_, ccomp=0, cmin=400.0, cmax=1900.0)
        args = ["infile=" + p, "vars=temp Y(H2) HeatRelease", "integralDimension=2", f"dir1={d1}", f"dir2={d2}", "cVar=temp", "cMin=400", "cMax=1900", "avg=1"]
        r = _tool("integral3d.ex", args, d)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout == I.integral_stdout(p, NAMES[:3], 2, H.nlev)
        out2 = I.outfile_name(p, 2, dir_, "temp", 400.0, 1900.0, 1)
        assert out2 == f"{p}_integral_dir{dir_}_ctemp_400.000000_1900.000000_avg"
        n = check_files(out2, 2, dir_, NAMES[:3], res, H, fl, 1, d)
        assert n == 5 * res["nslots"]
        for f in os.listdir(d):
            if f.startswith(os.path.basename(out2)):
                os.remove(os.path.join(d, f))
    # kind 1, every direction, a lower finestLevel
    for dir_, lev in ((0, fl), (1, fl), (2, max(fl - 1, 0))):
        res = I.integrate(H, st, [3, 0], 1, dir_, finest_level=lev)
        r = _tool("integral3d.ex", ["infile=" + p, "vars=density temp", "integralDimension=1", f"dir={dir_}", f"finestLevel={lev}"], d)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout == I.integral_stdout(p, ["density", "temp"], 1, lev + 1)
        out1 = I.outfile_name(p, 1, dir_)
        n = check_files(out1, 1, dir_, ["density", "temp"], res, H, lev, 0, d)
        assert n == 3 * res["nslots"] + sum(res["shape"])
        for f in os.listdir(d):
            if f.startswith(os.path.basename(out1)):
                os.remove(os.path.join(d, f))


def test_integral_tool_nine_variables_in_two_groups(tmp_path):
    """more than 8 variables: groups of at most 8; every variable's row is what a run of that variable alone writes"""
    H = HIERS["nested"]
    names = [f"v{q}" for q in range(9)]
    st = make_states(H, 9, 0, field_flame, seed=22)
    p = str(tmp_path / "plt9")
    write_plotfile(p, H, st, names, time=0.0)
    for extra in ([], ["cVar=v8", "cMin=400", "cMax=2200"], ["cVar=v0", "cMin=400", "cMax=2200"]):
        r = _tool("integral3d.ex", ["infile=" + p, "vars=" + " ".join(names), "integralDimension=2", "dir1=0", "dir2=1"] + extra, tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout == I.integral_stdout(p, names, 2, H.nlev)
        cv = extra[0][5:] if extra else ""
        base = I.outfile_name(p, 2, 2, cv, 400.0, 2200.0, 0)
        rows = open(base + "_allVars.dat").read().splitlines()
        assert len(rows) == 10
        kw = dict(ccomp=names.index(cv), cmin=400.0, cmax=2200.0) if extra else {}
        res = I.integrate(H, st, list(range(9)), 2, 2, **kw)
        check_files(base, 2, 2, names, res, H, H.nlev - 1, 0, str(tmp_path))
        for q in (0, 7, 8):
            vs = [names[q]] + ([cv] if extra and cv != names[q] else [])
            r1 = _tool("integral3d.ex", ["infile=" + p, "vars=" + " ".join(vs), "integralDimension=2", "dir1=0", "dir2=1"] + extra, tmp_path)
            assert r1.returncode == 0, r1.stdout + r1.stderr
            alone = open(base + "_allVars.dat").read().splitlines()
            assert alone[0] == rows[0] and alone[1] == rows[1 + q], f"variable {q} depends on its group"
        for f in os.listdir(tmp_path):
            if f.startswith("plt9_integral"):
                os.remove(tmp_path / f)


def test_integral_tool_ppm(plotfiles):
    """a pixel must equal the colour map applied to the lower or to the upper end of its bracket; the share of pixels where the two
    differ is a condition on the test image (at most 0.1 %), asserted from the restatement alone before the tool's output is looked at"""
    H, st = I.ppm_case()
    d = os.path.dirname(plotfiles["nested"][0])
    p = os.path.join(d, "plt_ppm")
    write_plotfile(p, H, st, ["temp", "fuel"], time=0.0)
    for dir_, gpm, avg in ((0, 1, 1), (2, 0, 1), (1, 1, 0)):
        res = I.integrate(H, st, [0, 1], 1, dir_)
        npx, differ, ends = I.ppm_bracket_pixels(res, avg=bool(avg), go_past_max=gpm)
        assert npx > 0 and differ <= 0.001 * npx
        args = ["infile=" + p, "vars=temp fuel", "integralDimension=1", f"dir={dir_}", "format=ppm", f"goPastMax={gpm}", f"avg={avg}"]
        r = _tool("integral3d.ex", args, d)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout == I.integral_stdout(p, ["temp", "fuel"], 1, H.nlev, fmt="ppm")
        base = I.outfile_name(p, 1, dir_, avg=avg)
        made = sorted(f for f in os.listdir(d) if f.startswith(os.path.basename(base) + "_"))
        assert made == sorted(os.path.basename(base) + s for s in ("_length.ppm", "_temp.ppm", "_fuel.ppm"))
        n1, n2 = res["shape"]
        head = ("P6\n%i %i\n255\n" % (n2, n1)).encode()
        # the measure is the same exact number in every pixel: vMax == vMin, the quotient is NaN, the colour 1.5
        want = head + bytes([255, 255, 255] if gpm == 1 else [128, 0, 0]) * (n1 * n2)
        assert open(base + "_length.ppm", "rb").read() == want
        for q, nm in enumerate(("temp", "fuel")):
            raw = open(base + "_" + nm + ".ppm", "rb").read()
            assert raw[:len(head)] == head and len(raw) == len(head) + 3 * n1 * n2
            px = np.frombuffer(raw[len(head):], np.uint8).reshape(n1, n2, 3)[::-1].reshape(n1 * n2, 3)  # undo the row flip
            ok = np.all(px == ends[q][0], axis=1) | np.all(px == ends[q][1], axis=1)
            assert ok.all(), f"{nm}: {int((~ok).sum())} pixels match neither end of their bracket"
        for f in made:
            os.remove(os.path.join(d, f))
    # useminmaxN counts from 1 and leaves the other variables on the file's values
    r = _tool("integral3d.ex", ["infile=" + p, "vars=temp fuel", "integralDimension=1", "dir=2", "format=ppm", "useminmax2=500 1500"], d)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout == I.integral_stdout(p, ["temp", "fuel"], 1, H.nlev, fmt="ppm", useminmax={2: (500.0, 1500.0)})
    res = I.integrate(H, st, [0, 1], 1, 2)
    lo, hi = brackets(res, 0)
    base = I.outfile_name(p, 1, 2)
    raw = open(base + "_fuel.ppm", "rb").read()
    ends = [I.write_ppm(e[2], 1, 500.0, 1500.0) for e in (lo, hi)]
    a, b, c = (np.frombuffer(t[-3 * res["nslots"]:], np.uint8).reshape(-1, 3) for t in (raw, ends[0], ends[1]))
    assert (np.any(b != c, axis=1)).sum() <= 0.001 * len(b)
    assert np.all(np.all(a == b, axis=1) | np.all(a == c, axis=1))
    r = _tool("integral3d.ex", ["infile=" + p, "vars=temp fuel", "integralDimension=1", "dir=2", "format=ppm", "useminmax1=1 2 3"], d)
    assert r.returncode != 0 and "Need to specify 2 values for useMinMax" in r.stderr


def test_integral_tool_deviation_aborts(plotfiles, tmp_path):
    p, H, st = plotfiles["nested"]
    ok = ["infile=" + p, "vars=temp density"]
    for args, msg in ((ok + ["integralDimension=3", "cVar=temp", "cMin=300"], "cVar needs both cMin and cMax"),
                      (ok + ["integralDimension=3", "cVar=temp", "cMax=300"], "cVar needs both cMin and cMax"),
                      (ok + ["integralDimension=3", "cVar=Y(H2)", "cMin=0", "cMax=1"], "cVar not in list of vars!"),
                      (ok + ["integralDimension=4"], "integralDimension must be 1, 2 or 3"),
                      (ok + ["integralDimension=0"], "integralDimension must be 1, 2 or 3"),
                      (ok + ["integralDimension=1", "dir=3"], "dir must be 0, 1 or 2"),
                      (ok + ["integralDimension=1", "dir=0", "format=png"], "format must be dat or ppm"),
                      (ok + ["integralDimension=2", "dir1=1", "dir2=1"], "two different directions"),
                      (ok + ["integralDimension=2", "dir1=0", "dir2=3"], "two different directions"),
                      (["infile=" + p, "integralDimension=3"], "need to specify vars"),
                      (["infile=" + p, "vars=temp nosuch", "integralDimension=3"], "variable nosuch is not in"),
                      (ok + ["integralDimension=3", "finestLevel=7"], "finestLevel out of range"),
                      (ok + ["integralDimension=3", "ngpus=2"], "ngpus > 1 is not supported")):
        r = _tool("integral3d.ex", args, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stdout[-300:], r.stderr)
    # an output file that cannot be opened: a directory stands where it goes
    os.makedirs(p + "_integral_allVars.dat")
    r = _tool("integral3d.ex", ok + ["integralDimension=3"], tmp_path)
    os.rmdir(p + "_integral_allVars.dat")
    assert r.returncode != 0 and "Unable to create" in r.stderr
    lev = Level([[0, 0, 0, 7, 7, 0]], (0, 0, 0), (7, 7, 0), (0, 0, 0), np.zeros(3), np.ones(3))
    write_plotfile(str(tmp_path / "plt2d"), Hierarchy([lev], 2), [MultiFab(lev, 3, 0)], ["x_velocity", "y_velocity", "z_velocity"], dim=2)
    for exe, args in (("integral3d.ex", ["infile=" + str(tmp_path / "plt2d"), "vars=x_velocity", "integralDimension=2"]), ("rmsVel3d.ex", ["infiles=" + str(tmp_path / "plt2d")])):
        r = _tool(exe, args, tmp_path)
        assert r.returncode != 0 and "only 3-D plotfiles are supported" in r.stderr
    r = _tool("rmsVel3d.ex", ["infiles=" + p], tmp_path)
    assert r.returncode != 0 and "variable x_velocity is not in" in r.stderr
    r = _tool("rmsVel3d.ex", ["infiles=" + p, "ngpus=2"], tmp_path)
    assert r.returncode != 0 and "ngpus > 1 is not supported" in r.stderr


def test_rmsvel_tool_over_two_plotfiles(tmp_path):
    """the subtraction ux2 - uxb*uxb cancels: the file's urms must lie within 8 kappa 2^-53 relative of the restatement's value, kappa
    the condition number the restatement computes; the fields keep kappa <= 1e6 (asserted), far below the seven printed digits"""
    cases = I.rmsvel_cases()
    names = ["x_velocity", "y_velocity", "z_velocity", "temp"]
    paths = []
    for q, (H, st, t) in enumerate(cases):
        p = str(tmp_path / f"plt{q}")
        write_plotfile(p, H, st, names, time=t)
        paths.append(p)
    for fl, shown in ((None, [None, None]), (1, [1, 1]), (5, [None, None])):
        ref = [I.rmsvel(H, st, finest_level=fl) for H, st, _ in cases]
        assert all(r["kappa"] <= 1e6 for r in ref)
        r = _tool("rmsVel3d.ex", ["infiles=" + " ".join(paths)] + ([f"finestLevel={fl}"] if fl is not None else []), tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout == I.rmsvel_stdout(paths, shown)
        lines = open(tmp_path / "RmsVel.dat").read().splitlines(True)
        assert len(lines) == 2 and all(l.endswith("\n") for l in lines)
        for line, rr, (_, _, t) in zip(lines, ref, cases):
            tt, uu = line.split()
            assert re.fullmatch(r"\d\.\d{6}e[+-]\d\d \d\.\d{6}e[+-]\d\d\n", line)
            assert tt == "%e" % t
            tol = 8 * rr["kappa"] * R.EPS
            assert tol < 1e-8
            lo, hi = "%e" % (rr["urms"] * (1 - tol)), "%e" % (rr["urms"] * (1 + tol))
            assert float(lo) <= float(uu) <= float(hi), f"urms {uu} outside [{lo}, {hi}]"
    # the boxes of finestLevel only: the level's own cells, covered or not -- not the composite
    H, st, _ = cases[0]
    assert len(I.rmsvel(H, st)["keys"]) == H.levels[-1].ncells
