"""GPU tier: the binned-statistics kernels (peleanalysis_amd/csrc/pa_stats.hip) through the C ABI against the numpy restatement of
jpdf.cpp / conditionalMean.cpp (tests/stats_ref.py).  Exact parts (axis minima / maxima, bin indices = the set of non-empty bins, the
out-of-range counters, binHits, per-bin minima and maxima) are compared with ==; every sum S of a bin must satisfy
|S - fsum(t)| <= n 2^-53 sum|t| over the terms t the restatement adds into that bin; the same input must give the same BITS on every
run, for a re-tiled level, for a shuffled box order and for the uncombined kernel.  Every bin of every accumulator is compared."""
import numpy as np
import pytest

import fixed192_ref as F
import stats_ref as R
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, field_flame, nested_hierarchy, regrid_copy, retile_level
from util import bits_equal, make_states

pytestmark = pytest.mark.gpu

HIERS = R.stats_hierarchies()
STOICH_ABS = 2.0 ** 40  # declared magnitude of the stoichiometry variable (its axis is 0 .. 2, its values are whatever the data give)


def _vol(lev):
    dx = lev.dx
    v = dx[0] * dx[1]
    return v * dx[2]


def gpu_minmax(ctx, H, states, comps, fl):
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels[:fl + 1]]
    mn, mx = np.full(len(comps), np.inf), np.full(len(comps), -np.inf)
    for l, dl in enumerate(dls):
        with capi.DevMF.from_host(ctx, dl, states[l]) as mf:
            a, b = capi.minmax_comps_level(ctx, mf, comps)
        mn, mx = np.minimum(mn, a), np.maximum(mx, b)
    for dl in dls:
        dl.close()
    return mn, mx


def gpu_jpdf(ctx, H, states, nload, nbins, vmin, vmax, finest_level=None, uncombined=False, vabs=None, **kw):
    """the level loop of jpdf.cpp:440-522 on the device -> (bin, binX1, binX2 [npairs][nb][nb], outside [npairs][nlev][4], nan [npairs]), with the
    magnitudes declared at begin in .declared.  vabs: the magnitudes of the loaded variables, default the data's own"""
    fl = H.nlev - 1 if finest_level is None else finest_level
    rr = R.ref_ratios(H)
    stoich = bool(kw.get("do_stoichiometry"))
    nvars = nload + (1 if stoich else 0)
    if vabs is None:
        mn, mx = gpu_minmax(ctx, H, states, list(range(nload)), fl)
        vabs = np.maximum(np.abs(mn), np.abs(mx))
    vabs = [float(v) for v in vabs] + ([STOICH_ABS] if stoich else [])
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels[:fl + 1]]
    P = capi.jpdf_params(nload, vmin, vmax, uncombined=uncombined, **kw)
    outs, nan = [], np.zeros(nvars * (nvars - 1) // 2, np.int64)
    with capi.JpdfAcc(ctx, nvars, nbins) as acc:
        acc.begin(_vol(H.levels[0]), vabs)
        for l in range(fl + 1):
            with capi.DevMF.from_host(ctx, dls[l], states[l]) as mf:
                o, n = acc.add_level(mf, dls[l + 1] if l < fl else None, rr[l] if l < fl else 1, _vol(H.levels[l]), P)
            outs.append(o)
            nan += n
        b, x1, x2 = acc.read()
    for dl in dls:
        dl.close()
    got = F.Sums((b, x1, x2, np.stack(outs, axis=1), nan))
    got.declared = dict(vol_max=_vol(H.levels[0]), vabs=vabs)
    return got


def check_jpdf(res, got, nbins, what, bound=True):
    """the counters and the set of non-empty bins with ==; every bin of every accumulator inside the contract's bound AND equal, bit for bit, to
    the big-integer model at the scales of the declared magnitudes (tests/fixed192_ref.py), == fsum where the terms convert exactly.  bound=False (tests/test_gpu_fixed_sums.py only): inputs with
    terms below the quantum 2^(k-157), which the accumulator truncates by design -- the model includes that, the bound presumes terms it can hold"""
    b, x1, x2, outside, nan = got
    s_vol, s_x = F.jpdf_scales(**got.declared)
    nb2 = nbins * nbins
    assert np.array_equal(outside, res["outside"]), f"{what}: out-of-range counters"
    assert np.array_equal(nan, res["nan"]), f"{what}: NaN counts"
    worst = 0.0
    for p in range(len(res["pairs"])):
        occupied = np.bincount(res["keys"][p], minlength=nb2) > 0
        assert np.array_equal(b[p].ravel() > 0, occupied), f"{what} pair {p}: the set of non-empty bins differs"
        for w, arr in enumerate((b, x1, x2)):
            if bound:
                worst = max(worst, R.assert_sum_bound(arr[p], res["keys"][p], res["terms"][p][w], nb2, f"{what} pair {p} acc {w}"))
            s = s_vol if w == 0 else s_x[res["pairs"][p][w - 1]]
            F.assert_bins_match_model(arr[p], res["keys"][p], res["terms"][p][w], s, nb2, f"{what} pair {p} acc {w}")
    return worst


def gpu_condmean(ctx, H, states, bin_comp, avg_comps, nbins, bin_min, bin_max, finest_level=None, bounds=None, with_minmax=True, uncombined=False,
                 weights_from=None, vabs=None):
    """the level loop of conditionalMean.cpp:236-298 on the device -> (hits, sum, sumsq, mn, mx), with the magnitudes declared at begin in
    .declared.  vabs: the magnitudes of the averaged components, default the data's own"""
    plan = R.condmean_plan(H, finest_level, bounds)
    wplan = plan if weights_from is None else R.condmean_plan(weights_from, finest_level, bounds)
    comps = [bin_comp] + list(avg_comps)
    fl = plan[-1]["level"]
    if vabs is None:
        mn, mx = gpu_minmax(ctx, H, states, list(avg_comps), fl)
        vabs = np.maximum(np.abs(mn), np.abs(mx))
    vabs = [float(v) for v in vabs]
    dls = {P["level"]: capi.DevLevel(ctx, H.levels[P["level"]]) for P in plan}
    with capi.CondMeanAcc(ctx, len(avg_comps), nbins, with_minmax) as acc:
        acc.begin(wplan[0]["weight"], vabs)
        for q, P in enumerate(plan):
            lev = H.levels[P["level"]]
            s = MultiFab(lev, len(comps), 0)
            for b in range(lev.nboxes):
                s.valid(b)[...] = states[P["level"]].valid(b)[comps]
            with capi.DevMF.from_host(ctx, dls[P["level"]], s) as mf:
                acc.add_level(mf, dls[P["finer"]] if P["finer"] is not None else None, P["ratio"], P["domain"], wplan[q]["weight"], bin_min, bin_max,
                              uncombined=uncombined)
        out = F.Sums(acc.read())
    for dl in dls.values():
        dl.close()
    out.declared = dict(weight_max=wplan[0]["weight"], vabs=vabs)
    return out


def check_condmean(res, got, nbins, what, bound=True):
    """binHits, minima and maxima with ==; every bin of every sum inside the contract's bound AND equal, bit for bit, to the big-integer model
    at the scales of the declared magnitudes, == fsum where the terms convert exactly.  bound=False: as for check_jpdf"""
    hits, s, s2, mn, mx = got
    s_sum, s_sq = F.condmean_scales(**got.declared)
    assert np.array_equal(hits, res["hits"]), f"{what}: binHits"
    worst = 0.0
    for a in range(s.shape[1]):
        if bound:
            worst = max(worst, R.assert_sum_bound(s[:, a], res["keys"], res["terms_sum"][a], nbins, f"{what} sum {a}"))
            worst = max(worst, R.assert_sum_bound(s2[:, a], res["keys"], res["terms_sq"][a], nbins, f"{what} sumsq {a}"))
        F.assert_bins_match_model(s[:, a], res["keys"], res["terms_sum"][a], s_sum[a], nbins, f"{what} sum {a}")
        F.assert_bins_match_model(s2[:, a], res["keys"], res["terms_sq"][a], s_sq[a], nbins, f"{what} sumsq {a}")
    if mn is not None:
        assert np.array_equal(mn, res["mn"]) and np.array_equal(mx, res["mx"]), f"{what}: per-bin minima / maxima"
    return worst


# ----------------------------------------------------------------------------- against the restatement
@pytest.mark.parametrize("name", sorted(HIERS))
def test_minmax_comps_is_exact(ctx, name):
    H = HIERS[name]
    st = make_states(H, 5, 0, field_flame, seed=2)
    for fl in range(H.nlev):
        mn, mx = gpu_minmax(ctx, H, st, [3, 0, 4], fl)
        wmn, wmx = R.jpdf_minmax(st, [3, 0, 4], fl)
        assert list(mn) == wmn and list(mx) == wmx


@pytest.mark.parametrize("name,nload,nbins,cond", [("nested", 2, 16, 0), ("nested", 4, 64, 1), ("union", 3, 128, 2), ("union", 5, 24, 0), ("ratio4", 3, 64, 1),
                                                   ("ratio4", 2, 128, 2), ("nested", 5, 128, 2), ("union", 2, 37, 1)])
def test_jpdf_matches_the_restatement(ctx, name, nload, nbins, cond):
    H = HIERS[name]
    st = make_states(H, nload, 0, field_flame, seed=1)
    vmin, vmax = R.jpdf_minmax(st, list(range(nload)), H.nlev - 1)
    kw = dict(do_conditioning=cond, cvar=nload - 1, norm_cval=1 if cond == 2 else 0, cnorm_min=vmin[nload - 1], cnorm_max=vmax[nload - 1],
              cmin=0.05 if cond == 2 else vmin[nload - 1] + 100.0, cmax=1.0 if cond == 2 else vmax[nload - 1] - 50.0)
    res = R.jpdf_accumulate(H, st, nload, nbins, vmin, vmax, **kw)
    assert all(len(k) > 0 for k in res["keys"])
    worst = check_jpdf(res, gpu_jpdf(ctx, H, st, nload, nbins, vmin, vmax, **kw), nbins, f"{name} nload={nload} nbins={nbins} cond={cond}")
    print(f"worst |S - fsum| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", sorted(HIERS))
def test_jpdf_stoichiometry_useminmax_and_a_lower_finest_level(ctx, name):
    H = HIERS[name]
    st = make_states(H, 3, 0, field_flame, seed=6)
    vmin, vmax = R.jpdf_minmax(st, [0, 1, 2], H.nlev - 1)
    vmin, vmax = vmin + [0.0], vmax + [2.0]
    vmin[1], vmax[1] = 600.0, 1500.0  # useminmax2: cells below and above the axis are clamped and counted
    kw = dict(do_stoichiometry=True, hlist=[2, 0, 1], olist=[0, 2, 1], do_conditioning=1, cvar=3, cmin=0.3, cmax=1.9)
    for fl in (H.nlev - 1, 0):
        res = R.jpdf_accumulate(H, st, 3, 32, vmin, vmax, finest_level=fl, **kw)
        assert res["outside"][:, :, 0].sum() > 0 and res["outside"][:, :, 3].sum() > 0
        check_jpdf(res, gpu_jpdf(ctx, H, st, 3, 32, vmin, vmax, finest_level=fl, **kw), 32, f"{name} stoichiometry finestLevel={fl}")


def test_jpdf_nan_and_infinite_quotients(ctx):
    """NaN skips the cell for the pair and is counted; a value far outside the axis clamps and is counted (the restatement's rule)"""
    H = nested_hierarchy(16, 2, 8)
    st = make_states(H, 2, 0, field_flame, seed=3)
    st[1].valid(2)[0, 3, 4, 5] = np.nan
    st[0].valid(0)[1, 1, 1, 1] = 1e20
    st[0].valid(0)[1, 1, 1, 2] = -1e20
    res = R.jpdf_accumulate(H, st, 2, 16, [300.0, 300.0], [2000.0, 2500.0])
    assert res["nan"][0] == 1 and res["outside"][0, 0, 2] >= 1 and res["outside"][0, 0, 3] >= 1
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    P = capi.jpdf_params(2, [300.0, 300.0], [2000.0, 2500.0])
    with capi.JpdfAcc(ctx, 2, 16) as acc:
        acc.begin(_vol(H.levels[0]), [1e20, 1e20])
        outs, nan = [], 0
        for l in range(2):
            with capi.DevMF.from_host(ctx, dls[l], st[l]) as mf:
                o, n = acc.add_level(mf, dls[l + 1] if l == 0 else None, 2, _vol(H.levels[l]), P)
            outs.append(o)
            nan += n
        got = F.Sums(acc.read() + (np.stack(outs, axis=1), nan))
        got.declared = dict(vol_max=_vol(H.levels[0]), vabs=[1e20, 1e20])
    for dl in dls:
        dl.close()
    check_jpdf(res, got, 16, "NaN / huge values")


@pytest.mark.parametrize("name,bounds,fl", [("nested", None, None), ("nested", (0.13, 0.2, 0.0, 0.8, 0.71, 0.55), None), ("union", (0.3, 0.1, 0.2, 0.9, 0.6, 0.7), None),
                                            ("union", None, 1), ("ratio4", (0.2, 0.3, 0.1, 0.6, 0.9, 0.8), None), ("ratio4", None, 0),
                                            ("nested", (0.0, 0.0, 0.0, 0.2, 0.2, 0.2), None)])
@pytest.mark.parametrize("navg,nbins", [(1, 16), (4, 128), (8, 100)])
def test_condmean_matches_the_restatement(ctx, name, bounds, fl, navg, nbins):
    H = HIERS[name]
    st = make_states(H, 9, 0, field_flame, seed=8)
    avg = list(range(1, 1 + navg))
    res = R.condmean_accumulate(H, st, 0, avg, nbins, 300.0, 2000.0, finest_level=fl, bounds=bounds)
    assert res["hits"].sum() > 0
    worst = check_condmean(res, gpu_condmean(ctx, H, st, 0, avg, nbins, 300.0, 2000.0, finest_level=fl, bounds=bounds), nbins, f"{name} {bounds} {fl} {navg} {nbins}")
    print(f"worst |S - fsum| / bound = {worst:.3f}")


def test_wide_span_component(ctx):
    """values from 1e-14 to 1 (a mass fraction) in one component: the 192-bit accumulator keeps every bit of every term down to 2^-105 of
    the declared magnitude, so the bound of the ordinary case holds -- which implies the coarser n^2 2^-53 max|t| the contract allows here"""
    H = HIERS["nested"]
    st = make_states(H, 3, 0, field_flame, seed=9)
    for l, s in enumerate(st):
        rng = np.random.default_rng(40 + l)
        for b in range(s.level.nboxes):
            v = s.valid(b)
            v[1] = 10.0 ** rng.uniform(-14, 0, size=v[1].shape)
            v[2] = -(10.0 ** rng.uniform(-14, 0, size=v[1].shape)) * np.sign(rng.uniform(-1, 3, size=v[1].shape))
    res = R.condmean_accumulate(H, st, 0, [1, 2], 64, 300.0, 2000.0)
    got = gpu_condmean(ctx, H, st, 0, [1, 2], 64, 300.0, 2000.0)
    check_condmean(res, got, 64, "wide span, conditionalMean")
    for a in range(2):
        R.assert_sum_bound(got[1][:, a], res["keys"], res["terms_sum"][a], 64, "wide span, coarse bound", coarse=True)
    vmin, vmax = R.jpdf_minmax(st, [0, 1, 2], 2)
    resj = R.jpdf_accumulate(H, st, 3, 64, vmin, vmax)
    gotj = gpu_jpdf(ctx, H, st, 3, 64, vmin, vmax)
    check_jpdf(resj, gotj, 64, "wide span, jpdf")
    # a fine axis near zero (useminmax): bins that hold ONLY tiny values, single cells among them
    vmin[1], vmax[1] = 0.0, 1e-10
    resj = R.jpdf_accumulate(H, st, 3, 64, vmin, vmax)
    check_jpdf(resj, gpu_jpdf(ctx, H, st, 3, 64, vmin, vmax), 64, "wide span, jpdf, axis 0 .. 1e-10")


def test_adversarial_distributions(ctx):
    """every cell in ONE bin (the natural state of flame data: all contention), and every cell in a DIFFERENT bin (no run to merge)"""
    H = nested_hierarchy(16, 1, 8)
    lev = H.levels[0]
    one = MultiFab(lev, 3, 0)
    rng = np.random.default_rng(5)
    for b in range(lev.nboxes):
        one.valid(b)[...] = 1000.0 + rng.uniform(0, 1, size=one.valid(b).shape)
    res = R.jpdf_accumulate(H, [one], 3, 128, [0.0] * 3, [2000.0 * 128 / 64] * 3)
    assert all(len(np.unique(k)) == 1 for k in res["keys"])
    check_jpdf(res, gpu_jpdf(ctx, H, [one], 3, 128, [0.0] * 3, [2000.0 * 128 / 64] * 3), 128, "one bin, jpdf")
    rc = R.condmean_accumulate(H, [one], 0, [1, 2], 128, 0.0, 4000.0)
    assert (rc["hits"] > 0).sum() == 1
    check_condmean(rc, gpu_condmean(ctx, H, [one], 0, [1, 2], 128, 0.0, 4000.0), 128, "one bin, conditionalMean")
    # 16^3 = 4096 cells, 64^2 = 4096 bins: cell number c -> bin (c // 64, c % 64)
    each = MultiFab(lev, 2, 0)
    for b in range(lev.nboxes):
        lo = lev.boxes[b, :3]
        k, j, i = np.meshgrid(*[np.arange(lo[d], lo[d] + 8) for d in (2, 1, 0)], indexing="ij")
        c = (k * 16 + j) * 16 + i
        each.valid(b)[0] = (c // 64) + 0.5
        each.valid(b)[1] = (c % 64) + 0.25
    res = R.jpdf_accumulate(H, [each], 2, 64, [0.0, 0.0], [64.0, 64.0])
    assert len(np.unique(res["keys"][0])) == 4096
    check_jpdf(res, gpu_jpdf(ctx, H, [each], 2, 64, [0.0, 0.0], [64.0, 64.0]), 64, "every cell its own bin")
    rc = R.condmean_accumulate(H, [each], 0, [1], 64, 0.0, 64.0)
    check_condmean(rc, gpu_condmean(ctx, H, [each], 0, [1], 64, 0.0, 64.0), 64, "every x-y plane row its own bin")


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
    vmin, vmax = R.jpdf_minmax(st, [0, 1, 2, 3], H.nlev - 1)
    kw = dict(do_conditioning=2, cvar=0, norm_cval=1, cnorm_min=vmin[0], cnorm_max=vmax[0], cmin=0.0, cmax=0.24)
    bounds = (0.1, 0.2, 0.0, 0.9, 0.8, 0.7)
    j0 = gpu_jpdf(ctx, H, st, 4, 64, vmin, vmax, **kw)
    c0 = gpu_condmean(ctx, H, st, 0, [1, 2, 3], 64, 300.0, 2000.0, bounds=bounds)
    variants = [("second run", H, st, False), ("uncombined kernel", H, st, True)]
    for how in ("retile", "shuffle"):
        H2, st2 = _retiled(H, st, how)
        assert how != "retile" or name != "nested" or H2.levels[0].nboxes < H.levels[0].nboxes
        variants.append((how, H2, st2, False))
    for what, H2, st2, unc in variants:
        j = gpu_jpdf(ctx, H2, st2, 4, 64, vmin, vmax, uncombined=unc, **kw)
        c = gpu_condmean(ctx, H2, st2, 0, [1, 2, 3], 64, 300.0, 2000.0, bounds=bounds, uncombined=unc)
        for q in range(3):
            assert bits_equal(j[q], j0[q]), f"{name}, {what}: jpdf accumulator {q} differs in its bits"
        assert np.array_equal(j[3].sum(axis=1), j0[3].sum(axis=1)) and np.array_equal(j[4], j0[4])
        assert np.array_equal(c[0], c0[0])
        for q in range(1, 5):
            assert bits_equal(c[q], c0[q]), f"{name}, {what}: conditionalMean accumulator {q} differs in its bits"


def test_accumulation_over_two_plotfiles(ctx):
    """do_average / two infiles: every file's sums are read once and added on the host in infile order (the scales of two files differ)"""
    H = HIERS["nested"]
    files = [make_states(H, 3, 0, field_flame, seed=s) for s in (20, 21)]
    for s in files[1]:
        s.data *= 1.0e3  # another magnitude: another fixed-point scale
    tot_hits, tot_sum, ref_hits = 0, 0.0, 0
    keys, terms = [], []
    for st in files:
        res = R.condmean_accumulate(H, st, 0, [1, 2], 32, 300.0, 2.0e6)
        got = gpu_condmean(ctx, H, st, 0, [1, 2], 32, 300.0, 2.0e6)
        check_condmean(res, got, 32, "one of two files")
        tot_hits, tot_sum, ref_hits = tot_hits + got[0], tot_sum + got[1], ref_hits + res["hits"]
        keys.append(res["keys"])
        terms.append(res["terms_sum"][0])
    assert np.array_equal(tot_hits, ref_hits)
    R.assert_sum_bound(tot_sum[:, 0], np.concatenate(keys), np.concatenate(terms), 32, "sum over two files")


# ----------------------------------------------------------------------------- error paths
def test_error_paths(ctx):
    H = nested_hierarchy(16, 1, 8)
    st = make_states(H, 3, 0, field_flame)
    dl = capi.DevLevel(ctx, H.levels[0])
    mf = capi.DevMF.from_host(ctx, dl, st[0])
    with pytest.raises(capi.PaError, match="2 to 8 variables"):
        capi.JpdfAcc(ctx, 1, 16)
    with pytest.raises(capi.PaError, match="1 to 8 averaged components"):
        capi.CondMeanAcc(ctx, 9, 16)
    with capi.JpdfAcc(ctx, 3, 16) as acc:
        with pytest.raises(capi.PaError, match="pa_jpdf_begin has not been called"):
            acc.add_level(mf, None, 1, 1.0, capi.jpdf_params(3, [0, 0, 0], [1, 1, 1]))
        acc.begin(_vol(H.levels[0]), [3000.0] * 3)
        with pytest.raises(capi.PaError, match="vMax == vMin for variable 1"):
            acc.add_level(mf, None, 1, _vol(H.levels[0]), capi.jpdf_params(3, [0, 5.0, 0], [1, 5.0, 1]))
        with pytest.raises(capi.PaError, match="2 variables, the accumulator was created for 3"):
            acc.add_level(mf, None, 1, _vol(H.levels[0]), capi.jpdf_params(2, [0, 0], [1, 1]))
        with pytest.raises(capi.PaError, match="cVar out of range"):
            acc.add_level(mf, None, 1, _vol(H.levels[0]), capi.jpdf_params(3, [0, 0, 0], [1, 1, 1], do_conditioning=1, cvar=3))
        # a scale taken from a magnitude the data exceed: the read fails instead of returning a wrapped sum
        acc.begin(_vol(H.levels[0]), [1.0] * 3)
        acc.add_level(mf, None, 1, _vol(H.levels[0]), capi.jpdf_params(3, [0, 0, 0], [3000, 3000, 3000]))
        with pytest.raises(capi.PaError, match="exceeds the magnitude declared"):
            acc.read()
    with capi.CondMeanAcc(ctx, 2, 16) as acc:
        acc.begin(1, [3000.0, 3000.0])
        with pytest.raises(capi.PaError, match="binMax must be greater than binMin"):
            acc.add_level(mf, None, 1, (0, 0, 0, 15, 15, 15), 1, 5.0, 5.0)
        with pytest.raises(capi.PaError, match="the bin component and 2 averaged ones"):
            with capi.DevMF(ctx, dl, 2, 0) as small:  # an input, refused for its component count before anything reads it
                acc.add_level(small, None, 1, (0, 0, 0, 15, 15, 15), 1, 0.0, 1.0)
        bad = st[0].copy()
        bad.valid(3)[1, 2, 2, 2] = np.inf
        with capi.DevMF.from_host(ctx, dl, bad) as mfb:
            acc.add_level(mfb, None, 1, (0, 0, 0, 15, 15, 15), 1, 0.0, 4000.0)
        with pytest.raises(capi.PaError, match="not finite"):
            acc.read()
    mf.close()
    dl.close()


# ----------------------------------------------------------------------------- device memory
def test_device_memory_of_the_accumulators_comes_back(ctx):
    """the pattern of tests/test_gpu_leaks.py for pa_hist: create / add / read / destroy cycles leave the free memory of the device where
    it was after the second one"""
    torch = pytest.importorskip("torch")
    H = HIERS["nested"]
    st = make_states(H, 4, 0, field_flame)
    vmin, vmax = R.jpdf_minmax(st, [0, 1, 2, 3], 2)

    def cycle():
        gpu_jpdf(ctx, H, st, 4, 128, vmin, vmax)
        gpu_condmean(ctx, H, st, 0, [1, 2, 3], 128, 300.0, 2000.0)
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


# ----------------------------------------------------------------------------- conditionalMean3d.ex end to end
import math
import os
import subprocess

from peleanalysis_amd.hierarchy import union_hierarchy
from peleanalysis_amd.plotfile import write_plotfile

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")
NAMES = ["temp", "Y(H2)", "rho/HR", "density"]


def _tool(exe, args, cwd):
    return subprocess.run([os.path.join(BIN, exe)] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def _digit(x):
    """one unit in the last of the six digits operator<< prints"""
    return 10.0 ** (math.floor(math.log10(abs(x))) - 5) if x != 0 and math.isfinite(x) else 0.0


def check_cm_file(head, rows, names, nbins, bmin, bmax, results, with_minmax):
    """the tool's CM file against the restatement of every plotfile that went into it (results, infile order).  Exact columns (bin centre,
    minima, maxima, N, p) and the header: byte for byte.  Columns that print sums: number by number, tolerance = the bound of every
    file's sums (n 2^-53 sum|t|) propagated through the host arithmetic + one unit in the last printed digit.  Returns the number of
    values compared; nothing is left out."""
    navg = len(names) - 1
    hits = sum(r["hits"] for r in results)
    mn = mx = None
    if with_minmax:
        seen = np.zeros(nbins, bool)
        mn, mx = np.zeros((nbins, navg)), np.zeros((nbins, navg))
        for r in results:
            h = r["hits"] > 0
            mn = np.where((h & ~seen)[:, None], r["mn"], np.where((h & seen)[:, None], np.minimum(mn, r["mn"]), mn))
            mx = np.where((h & ~seen)[:, None], r["mx"], np.where((h & seen)[:, None], np.maximum(mx, r["mx"]), mx))
            seen |= h
    S, dS, S2, dS2 = (np.zeros((nbins, navg)) for _ in range(4))
    for a in range(navg):
        for arr, d, key in ((S, dS, "terms_sum"), (S2, dS2, "terms_sq")):
            parts = [R.fsum_by_bin(r["keys"], r[key][a], nbins) for r in results]
            for b in range(nbins):
                arr[b, a] = math.fsum(p[0][b] for p in parts)
                d[b, a] = sum(p[2][b] * R.EPS * p[1][b] for p in parts) + (len(parts) - 1) * R.EPS * sum(abs(p[0][b]) for p in parts)
    whead, wrows, ntot = R.condmean_file(names, nbins, bmin, bmax, hits, S, S2, mn, mx)
    assert head == whead
    got, want = rows.splitlines(), wrows.splitlines()
    assert len(got) == len(want) == nbins
    compared = 0
    for b in range(nbins):
        g, w = got[b].split(" "), want[b].split(" ")
        assert len(g) == len(w), (b, got[b], want[b])
        exact = [0] + list(range(1 + 4 * navg, len(w)))
        for c in exact:
            assert g[c] == w[c] or (float(g[c]) == 0.0 == float(w[c])), f"bin {b} column {c}: {g[c]} != {w[c]}"
            compared += 1
        N = float(hits[b])
        for a in range(navg):
            cols = [(1 + a, S[b, a], dS[b, a]), (1 + navg + a, S2[b, a], dS2[b, a])]
            if hits[b] > 0:
                B, dB = S[b, a] / N, dS[b, a] / N + R.EPS * abs(S[b, a] / N)
                cols.append((1 + 2 * navg + a, B, dB))
                A, dA = S2[b, a] / N, dS2[b, a] / N + R.EPS * abs(S2[b, a] / N)
                var = A - B * B
                dvar = dA + 2 * abs(B) * dB + dB * dB + R.EPS * B * B + R.EPS * (abs(A) + B * B)
                if int((np.concatenate([r["keys"] for r in results]) == b).sum()) == 1:
                    assert var == 0.0 and float(g[1 + 3 * navg + a]) == 0.0, f"bin {b}: one cell, the variance term is an exact zero"
                    compared += 1
                else:
                    assert var - dvar > 0, f"bin {b}: the variance term is not resolved ({var} +- {dvar})"
                    cols.append((1 + 3 * navg + a, math.sqrt(var), dvar / (2 * math.sqrt(var - dvar)) + R.EPS * math.sqrt(var)))
            else:
                assert g[1 + 2 * navg + a] == "0.0" and g[1 + 3 * navg + a] == "0.0"
                compared += 2
            for c, ref, tol in cols:
                v = float(g[c])
                assert abs(v - ref) <= tol + _digit(ref), f"bin {b} column {c}: printed {g[c]}, exact {ref!r}, tolerance {tol:.3e} + {_digit(ref):.1e}"
                compared += 1
    assert compared == nbins * len(want[0].split(" ")), "a value was left out of the comparison"
    return compared


@pytest.fixture(scope="module")
def cm_plotfiles(tmp_path_factory):
    d = tmp_path_factory.mktemp("cm")
    out = {}
    for name, H in (("nested", nested_hierarchy(16, 3, 8)), ("union", union_hierarchy(11, nlev=3, n0=(16, 20, 16)))):
        for tag, seed in (("a", None), ("b", 31)):
            st = make_states(H, 4, 0, field_flame, seed=seed)
            p = str(d / f"plt_{name}_{tag}")
            write_plotfile(p, H, st, NAMES, time=0.5)
            out[(name, tag)] = (p, H, st)
    return out


@pytest.mark.parametrize("name", ["nested", "union"])
def test_conditionalmean_tool_end_to_end(cm_plotfiles, tmp_path, name):
    p, H, st = cm_plotfiles[(name, "a")]
    base = ["binComp=0", "avgComps=1 2", "binMin=300", "binMax=2000", "nBins=32"]
    res = R.condmean_accumulate(H, st, 0, [1, 2], 32, 300.0, 2000.0)
    r = _tool("conditionalMean3d.ex", ["infile=" + p] + base, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout == f"Opening file CM_temp.dat\ntotal bins: {int(res['hits'].sum())}\n"
    txt = open(tmp_path / "CM_temp.dat").read()
    head, rows = "".join(txt.splitlines(True)[:2]), "".join(txt.splitlines(True)[2:])
    check_cm_file(head, rows, NAMES[:3], 32, 300.0, 2000.0, [res], False)
    # the same bytes on a second run
    r2 = _tool("conditionalMean3d.ex", ["infile=" + p] + base, tmp_path)
    assert r2.returncode == 0 and open(tmp_path / "CM_temp.dat").read() == txt
    # minima / maxima, a bounds box through boxes and through the fine levels, finestLevel below the file's, verbose
    bounds = (0.13, 0.2, 0.0, 0.8, 0.71, 0.55)
    for fl in (None, 1):
        res = R.condmean_accumulate(H, st, 0, [2, 3, 1], 20, 300.0, 2000.0, bounds=bounds, finest_level=fl)
        args = ["infile=" + p, "binComp=0", "avgComps=2 3 1", "binMin=300", "binMax=2000", "nBins=20", "writeBinMinMax=1", "verbose=1",
                "bounds=" + " ".join(str(v) for v in bounds)] + ([f"finestLevel={fl}"] if fl is not None else [])
        r = _tool("conditionalMean3d.ex", args, tmp_path)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout == f"Processing 1 plotfiles...\n   {p}\n\nOpening {p}...\nOpening file CM_temp.dat\ntotal bins: {int(res['hits'].sum())}\n"
        txt = open(tmp_path / "CM_temp.dat").read()
        check_cm_file("".join(txt.splitlines(True)[:2]), "".join(txt.splitlines(True)[2:]), [NAMES[0], NAMES[2], NAMES[3], NAMES[1]], 20, 300.0, 2000.0, [res], True)


def test_conditionalmean_tool_two_infiles_and_aja(cm_plotfiles, tmp_path):
    """two plotfiles accumulate in infile order; aja = 1 writes the header lines to <plt0>/CM_<name>.key and the rows to <plt0>/CM_<name>.dat"""
    (pa_, H, sta), (pb, _, stb) = cm_plotfiles[("nested", "a")], cm_plotfiles[("nested", "b")]
    res = [R.condmean_accumulate(H, s, 0, [1, 2], 32, 300.0, 2000.0) for s in (sta, stb)]
    r = _tool("conditionalMean3d.ex", [f"infile={pa_} {pb}", "binComp=0", "avgComps=1 2", "binMin=300", "binMax=2000", "nBins=32", "aja=1", "writeBinMinMax=1"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    tot = int(res[0]["hits"].sum() + res[1]["hits"].sum())
    assert r.stdout == f"Output for aja\nOpening file {pa_}/CM_temp.key\nOpening file {pa_}/CM_temp.dat\ntotal bins: {tot}\n"
    check_cm_file(open(os.path.join(pa_, "CM_temp.key")).read(), open(os.path.join(pa_, "CM_temp.dat")).read(), NAMES[:3], 32, 300.0, 2000.0, res, True)


def test_conditionalmean_tool_error_paths(cm_plotfiles, tmp_path):
    p, H, st = cm_plotfiles[("nested", "a")]
    ok = ["infile=" + p, "binComp=0", "avgComps=1", "binMin=300", "binMax=2000"]
    for args, msg in ((ok[:4] + ["binMax=300"], "Bad bin min,max"), (ok + ["ngpus=2"], "ngpus > 1 is not supported"), (ok[:2] + ["binMin=300", "binMax=2000"], "need to specify avgComps"),
                      (["infile=" + p, "binComp=0", "avgComps=7", "binMin=300", "binMax=2000"], "Bad comp: 7"), (ok + ["bounds=0 0 1 1"], "bounds needs 6 values")):
        r = _tool("conditionalMean3d.ex", args, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
    from peleanalysis_amd.hierarchy import Hierarchy as Hy, Level as Lv
    lev = Lv([[0, 0, 0, 7, 7, 0]], (0, 0, 0), (7, 7, 0), (0, 0, 0), np.zeros(3), np.ones(3))
    s = MultiFab(lev, 2, 0)
    write_plotfile(str(tmp_path / "plt2d"), Hy([lev], 2), [s], ["a", "b"], dim=2)
    r = _tool("conditionalMean3d.ex", ["infile=" + str(tmp_path / "plt2d"), "binComp=0", "avgComps=1", "binMin=0", "binMax=1"], tmp_path)
    assert r.returncode != 0 and "only 3-D plotfiles are supported" in r.stderr


# ----------------------------------------------------------------------------- jpdf3d.ex end to end
import re


def _unit(tok):
    """one unit in the last printed digit of a number token (%e: six decimals; %.15g / %.17g: the last of 15 digits)"""
    m = re.fullmatch(r"-?\d\.\d{6}e([+-]\d+)", tok)
    return 10.0 ** (int(m.group(1)) - 6) if m else 1e-14 * abs(float(tok))


def compare_text(got, lo, hi, what):
    """got: the tool's file; lo / hi: the restatement's writer at both ends of the bound.  Tokens that agree in all three are exact bytes;
    the others must be numbers with min(lo, hi) - unit <= got <= max(lo, hi) + unit.  -> (tokens compared, of which numeric)"""
    shape = lambda t: re.sub(r"[^\s,]+", "#", t)
    assert shape(got) == shape(lo) == shape(hi), f"{what}: layout differs"
    tg, tl, th = (re.split(r"[\s,]+", t) for t in (got, lo, hi))
    nnum = 0
    for q, (g, a, b) in enumerate(zip(tg, tl, th)):
        if g == a == b:
            continue
        x, lo_, hi_ = float(g), min(float(a), float(b)), max(float(a), float(b))
        u = _unit(g)
        assert lo_ - u <= x <= hi_ + u, f"{what}: token {q}: {g} outside [{a}, {b}] + one unit in the last digit"
        nnum += 1
    return len(tg), nnum


def compare_fab(got, lo, hi, what):
    n = got.index(b"\n") + 1
    assert got[:n] == lo[:n] and len(got) == len(lo), f"{what}: FAB header"
    g, a, b = (np.frombuffer(t[n:]) for t in (got, lo, hi))
    lo_, hi_ = np.minimum(a, b), np.maximum(a, b)
    slack = 4 * R.EPS * np.maximum(np.abs(lo_), np.abs(hi_))  # the rounding of log() itself
    assert np.all((g >= lo_ - slack) & (g <= hi_ + slack)), f"{what}: {int((~((g >= lo_ - slack) & (g <= hi_ + slack))).sum())} values outside the bound"
    return len(g)


ALL_OUT = ("gnuplot", "matlab", "tecplot", "fab", "scatter")


def check_jpdf_outputs(tooldir, pltdir, names, nbins, vmin, vmax, results, domain_vol, time, nfiles_div=1, with_plotfile=True):
    br = R.jpdf_brackets(results, nbins, vmin, vmax, domain_vol, nfiles_div)
    pairs = results[0]["pairs"]
    ntok = nnum = 0
    for p, (a, b) in enumerate(pairs):
        ends = [R.jpdf_pair_files(names[a], names[b], nbins, vmin[a], vmax[a], vmin[b], vmax[b], *e, ALL_OUT)[0] for e in br[p]]
        for fn in ends[0]:
            path = os.path.join(tooldir, fn)
            if fn.endswith(".fab"):
                ntok += compare_fab(open(path, "rb").read(), ends[0][fn], ends[1][fn], fn)
            else:
                t, n = compare_text(open(path).read(), ends[0][fn], ends[1][fn], fn)
                if fn.endswith("_x.dat") or fn.startswith("Scatter_"):
                    assert n == 0 and open(path).read() == ends[0][fn], f"{fn}: exact bytes"
                ntok, nnum = ntok + t, nnum + n
    if with_plotfile:
        ends = [R.jpdf_plotfile(names, time, nbins, vmin, vmax, [e[k][0] for e in br]) for k in (0, 1)]
        assert open(os.path.join(pltdir, "Header")).read() == ends[0]["Header"] == ends[1]["Header"]
        t, n = compare_text(open(os.path.join(pltdir, "Level_0/Cell_H")).read(), ends[0]["Level_0/Cell_H"], ends[1]["Level_0/Cell_H"], "Cell_H")
        ntok, nnum = ntok + t, nnum + n
        ntok += compare_fab(open(os.path.join(pltdir, "Level_0/Cell_D_00000"), "rb").read(), ends[0]["Level_0/Cell_D_00000"], ends[1]["Level_0/Cell_D_00000"], "Cell_D")
    assert nnum > 0
    return ntok


@pytest.mark.parametrize("name", ["nested", "union"])
def test_jpdf_tool_end_to_end(cm_plotfiles, name):
    p, H, st = cm_plotfiles[(name, "a")]
    names = [NAMES[0], NAMES[2], NAMES[1]]
    sel = [0, 2, 1]
    sub = []
    for s in st:
        m = MultiFab(s.level, 3, 0)
        for b in range(s.level.nboxes):
            m.valid(b)[...] = s.valid(b)[sel]
        sub.append(m)
    vmin, vmax = R.jpdf_minmax(sub, [0, 1, 2], H.nlev - 1)
    res = R.jpdf_accumulate(H, sub, 3, 16, vmin, vmax)
    args = ["infile=" + p, "vars=" + " ".join(names), "nBins=16", "outSuffix=_out"] + ["output_%s=1" % o for o in ALL_OUT]
    r = _tool("jpdf3d.ex", args, os.path.dirname(p))
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    assert out.startswith("Output types:\n   + gnuplot\n   + matlab\n   + tecplot\n   + fab\n   + plotfile\n   + scatter\ndo_conditioning = 0\nProcessing 1 plotfiles...\n   " + p +
                          "\nVariable list:\n   temp\n   rho/HR\n   Y(H2)\ntemp -> temp\nrho/HR -> rho_HR\nY(H2) -> Y(H2)\n\nOpening " + p + "...\n   ...done.\nLoading data...\n   Level 0...\n")
    for pi, (a, b) in enumerate(res["pairs"]):  # the counter lines of every pair and level (:516-521)
        blk = out[out.index(f"   + {names[a]}-{names[b]}\n"):]
        blk = blk[:blk.index("   + ", 5)] if "   + " in blk[5:] else blk[:blk.index("   ...done.")]
        want = f"   + {names[a]}-{names[b]}\n"
        for l in range(H.nlev):
            want += f"      Level {l}\n"
            for lab, c in zip(("v1i<0:      ", "v1i>=nBins: ", "v2i<0:      ", "v2i>=nBins: "), res["outside"][pi, l]):
                want += f"{lab}{c}\n" if c else ""
        assert blk == want
    assert f"Opening file {p}_out/Pdf_temp_rho_HR.gpd\n" in out and "box: ((0,0,0) (15,15,0) (0,0,0))\n" in out
    n = check_jpdf_outputs(p + "_out", p + "_out", names, 16, vmin, vmax, [res], 1.0, 0.5)
    assert n > 3 * (5 * 256 + 2 * 16)
    # the same bytes on a second run
    before = {f: open(os.path.join(p + "_out", f), "rb").read() for f in os.listdir(p + "_out") if os.path.isfile(os.path.join(p + "_out", f))}
    assert _tool("jpdf3d.ex", args, os.path.dirname(p)).returncode == 0
    assert before == {f: open(os.path.join(p + "_out", f), "rb").read() for f in before}


def test_jpdf_tool_conditioning_stoichiometry_average(cm_plotfiles, tmp_path):
    """two infiles with do_average, conditioning mode 2 on the stoichiometry-free progress variable, the stoichiometry variable, useminmax axes,
    finestLevel below the file's; default outputs (the plotfile in <infile>jpdf) + matlab; the average in JPDFAverage/"""
    (pa_, H, sta), (pb, _, stb) = cm_plotfiles[("nested", "a")], cm_plotfiles[("nested", "b")]
    names = [NAMES[0], NAMES[3], "Stoichiometry"]
    vmin, vmax = [250.0, 300.0, 0.0], [2100.0, 2700.0, 2.0]
    kw = dict(do_stoichiometry=True, hlist=[2, 1], olist=[1, 3], do_conditioning=2, cvar=0, norm_cval=1, cnorm_min=300.0, cnorm_max=2000.0, cmin=0.01, cmax=0.25, finest_level=1)
    res = []
    for st in (sta, stb):
        sub = []
        for s in st:
            m = MultiFab(s.level, 2, 0)
            for b in range(s.level.nboxes):
                m.valid(b)[...] = s.valid(b)[[0, 3]]
            sub.append(m)
        res.append(R.jpdf_accumulate(H, sub, 2, 12, vmin, vmax, **kw))
    args = [f"infile={pa_} {pb}", "vars=temp density", "nBins=12", "finestLevel=1", "do_average=1", "output_matlab=1", "output_gnuplot=1", "output_tecplot=1", "output_fab=1",
            "output_scatter=1", "do_stoichiometry=1", "Hlist=2 1", "Olist=1 3", "do_conditioning=2", "cVar=0", "cNormMin=300", "cNormMax=2000", "cMin=0.01", "cMax=0.25",
            "useminmax1=250 2100", "useminmax2=300 2700"]
    r = _tool("jpdf3d.ex", args, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "   + forming average\n" in r.stdout and "Finest level: 1\n" in r.stdout and "Var1 (temp) using min/max: 250 / 2100\n" in r.stdout
    assert "Doing stoichiometry:\n   temp : #H=2 : #O=1\n   density : #H=1 : #O=3\n" in r.stdout and "cNormMin = 300\n" in r.stdout
    for pth, rs in ((pa_, res[0]), (pb, res[1])):
        check_jpdf_outputs(pth, pth + "jpdf", names, 12, vmin, vmax, [rs], 1.0, 0.5)
    check_jpdf_outputs(str(tmp_path / "JPDFAverage"), None, names, 12, vmin, vmax, res, 1.0, 0.5, nfiles_div=2, with_plotfile=False)


def test_jpdf_tool_error_paths(cm_plotfiles, tmp_path):
    p, H, st = cm_plotfiles[("nested", "a")]
    for args, msg in ((["infile=" + p, "vars=temp"], "Need to specify at least two variables."), (["infile=" + p, "vars=temp nosuch"], "Bad variable name (nosuch)"),
                      (["infile=" + p, "vars=temp density", "ngpus=2"], "ngpus > 1 is not supported"), (["infile=" + p, "vars=temp density", "useminmax2=5 5"], "vMax == vMin for variable density"),
                      (["infile=" + p, "vars=temp density", "useminmax1=1 2 3"], "Need to specify 2 values for useMinMax"),
                      (["infile=" + p, "vars=temp density", "do_stoichiometry=1", "Hlist=1"], "Need to specify one Hlist entry per variable")):
        r = _tool("jpdf3d.ex", args + ["output_plotfile=0"], tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stdout[-300:], r.stderr)


def test_jpdf_tool_nan_warning_and_2d_plotfile(tmp_path):
    """a NaN in a variable: the cell is skipped for the pairs it enters and the tool prints ONE warning line with the count; a 2-D plotfile aborts"""
    H = nested_hierarchy(16, 2, 8)
    st = make_states(H, 3, 0, field_flame, seed=3)
    st[1].valid(2)[1, 3, 4, 5] = np.nan
    p = str(tmp_path / "plt_nan")
    write_plotfile(p, H, st, ["a", "b", "c"], time=0.0)
    vmin, vmax = [300.0, 300.0, 300.0], [2100.0, 2400.0, 2700.0]
    res = R.jpdf_accumulate(H, st, 3, 8, vmin, vmax)
    assert list(res["nan"]) == [1, 0, 1]
    r = _tool("jpdf3d.ex", ["infile=" + p, "vars=a b c", "nBins=8", "useminmax1=300 2100", "useminmax2=300 2400", "useminmax3=300 2700", "output_matlab=1"], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("Warning: 2 (cell, pair) contributions skipped: the bin quotient is NaN\n") == 1
    br = R.jpdf_brackets([res], 8, vmin, vmax, 1.0)
    for pi, (a, b) in enumerate(res["pairs"]):
        n = ["a", "b", "c"]
        ends = [R.jpdf_pair_files(n[a], n[b], 8, vmin[a], vmax[a], vmin[b], vmax[b], *e, ("matlab",))[0] for e in br[pi]]
        for fn in ends[0]:
            compare_text(open(os.path.join(p, fn)).read(), ends[0][fn], ends[1][fn], fn)
    from peleanalysis_amd.hierarchy import Hierarchy as Hy, Level as Lv
    lev = Lv([[0, 0, 0, 7, 7, 0]], (0, 0, 0), (7, 7, 0), (0, 0, 0), np.zeros(3), np.ones(3))
    write_plotfile(str(tmp_path / "plt2d"), Hy([lev], 2), [MultiFab(lev, 2, 0)], ["a", "b"], dim=2)
    r = _tool("jpdf3d.ex", ["infile=" + str(tmp_path / "plt2d"), "vars=a b"], tmp_path)
    assert r.returncode != 0 and "only 3-D plotfiles are supported" in r.stderr
