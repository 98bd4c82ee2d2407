"""GPU tier: the fixed-point sums of jpdf, conditionalMean and integral / rmsVel (pa_stats.hip, pa_integral.hip over pa_fixed192.h) held to
the big-integer model of DESIGN.md 3.7 (tests/fixed192_ref.py) in EVERY bin of EVERY accumulator, on every path the launchers choose:
the bits of a sum == the bits of the model's one rounding of the exact integer sum of the truncated terms, and == math.fsum of the
terms where every term converts exactly.  The inputs (tests/fixed_sums_cases.py) cancel so far that the low limbs decide the rounded
result -- a lost carry out of limb 0 is 2^-93 of the declared magnitude -- and put ties of the rounding, carry and borrow chains over
both limb boundaries, terms below the quantum and sums of both signs into the bins; tests/test_fixed_sums_cases.py asserts on the CPU
that they do (the visibility condition).  The counters, the set of non-empty bins, minima / maxima and the measure are checked as in
test_gpu_stats.py / test_gpu_integral.py, through the same helpers.  The contract's bound n 2^-53 sum|t| is asserted as well wherever no
term of the case loses bits below its quantum 2^(k-157).  Where one does -- the `range` family, the squares of 2^-100-sized values: on
purpose -- the accumulator truncates it by design, the bound (which presumes terms the accumulator can hold) does not apply, and the
equality with the model, which includes the truncation, is the whole assertion.

A path after the first of a case is compared with the first bit for bit; where it differs it goes through the whole check, whose
message names the path, the bin, the expected limbs and both values."""
import math

import numpy as np
import pytest

import fixed192_ref as F
import fixed_sums_cases as C
import integral_ref as I
import stats_ref as R
from test_gpu_integral import check_integral, gpu_integral
from test_gpu_stats import check_condmean, check_jpdf, gpu_condmean, gpu_jpdf
from util import bits_equal

pytestmark = pytest.mark.gpu


def _same(a, b):
    return all((x is None and y is None) or (x.dtype == y.dtype and (bits_equal(x, y) if x.dtype == np.float64 else np.array_equal(x, y))) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- jpdf
def run_jpdf(ctx, case, what):
    """the combined kernel (private runs -> the 512-slot cache of hot bins -> the global table) and the uncombined one"""
    first, bound = None, C.jpdf_holds_every_term(case)
    for unc in (False, True):
        got = gpu_jpdf(ctx, case["H"], case["states"], case["nvars"], case["nbins"], case["vmin"], case["vmax"], uncombined=unc, vabs=case["vabs"])
        assert got.declared["vol_max"] == case["vol_max"]
        if first is None or not _same(got, first):
            check_jpdf(case["res"], got, case["nbins"], f"{what}, path {'uncombined' if unc else 'combined'}", bound=bound)
        first = first or got


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("hname,nvars,nbins", C.JPDF_CASES)
def test_jpdf_families(ctx, hname, nvars, nbins, family):
    """2, 3 and 4 variables (6 pairs share the cache), bins of 3 and 5 whose middle one straddles zero, `bin` = count x Vol over levels of
    different Vol"""
    case = C.jpdf_case(hname, nvars, nbins, family)
    assert all(len(np.unique(k)) >= 3 for k in case["res"]["keys"])
    assert hname == "odd" or len(set(case["res"]["vols"])) > 1
    run_jpdf(ctx, case, f"jpdf {hname} {nvars} variables {nbins} bins, {family}")


def test_jpdf_one_bin(ctx):
    """every cell of every pair in ONE bin: all contention, the longest private runs"""
    case = C.jpdf_case("nested", 4, 5, "cancel_tail", "one_bin")
    assert all(len(np.unique(k)) == 1 for k in case["res"]["keys"])
    run_jpdf(ctx, case, "jpdf one bin")


def test_jpdf_every_cell_its_own_bin(ctx):
    """one workgroup, 4096 cells in 4096 different bins: no run to combine, and at most 512 of the bins find a slot in the cache -- the
    others go to the global table one by one"""
    case = C.jpdf_case("cube", 2, 64, "cancel_tail", "all_different")
    lv = case["H"].levels[0]
    assert lv.nboxes == 1 and lv.ncells == 4096 and len(np.unique(case["res"]["keys"][0])) == 4096 > 512
    run_jpdf(ctx, case, "jpdf every cell its own bin")


def test_jpdf_largest_accepted_term(ctx):
    """a term of nextafter(2^(k+1), 0) for the declared magnitude M < 2^k is accepted and summed exactly"""
    case = dict(C.jpdf_case("odd", 2, 3, "cancel_tail"))
    k = C.k_of(case["vol_max"] * case["vabs"][0])
    case["states"] = [s.copy() for s in case["states"]]
    case["states"][0].valid(0)[0, 1, 2, 3] = math.nextafter(math.ldexp(1.0, k + 1), 0.0) / case["vol_max"]
    case["res"] = R.jpdf_accumulate(case["H"], case["states"], 2, 3, case["vmin"], case["vmax"])
    big = max(float(np.abs(t[1]).max()) for t in case["res"]["terms"])
    assert big == math.nextafter(math.ldexp(1.0, k + 1), 0.0) and case["res"]["outside"][0, 0, 1] == 1
    run_jpdf(ctx, case, "jpdf largest accepted term")


# ----------------------------------------------------------------------------- conditionalMean
def run_condmean(ctx, case, what, minmax):
    """the LDS table or (beyond 48 KB) the global one behind private runs, and the uncombined kernel; minima / maxima as given, and the other
    way round for the combined kernel"""
    first, bound = None, C.condmean_holds_every_term(case)
    avg = list(range(1, 1 + case["navg"]))
    for unc, mm in ((False, minmax), (True, minmax), (False, not minmax)):
        mode = C.condmean_mode(case["nbins"], case["navg"], mm, unc)
        got = gpu_condmean(ctx, case["H"], case["states"], 0, avg, case["nbins"], case["bmin"], case["bmax"], with_minmax=mm, uncombined=unc, vabs=case["vabs"])
        assert got.declared["weight_max"] == case["weight_max"]
        if first is None or not _same(got[:3], first[:3]):
            check_condmean(case["res"], got, case["nbins"], f"{what}, path mode {mode} minmax {mm}", bound=bound)
        elif mm:
            assert np.array_equal(got[3], case["res"]["mn"]) and np.array_equal(got[4], case["res"]["mx"]), f"{what}, path mode {mode}: per-bin minima / maxima"
        first = first or got


@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("hname,navg,nbins,minmax,mode", C.CONDMEAN_CASES)
def test_condmean_families(ctx, hname, navg, nbins, minmax, mode, family):
    """1 to 8 averaged components; tables in LDS (mode 2) and beyond 48 KB (512 bins x 8 components: mode 1); the weights of several levels"""
    case = C.condmean_case(hname, navg, nbins, family)
    assert C.condmean_mode(nbins, navg, minmax, False) == mode and C.condmean_mode(nbins, navg, minmax, True) == 0
    assert hname == "odd" or len(np.unique(case["res"]["w"])) > 1
    run_condmean(ctx, case, f"conditionalMean {hname} {navg} components {nbins} bins, {family}", minmax)


@pytest.mark.parametrize("hname,navg,nbins,mode", [("nested", 2, 16, "one_bin"), ("cube", 1, 4096, "all_different")])
def test_condmean_one_bin_and_every_cell_its_own_bin(ctx, hname, navg, nbins, mode):
    """all contention in one LDS entry; and 4096 cells in 4096 bins, a table beyond LDS: no run to combine, every add a global one"""
    case = C.condmean_case(hname, navg, nbins, "cancel_tail", mode)
    if mode == "one_bin":
        assert (case["res"]["hits"] > 0).sum() == 1 and C.condmean_mode(nbins, navg, False, False) == 2
    else:
        assert (case["res"]["hits"] == 1).all() and C.condmean_mode(nbins, navg, False, False) == 1
    run_condmean(ctx, case, f"conditionalMean {mode}", False)


def test_condmean_largest_accepted_term(ctx):
    """conditionalMean declares ONE magnitude per component for the sum and for the sum of squares (weight vabs and weight vabs^2), and a
    value whose sum term reached 2^(k+1) would have a square of at least 4 weight vabs^2 >= 2^(k2+1): refused.  So the term at the limit
    is the largest square that is accepted: (w val) val in the last binade below 2^(k2+1), within 2^-50 of it, summed exactly."""
    case = dict(C.condmean_case("odd", 1, 8, "cancel_tail"))
    w = float(case["weight_max"])
    k2 = C.k_of(w * case["vabs"][0] * case["vabs"][0])
    limit = math.ldexp(1.0, k2 + 1)
    val = math.sqrt(limit / w)
    while (w * val) * val >= limit:
        val = math.nextafter(val, 0.0)
    assert limit * (1.0 - 2.0 ** -50) <= (w * val) * val < limit
    case["states"] = [s.copy() for s in case["states"]]
    case["states"][0].valid(0)[1, 1, 2, 3] = val
    case["res"] = R.condmean_accumulate(case["H"], case["states"], 0, [1], 8, case["bmin"], case["bmax"])
    assert float(case["res"]["terms_sq"][0].max()) == (w * val) * val
    run_condmean(ctx, case, "conditionalMean largest accepted term", True)


# ----------------------------------------------------------------------------- integral / rmsVel
def run_integral(ctx, case, what, want_paths=()):
    H, first, bound = case["H"], None, C.integral_holds_every_term(case)
    for unc in (False, True):
        paths = C.integral_paths(H, case["kind"], case["dir"], case["res"]["nrows"], unc)
        got = gpu_integral(ctx, H, case["states"], case["comps"], case["kind"], case["dir"], squares=case["squares"], uncombined=unc, vabs=case["vabs"], **case["kw"])
        assert got.declared["w_max"] == case["w_max"]
        if first is None or not bits_equal(got, first):
            check_integral(case["res"], got, H, f"{what}, paths (wavefront sum, table) {sorted(paths)}", bound=bound)
        first = got if first is None else first
        for p in (want_paths if not unc else ()):
            assert p in paths, (what, p, paths)


def _ikey(c):
    return f"{c[0]}-kind{c[1]}-dir{c[2]}-{c[4]}{'-squares' if c[5] else ''}{'-cond' if c[6] else ''}"


@pytest.mark.parametrize("icase", C.integral_cases(), ids=_ikey)
def test_integral_families(ctx, icase):
    """every family through kind 3 (wavefront sum at the end, LDS), kind 2 along x (runs of 128, LDS) and across it (wavefront sum per tile,
    LDS), kind 1 along x (wavefront sum per step) and across it; the rows of squares (the rmsVel sums) and the condition window rotate"""
    hname, kind, dir_, nv, family, squares, cond = icase
    case = C.integral_case(hname, kind, dir_, nv, family, squares, cond)
    want = {3: ("end", 2), 2: ("none", 2) if dir_ == 0 else ("tile", 2), 1: ("step", 1) if dir_ == 0 else ("none", 1)}[kind]
    run_integral(ctx, case, "integral " + _ikey(icase), [want])


@pytest.mark.parametrize("kind,dir_", [(2, 1), (2, 2), (3, 0), (1, 0)])
def test_integral_rows_of_whole_wavefronts(ctx, kind, dir_):
    """a box 64 cells wide: 192-bit wavefront sums over rows in which every lane holds a run; kind 2 across x goes straight to the global table"""
    case = C.integral_case("wide", kind, dir_, 3, "cancel_tail", True, False)
    run_integral(ctx, case, f"integral wide kind {kind} dir {dir_}", [("tile", 1)] if kind == 2 else [])


@pytest.mark.parametrize("dir_", [0, 1])
def test_integral_table_beyond_lds(ctx, dir_):
    """128 slots x 17 rows: more than the launcher keeps in LDS, the finest level's runs go to the global table"""
    case = C.integral_case("tall", 2, dir_, 8, "cancel_tail", True, False)
    run_integral(ctx, case, f"integral tall dir {dir_}", [("none", 1) if dir_ == 0 else ("tile", 1)])


def test_integral_largest_accepted_term(ctx):
    case = dict(C.integral_case("odd", 3, 0, 3, "cancel_tail", False, False))
    k = C.k_of(case["w_max"] * case["vabs"][0])
    big = math.nextafter(math.ldexp(1.0, k + 1), 0.0)
    case["states"] = [s.copy() for s in case["states"]]
    case["states"][0].valid(0)[1, 1, 2, 3] = -big / case["w_max"]
    case["res"] = I.integrate(case["H"], case["states"], case["comps"], 3, 0)
    assert float(case["res"]["terms"][2].min()) == -big
    run_integral(ctx, case, "integral largest accepted term")
