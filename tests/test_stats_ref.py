"""CPU tier: known answers for the numpy restatement of jpdf.cpp / conditionalMean.cpp (tests/stats_ref.py) -- the checker of
tests/test_gpu_stats.py.  No golden file from the reference exists (neither tool compiles without AMReX)."""
import math

import numpy as np
import pytest

import stats_ref as R
from peleanalysis_amd.hierarchy import MultiFab, field_flame, fill_analytic, nested_hierarchy, union_hierarchy
from util import make_states

HIERS = R.stats_hierarchies()


def _domain_vol(H):
    l0 = H.levels[0]
    return float(np.prod(l0.prob_hi - l0.prob_lo))


@pytest.mark.parametrize("name", sorted(HIERS))
def test_jpdf_partition_of_unity(name):
    """without conditioning and with axes wide enough every volume element is counted exactly once: sum bin / domainVol = 1 to the
    bound -- a cell counted under a finer level, or a fine region left out, moves the sum by at least one cell volume"""
    H = HIERS[name]
    st = make_states(H, 3, 0, field_flame)
    vmin, vmax = R.jpdf_minmax(st, [0, 1, 2], H.nlev - 1)
    vmax = [v + 1.0 for v in vmax]  # the maximum itself would clamp
    res = R.jpdf_accumulate(H, st, 3, 16, vmin, vmax)
    assert res["outside"].sum() == 0 and res["nan"].sum() == 0
    for p in range(3):
        total = math.fsum(res["bin"][p]) / _domain_vol(H)
        n = len(res["keys"][p])
        assert abs(total - 1.0) <= n * R.EPS, (name, p, total)
    # finestLevel below the file's: the same with the coarser levels only
    res = R.jpdf_accumulate(H, st, 3, 16, vmin, vmax, finest_level=0)
    assert abs(math.fsum(res["bin"][0]) / _domain_vol(H) - 1.0) <= len(res["keys"][0]) * R.EPS


@pytest.mark.parametrize("name", sorted(HIERS))
def test_condmean_hits_count_the_finest_cells(name):
    """sum binHits = the number of finest-level cells of the (bounded) domain, exactly"""
    H = HIERS[name]
    st = make_states(H, 2, 0, field_flame)
    for bounds in (None, (0.13, 0.2, 0.0, 0.8, 0.71, 0.55)):
        res = R.condmean_accumulate(H, st, 0, [1], 32, -1e30, 1e30, bounds=bounds)
        plan = R.condmean_plan(H, None, bounds)
        d0 = np.array(plan[0]["domain"])
        ncoarse = int(np.prod(d0[3:] - d0[:3] + 1))
        assert int(res["hits"].sum()) == ncoarse * plan[0]["weight"], (name, bounds)
        if bounds is not None:
            assert ncoarse < H.levels[0].ncells


def test_condmean_plan_stops_at_an_empty_level():
    """a bounds box outside the refined region: the fine levels hold no cell of it, and level 0 has no finer level (the reference reads
    bas[iLevel+1] out of range there, conditionalMean.cpp:249)"""
    H = nested_hierarchy(16, 3, 8)
    plan = R.condmean_plan(H, None, (0.0, 0.0, 0.0, 0.2, 0.2, 0.2))
    assert [P["level"] for P in plan] == [0] and plan[0]["finer"] is None and plan[0]["weight"] == 64
    st = make_states(H, 2, 0, field_flame)
    res = R.condmean_accumulate(H, st, 0, [1], 8, -1e30, 1e30, bounds=(0.0, 0.0, 0.0, 0.2, 0.2, 0.2))
    d = np.array(plan[0]["domain"])
    assert int(res["hits"].sum()) == 64 * int(np.prod(d[3:] - d[:3] + 1))


def test_linear_field_gives_a_uniform_marginal_and_binx1_lies_in_its_bin():
    H = nested_hierarchy(16, 1, 8)
    s = MultiFab(H.levels[0], 2, 0)
    fill_analytic(s, 0, lambda x, y, z: x + 0 * y + 0 * z)
    fill_analytic(s, 1, lambda x, y, z: y + 0 * x + 0 * z)
    res = R.jpdf_accumulate(H, [s], 2, 8, [0.0, 0.0], [1.0, 1.0])
    b, x1, x2 = R.jpdf_finish(res["bin"][0], res["binX1"][0], res["binX2"][0], 0.0, 1.0, 0.0, 1.0, 8, 1.0)
    assert np.allclose(b.sum(axis=1), 1.0 / 8, rtol=1e-13, atol=0) and np.allclose(b, 1.0 / 64, rtol=1e-13, atol=0)
    edges = np.arange(9) / 8.0
    assert np.all((x1 >= edges[:-1, None]) & (x1 < edges[1:, None])) and np.all((x2 >= edges[None, :-1]) & (x2 < edges[None, 1:]))
    # an empty bin takes the bin centre (jpdf.cpp:580-583)
    res = R.jpdf_accumulate(H, [s], 2, 8, [0.0, 0.0], [2.0, 1.0])
    b, x1, x2 = R.jpdf_finish(res["bin"][0], res["binX1"][0], res["binX2"][0], 0.0, 2.0, 0.0, 1.0, 8, 1.0)
    assert np.all(b[4:] == 0) and np.array_equal(x1[4:, 0], 0.0 + 0.25 * (0.5 + np.arange(4, 8)))


def test_truncation_rule_and_the_four_counters():
    """quotients -0.5 (bin 0, not counted), -1 (bin 0, counted), nBins (last bin, counted), just below nBins (last bin, not counted),
    +-inf (clamped, counted), NaN (skipped, counted apart)"""
    nb = 8
    q = np.array([-0.5, -1.0, float(nb), np.nextafter(float(nb), 0.0), 3.25, np.inf, -np.inf, np.nan, -0.999])
    v = q / nb  # vmin 0, vmax 1: nBins * v / 1 = q exactly (nb is a power of two)
    idx, low, high, nan = R.jpdf_bin_index(v, 0.0, 1.0, nb)
    assert list(idx[:7]) == [0, 0, nb - 1, nb - 1, 3, nb - 1, 0] and idx[8] == 0
    assert list(low) == [False, True, False, False, False, False, True, False, False]
    assert list(high) == [False, False, True, False, False, True, False, False, False]
    assert list(nan) == [False] * 7 + [True, False]
    # through the accumulator: one level of 3 x 3 x 1 cells holding these values against an in-range partner
    from peleanalysis_amd.hierarchy import Hierarchy, Level
    lev = Level([[0, 0, 0, 2, 2, 0]], (0, 0, 0), (2, 2, 0), (0, 0, 0), np.zeros(3), np.ones(3))
    s = MultiFab(lev, 2, 0)
    s.valid(0)[0] = v.reshape(1, 3, 3)
    s.valid(0)[1] = 0.5
    res = R.jpdf_accumulate(Hierarchy([lev], 2), [s], 2, nb, [0.0, 0.0], [1.0, 1.0])
    assert list(res["outside"][0, 0]) == [2, 2, 0, 0] and res["nan"][0] == 1 and len(res["keys"][0]) == 8
    res = R.jpdf_accumulate(Hierarchy([lev], 2), [s], 2, nb, [0.0, 0.0], [1.0, 0.25])  # the partner now clamps high in every cell
    assert list(res["outside"][0, 0]) == [2, 2, 0, 8]


@pytest.mark.parametrize("name", sorted(HIERS))
def test_serial_sums_meet_the_fsum_bound(name):
    """the reference's own order of additions (numpy.bincount adds in input order) satisfies |S - fsum(t)| <= n 2^-53 sum|t| in every bin:
    the bound the GPU tier uses is one the reference meets"""
    H = HIERS[name]
    st = make_states(H, 3, 0, field_flame, seed=4)
    vmin, vmax = R.jpdf_minmax(st, [0, 1, 2], H.nlev - 1)
    res = R.jpdf_accumulate(H, st, 3, 16, vmin, vmax, do_conditioning=2, cvar=0, norm_cval=1, cnorm_min=vmin[0], cnorm_max=vmax[0], cmin=0.0, cmax=0.2)
    worst = 0.0
    for p in range(3):
        for w, nm in enumerate(("bin", "binX1", "binX2")):
            worst = max(worst, R.assert_sum_bound(res[nm][p], res["keys"][p], res["terms"][p][w], 256, f"{name} pair {p} {nm}"))
    cm = R.condmean_accumulate(H, st, 0, [1, 2], 32, 300.0, 2000.0)
    for a in range(2):
        worst = max(worst, R.assert_sum_bound(cm["sum"][:, a], cm["keys"], cm["terms_sum"][a], 32, f"{name} sum {a}"))
        worst = max(worst, R.assert_sum_bound(cm["sumsq"][:, a], cm["keys"], cm["terms_sq"][a], 32, f"{name} sumsq {a}"))
    assert 0.0 < worst <= 1.0


def test_numpy_bincount_adds_in_input_order():
    t = np.array([1.0, 2.0 ** -53, 2.0 ** -53, -1.0])
    assert np.bincount(np.zeros(4, np.int64), weights=t)[0] == ((1.0 + 2.0 ** -53) + 2.0 ** -53) - 1.0 == 0.0
    assert np.bincount(np.zeros(4, np.int64), weights=t[::-1])[0] == ((-1.0 + 2.0 ** -53) + 2.0 ** -53) + 1.0 != 0.0


def test_conditioning_modes_and_stoichiometry():
    H = nested_hierarchy(16, 2, 8)
    st = make_states(H, 3, 0, field_flame)
    vmin, vmax = R.jpdf_minmax(st, [0, 1, 2], 1)
    full = R.jpdf_accumulate(H, st, 3, 8, vmin, [v + 1 for v in vmax])
    c1 = R.jpdf_accumulate(H, st, 3, 8, vmin, [v + 1 for v in vmax], do_conditioning=1, cvar=0, cmin=500.0, cmax=1500.0)
    c2 = R.jpdf_accumulate(H, st, 3, 8, vmin, [v + 1 for v in vmax], do_conditioning=2, cvar=0, norm_cval=1, cnorm_min=vmin[0], cnorm_max=vmax[0], cmin=0.1, cmax=1.0)
    assert 0 < len(c1["keys"][0]) < len(full["keys"][0]) and 0 < len(c2["keys"][0]) < len(full["keys"][0])
    # stoichiometry: one more variable = 0.5 * sumH / sumO, axis 0 .. 2 (jpdf.cpp:307-310, :410-418)
    s = R.jpdf_accumulate(H, st, 3, 8, vmin + [0.0], [v + 1 for v in vmax] + [2.0], do_stoichiometry=True, hlist=[2, 0, 1], olist=[0, 2, 1])
    assert len(s["pairs"]) == 6 and s["pairs"][2] == (0, 3)
    v = [np.concatenate([st[1].valid(b)[c].ravel() for b in range(H.levels[1].nboxes)]) for c in range(3)]
    want = 0.5 * ((0.0 + v[0] * 2.0 + v[1] * 0.0 + v[2] * 1.0) / (0.0 + v[0] * 0.0 + v[1] * 2.0 + v[2] * 1.0))
    assert want.min() > 0 and want.max() < 2 and s["outside"][2].sum() == 0


def test_condmean_file_bytes_of_a_tiny_case():
    """the writer, conditionalMean.cpp:325-397, on a case small enough to write out: 2 x 2 x 1 cells, two bins"""
    from peleanalysis_amd.hierarchy import Hierarchy, Level
    lev = Level([[0, 0, 0, 1, 1, 0]], (0, 0, 0), (1, 1, 0), (0, 0, 0), np.zeros(3), np.ones(3))
    s = MultiFab(lev, 2, 0)
    s.valid(0)[0] = np.array([0.1, 0.2, 0.7, 5.0]).reshape(1, 2, 2)
    s.valid(0)[1] = np.array([1.0, 3.0, -2.5, 9.0]).reshape(1, 2, 2)
    r = R.condmean_accumulate(Hierarchy([lev], 2), [s], 0, [1], 2, 0.0, 1.0)
    assert list(r["hits"]) == [2, 1]
    head, rows, ntot = R.condmean_file(["T", "Y"], 2, 0.0, 1.0, r["hits"], r["sum"], r["sumsq"], r["mn"], r["mx"])
    assert ntot == 3
    assert head == "VARIABLES = T Y_sum Y_sumSq Y_avg Y_std Y_min Y_max N  p \nZONE I=2 DATAPACKING=POINT\n"
    assert rows == "0.25 4 10 2 1 1 3 2 0.666667\n0.75 -2.5 6.25 -2.5 0 -2.5 -2.5 1 0.333333\n"
    # an empty bin prints "0.0" for _avg and _std (:380-385); no min / max columns without writeBinMinMax
    head, rows, _ = R.condmean_file(["T", "Y"], 4, 0.0, 20.0, np.array([3, 0, 0, 0]), np.array([[1.5], [0], [0], [0]]), np.array([[9.0], [0], [0], [0]]))
    assert head.startswith("VARIABLES = T Y_sum Y_sumSq Y_avg Y_std N  p \n")
    assert rows.splitlines()[1] == "7.5 0 0 0.0 0.0 0 0"


@pytest.mark.parametrize("name", ["nested", "union"])
def test_flame_fields_keep_the_std_column_well_conditioned(name):
    """the inputs of the end-to-end comparison of the _std column (tests/test_gpu_stats.py): with field_flame m = 0 as the bin variable and
    m = 1, 2 averaged, binMin 300, binMax 2000, 32 bins, the variance term S2/N - (S/N)^2 is never negative and at least 1e-9 of the
    squared mean in every bin with more than one cell -- the tolerance propagated through the square root relies on it"""
    H = nested_hierarchy(16, 3, 8) if name == "nested" else union_hierarchy(11, nlev=3, n0=(16, 20, 16))
    st = make_states(H, 3, 0, field_flame)
    r = R.condmean_accumulate(H, st, 0, [1, 2], 32, 300.0, 2000.0)
    checked = 0
    for a in range(2):
        ex, _, n, _ = R.fsum_by_bin(r["keys"], r["terms_sum"][a], 32)
        ex2, _, _, _ = R.fsum_by_bin(r["keys"], r["terms_sq"][a], 32)
        for b in range(32):
            cells = int((r["keys"] == b).sum())
            if cells > 1:
                N = float(r["hits"][b])
                var, mean2 = ex2[b] / N - (ex[b] / N) ** 2, (ex[b] / N) ** 2
                assert var >= 1e-9 * mean2, (name, a, b, var, mean2)
                checked += 1
    assert checked >= 20


def test_jpdf_writer_bytes_of_a_tiny_case():
    """every jpdf output (jpdf.cpp:595-870) for 2 bins, two variables, three cells -- small enough to write out"""
    from peleanalysis_amd.hierarchy import Hierarchy, Level
    lev = Level([[0, 0, 0, 1, 1, 0]], (0, 0, 0), (1, 1, 0), (0, 0, 0), np.zeros(3), np.array([1.0, 1.0, 0.5]))
    s = MultiFab(lev, 2, 0)
    s.valid(0)[0] = np.array([0.25, 0.25, 0.75, 0.75]).reshape(1, 2, 2)
    s.valid(0)[1] = np.array([1.0, 3.0, 3.0, 3.5]).reshape(1, 2, 2)
    res = R.jpdf_accumulate(Hierarchy([lev], 2), [s], 2, 2, [0.0, 0.0], [1.0, 4.0])
    assert list(res["bin"][0]) == [0.125, 0.125, 0.0, 0.25]
    p, x1, x2 = R.jpdf_finish(res["bin"][0], res["binX1"][0], res["binX2"][0], 0.0, 1.0, 0.0, 4.0, 2, 0.5)
    files, order = R.jpdf_pair_files("a/b", "T", 2, 0.0, 1.0, 0.0, 4.0, p, x1, x2, ("gnuplot", "matlab", "tecplot", "fab", "scatter"))
    assert order == ["Pdf_a_b_T.gpd", "Pdf_a_b_T.dat", "Pdf_a_b_x.dat", "Pdf_T_x.dat", "PdfX1_a_b_T.dat", "PdfX2_a_b_T.dat", "Pdf_a_b_T.tpd", "Pdf_a_b_T.fab", "Scatter_a_b_T.dat"]
    assert files["Pdf_a_b_T.gpd"] == ("2.500000e-01 1.000000e+00 2.500000e-01\n2.500000e-01 3.000000e+00 2.500000e-01\n"
                                      "7.500000e-01 1.000000e+00 0.000000e+00\n7.500000e-01 3.000000e+00 5.000000e-01\n")
    assert files["Pdf_a_b_T.dat"] == "2.500000e-01 2.500000e-01 \n0.000000e+00 5.000000e-01 \n"
    assert files["Pdf_a_b_x.dat"] == "2.500000e-01\n7.500000e-01\n" and files["Pdf_T_x.dat"] == "1.000000e+00\n3.000000e+00\n"
    assert files["PdfX1_a_b_T.dat"] == "2.500000e-01 2.500000e-01 \n7.500000e-01 7.500000e-01 \n"  # the empty bin takes its centre
    assert files["PdfX2_a_b_T.dat"] == "1.000000e+00 3.000000e+00 \n1.000000e+00 3.250000e+00 \n"
    assert files["Pdf_a_b_T.tpd"] == ("VARIABLES = a/b T logpdf pdf\nZONE N=4 E=1 F=FEPOINT ET=QUADRILATERAL\n"
                                      "2.500000e-01 1.000000e+00 -1.386294e+00 2.500000e-01\n2.500000e-01 3.000000e+00 -1.386294e+00 2.500000e-01\n"
                                      "7.500000e-01 1.000000e+00 -1.611810e+01 0.000000e+00\n7.500000e-01 3.000000e+00 -6.931470e-01 5.000000e-01\n1 3 4 2\n")
    assert files["Scatter_a_b_T.dat"] == "2.500000e-01 1.000000e+00\n2.500000e-01 3.000000e+00\n7.500000e-01 3.000000e+00\n"
    fab = files["Pdf_a_b_T.fab"]
    head = b"FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))((0,0,0) (1,1,0) (0,0,0)) 4\n"
    assert fab.startswith(head) and len(fab) == len(head) + 4 * 4 * 8
    d = np.frombuffer(fab[len(head):]).reshape(4, 2, 2)
    assert d[0].tolist() == [[0.25, 0.75], [0.25, 0.75]] and d[1].tolist() == [[1.0, 1.0], [3.0, 3.0]] and d[3].tolist() == [[0.25, 0.0], [0.25, 0.5]]
    plt = R.jpdf_plotfile(["a/b", "T"], 0.5, 2, [0.0, 0.0], [1.0, 4.0], [p])
    assert plt["Header"] == ("NavierStokes-V1.1\n2\nPdf_a/b_T\nPdf_a/b_T (log)\n2\n0.5\n0\n0 0\n1 1\n\n((0,0) (1,1) (0,0))\n0\n0.5 0.5\n0\n0\n0 1 0.5\n0\n0 1\n0 1\nLevel_0/Cell\n0 1\n0 4\n")
    assert plt["Level_0/Cell_H"].startswith("1\n1\n2\n0\n(1 0\n((0,0,0) (1,1,0) (0,0,0))\n)\n1\nFabOnDisk: Cell_D_00000 0\n\n1,2\n0,-16.11809565095832,\n\n1,2\n0.5,")
    cd = np.frombuffer(plt["Level_0/Cell_D_00000"][len(head) - 2 + len(b"2\n"):]).reshape(2, 2, 2)
    assert cd[0].tolist() == [[0.25, 0.0], [0.25, 0.5]]
