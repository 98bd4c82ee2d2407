"""CPU tier: the numpy restatement of integral.cpp / rmsVel.cpp (tests/integral_ref.py) pinned by known answers, and the C ABI of the
composite integrals declared and bound."""
import math
import os

import numpy as np
import pytest

import integral_ref as I
import stats_ref as R
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import MultiFab, field_flame, fill_analytic, nested_hierarchy
from util import make_states

HIERS = R.stats_hierarchies()


def _const_states(H, vals):
    out = []
    for lev in H.levels:
        s = MultiFab(lev, len(vals), 0)
        for b in range(lev.nboxes):
            for c, v in enumerate(vals):
                s.valid(b)[c] = v
        out.append(s)
    return out


@pytest.mark.parametrize("name", sorted(HIERS))
@pytest.mark.parametrize("dir_", [0, 1, 2])
def test_unconditioned_measures_are_the_domain(name, dir_):
    """every kind-1 pixel's length is the domain length in dir, every kind-2 slot's area the cross-section, the volume the domain's"""
    H = HIERS[name]
    st = _const_states(H, [1.0])
    L = H.levels[0].prob_hi - H.levels[0].prob_lo
    for fl in range(H.nlev):
        r1 = I.integrate(H, st, [0], 1, dir_, fl)
        assert r1["out"].shape[1:] == I.out_shape(H, 1, dir_, fl)
        assert np.allclose(r1["out"][0], L[dir_], rtol=1e-13, atol=0)
        assert np.array_equal(I.measure_exact(r1, H, fl), np.full(r1["shape"], I.measure_exact(r1, H, fl).flat[0]))
        r2 = I.integrate(H, st, [0], 2, dir_, fl)
        assert np.allclose(r2["out"][0], L[(dir_ + 1) % 3] * L[(dir_ + 2) % 3], rtol=1e-13, atol=0)
        r3 = I.integrate(H, st, [0], 3, 0, fl)
        assert r3["out"].shape == (2,) and math.isclose(r3["out"][0], float(np.prod(L)), rel_tol=1e-12)
        # the terms of a slot are those of the serial sum
        ex, _, n, _ = R.fsum_by_bin(r2["keys"], r2["terms"][0], r2["nslots"])
        assert np.all(n > 0) and np.allclose(ex, r2["out"][0], rtol=1e-13)


@pytest.mark.parametrize("name", sorted(HIERS))
def test_constant_field_and_avg(name):
    H = HIERS[name]
    st = _const_states(H, [2.5, -4.0])
    for kind, dir_ in ((1, 2), (2, 1), (3, 0)):
        res = I.integrate(H, st, [0, 1], kind, dir_)
        assert np.allclose(res["out"][1], 2.5 * res["out"][0], rtol=1e-13) and np.allclose(res["out"][2], -4.0 * res["out"][0], rtol=1e-13)
        a = I.apply_avg(res["out"])
        assert np.allclose(a[1], 2.5, rtol=1e-13) and np.allclose(a[2], -4.0, rtol=1e-13) and np.array_equal(a[0], res["out"][0])


def test_avg_leaves_empty_slots_alone():
    o = np.array([[0.0, 2.0], [7.0, 3.0]])
    assert np.array_equal(I.apply_avg(o), [[0.0, 2.0], [7.0, 1.5]])


@pytest.mark.parametrize("name", sorted(HIERS))
def test_linear_field_gives_the_linear_profile(name):
    """f = x: the plane average at fine slot i of a kind-2 integral along x is the mean of x over the cells that cover the slot; where
    only the finest level covers it that is the fine cell centre, and the volume integral is 1/2"""
    H = HIERS[name]
    st = []
    for lev in H.levels:
        s = MultiFab(lev, 1, 0)
        fill_analytic(s, 0, lambda x, y, z: x + 0 * y + 0 * z)
        st.append(s)
    r3 = I.integrate(H, st, [0], 3)
    assert math.isclose(r3["out"][1], 0.5, rel_tol=1e-12)
    H1 = nested_hierarchy(16, 1, 8)
    s = MultiFab(H1.levels[0], 1, 0)
    fill_analytic(s, 0, lambda x, y, z: x + 0 * y + 0 * z)
    a = I.apply_avg(I.integrate(H1, [s], [0], 2, 0)["out"])
    assert np.allclose(a[1], I.coords(H1, 0, 0), rtol=1e-13) and np.allclose(I.coords(H1, 0, 0), (np.arange(16) + 0.5) / 16)
    # composite: the profile along x of f = x averaged over each plane is still x_i of the coarse cells' mean: integrate exactly
    r2 = I.integrate(H, st, [0], 2, 0)
    a = I.apply_avg(r2["out"])
    xf = I.coords(H, 0, H.nlev - 1)
    Rm = r2["R"][0]
    assert np.all(np.abs(a[1] - xf) <= 0.5 * Rm * (xf[1] - xf[0]) + 1e-13)  # within half a coarse cell of the fine centre
    assert math.isclose(float(np.sum(r2["out"][1]) * (xf[1] - xf[0])), 0.5, rel_tol=1e-12)


def test_condition_window_half_space_halves_the_volume():
    H = HIERS["nested"]
    st = []
    for lev in H.levels:
        s = MultiFab(lev, 2, 0)
        fill_analytic(s, 0, lambda x, y, z: 1.0 + 0 * x)
        fill_analytic(s, 1, lambda x, y, z: z + 0 * x)
        st.append(s)
    full = I.integrate(H, st, [0, 1], 3)
    half = I.integrate(H, st, [0, 1], 3, ccomp=1, cmin=0.0, cmax=0.5)
    assert math.isclose(half["out"][0], 0.5 * full["out"][0], rel_tol=1e-12)
    # cMax is exclusive, cMin inclusive; NaN fails
    st[0].valid(0)[1, 0, 0, 0] = np.nan
    n0 = len(I.integrate(H, st, [0, 1], 3, ccomp=1, cmin=-1.0, cmax=2.0)["keys"])
    assert n0 == len(full["keys"]) - 1
    one = _const_states(nested_hierarchy(8, 1, 8), [3.0])
    assert len(I.integrate(nested_hierarchy(8, 1, 8), one, [0], 3, ccomp=0, cmin=3.0, cmax=4.0)["keys"]) == 512
    assert len(I.integrate(nested_hierarchy(8, 1, 8), one, [0], 3, ccomp=0, cmin=2.0, cmax=3.0)["keys"]) == 0


@pytest.mark.parametrize("name", sorted(HIERS))
def test_finest_level_zero_ignores_finer_data(name):
    H = HIERS[name]
    st = make_states(H, 1, 0, field_flame, seed=4)
    for s in st[1:]:
        s.data[...] = 1e30
    res = I.integrate(H, st, [0], 2, 1, finest_level=0)
    lev = H.levels[0]
    assert res["shape"] == (int(lev.domhi[1] - lev.domlo[1] + 1),) and len(res["keys"]) == lev.ncells
    assert np.all(np.abs(res["out"][1]) < 1e6)


def test_flag_rules():
    assert I.ieee_sum_rule([1.0, 2.0]) is None
    assert math.isnan(I.ieee_sum_rule([1.0, float("nan"), float("inf")]))
    assert math.isnan(I.ieee_sum_rule([float("-inf"), float("inf")]))
    assert I.ieee_sum_rule([float("inf"), 3.0, float("inf")]) == float("inf")
    assert I.ieee_sum_rule([float("-inf"), 3.0]) == float("-inf")
    # ... and that is what additions in any order give
    rng = np.random.default_rng(0)
    for t in ([1.0, float("inf"), -2.0], [float("-inf"), float("inf"), 1.0], [float("nan"), 1.0], [float("-inf"), -1e308, 5.0]):
        for _ in range(5):
            s = 0.0
            with np.errstate(invalid="ignore"):
                for v in rng.permutation(t):
                    s += v
            w = I.ieee_sum_rule(t)
            assert (math.isnan(s) and math.isnan(w)) or s == w
    sp, k, t = I.split_nonfinite(np.array([0, 1, 1, 2]), np.array([1.0, float("inf"), 2.0, 3.0]), 3)
    assert sp == {1: float("inf")} and list(k) == [0, 2] and list(t) == [1.0, 3.0]


def test_ppm_bytes_of_a_hand_made_array():
    """2 x 3: colours 0, 0.25, 0.5 / 0.75, 1.0, NaN over vMin = 0, vMax = 4: the row flip puts row 1 first"""
    a = np.array([[0.0, 1.0, 2.0], [3.0, 4.0, float("nan")]])
    head = b"P6\n3 2\n255\n"
    row0 = bytes([0, 0, 127]) + bytes([0, 127, 255]) + bytes([127, 255, 127])
    past = head + bytes([255, 127, 0]) + bytes([127, 0, 0]) + bytes([255, 255, 255]) + row0
    nopast = head + bytes([255, 127, 0]) + bytes([128, 0, 0]) + bytes([128, 0, 0]) + row0
    assert I.write_ppm(a, 1, 0.0, 4.0) == past
    assert I.write_ppm(a, 0, 0.0, 4.0) == nopast
    # beyond the maximum with goPastMax: 1.1 -> (229, 0, 102), 1.2 -> (255, 0, 204), 1.3 -> (255, 51, 255)
    b = np.array([[4.4, 4.8, 5.2]])
    assert I.write_ppm(b, 1, 0.0, 4.0) == b"P6\n3 1\n255\n" + bytes([int((4.4 / 4.0 - 0.875) * 1020.), 0, int((4.4 / 4.0 - 1.0) * 1020.)]) + \
        bytes([255, 0, int((4.8 / 4.0 - 1.0) * 1020.)]) + bytes([255, int((5.2 / 4.0 - 1.25) * 1020.), 255])
    # vMax == vMin: 0 / 0 is NaN, fmin / fmax turn it into 1.5
    assert I.colour_of(2.0, 2.0, 2.0) == 1.5 and I.colour_of(-1.0, 0.0, 4.0) == 0.0 and I.colour_of(100.0, 0.0, 4.0) == 1.5
    assert I.find_min_max(a) == (0.0, 4.0)


def test_file_names_and_writers():
    assert I.outfile_name("plt0", 3, 0) == "plt0_integral"
    assert I.outfile_name("../plt0/", 2, 1, avg=1) == "../plt0/_integral_dir1_avg"
    assert I.outfile_name("plt0", 1, 2, "temp", 300.0, 1e7, 1) == "plt0_integral_dir2_ctemp_300.000000_10000000.000000_avg"
    assert I.outfile_name("plt0", 3, 2, "Y(H2)", -0.5, 1e-9, 0) == "plt0_integral_cY(H2)_-0.500000_0.000000"
    assert I.write_dat_1d([1.0, -2.5e-7]) == "1.000000e+00 -2.500000e-07 "
    assert I.write_dat_2d([[1.0, 2.0], [3.0, float("inf")]]) == "1.000000e+00 2.000000e+00 \n3.000000e+00 inf \n"
    H = nested_hierarchy(8, 2, 8)
    out = np.arange(3 * 16, dtype=np.float64).reshape(3, 16)
    f = I.integral_files("p_integral_dir0", 2, 0, ["a", "b"], out, H, 1)
    assert sorted(f) == ["p_integral_dir0_allVars.dat", "p_integral_dir0_x.dat"] and f["p_integral_dir0_allVars.dat"].count("\n") == 3
    f = I.integral_files("p_integral_dir2", 1, 2, ["a"], np.zeros((2, 16, 16)), H, 1)
    assert sorted(f) == ["p_integral_dir2_a.dat", "p_integral_dir2_length.dat", "p_integral_dir2_x.dat", "p_integral_dir2_y.dat"]
    f = I.integral_files("p_integral_dir2", 1, 2, ["a"], np.zeros((2, 16, 16)), H, 1, fmt="ppm")
    assert sorted(f) == ["p_integral_dir2_a.ppm", "p_integral_dir2_length.ppm"]
    assert I.integral_stdout("p", ["a"], 3, 2).count("Integrating level") == 2
    assert I.integral_stdout("p", ["a"], 2, 2).index("Integrating level 1") < I.integral_stdout("p", ["a"], 2, 2).index("Integrating level 0")


def test_urms_of_a_field_with_known_moments():
    """u = (m + a s, 2 m, 0) with s = +-1 on alternating cells: mean (m, 2m, 0), variances (a^2, 0, 0): urms = a / sqrt(3)"""
    H = nested_hierarchy(8, 2, 8)
    m, a = 3.0, 0.5
    st = []
    for lev in H.levels:
        s = MultiFab(lev, 3, 0)
        for b in range(lev.nboxes):
            v = s.valid(b)
            k, j, i = np.indices(v[0].shape)
            v[0] = m + a * np.where((i + j + k) % 2 == 0, 1.0, -1.0)
            v[1] = 2 * m
            v[2] = 0.0
        st.append(s)
    r = I.rmsvel(H, st)
    assert r["level"] == 1 and len(r["keys"]) == H.levels[1].ncells  # the finest level's boxes only, covered or not
    assert math.isclose(r["urms"], a / math.sqrt(3.0), rel_tol=1e-12)
    assert math.isclose(r["kappa"], (m * m + a * a + 4 * m * m + m * m + 4 * m * m) / (a * a), rel_tol=1e-9)
    r0 = I.rmsvel(H, st, finest_level=0)
    assert r0["level"] == 0 and len(r0["keys"]) == H.levels[0].ncells
    assert I.rmsvel_file([0.5, 1.0], [r["urms"], 2.0]) == "5.000000e-01 %e\n1.000000e+00 2.000000e+00\n" % r["urms"]
    assert I.rmsvel_stdout(["a", "b"], [None, 1]) == "Loading a\nLoading b\nProcessing 0/2\nFinest level: 1\nProcessing 1/2\n   ...done.\n"


def test_ppm_pixels_are_stable_across_the_bound():
    """the share of pixels whose colour differs between the two ends of the bracket the numerics contract allows is a condition on the
    test image: at most 0.1 %, asserted from the restatement alone"""
    H, st = I.ppm_case()
    for dir_ in (0, 2):
        res = I.integrate(H, st, [0, 1], 1, dir_)
        n, differ = I.ppm_bracket_pixels(res, avg=True)[:2]
        assert n > 0 and differ <= 0.001 * n, (dir_, differ, n)


def test_rmsvel_test_fields_are_well_conditioned():
    """the fields of the GPU tier's rmsVel3d test: kappa <= 1e6, so that 8 kappa 2^-53 stays far below the seven printed digits"""
    for H, st, _ in I.rmsvel_cases():
        r = I.rmsvel(H, st)
        assert r["kappa"] <= 1e6 and 8 * r["kappa"] * R.EPS < 1e-8


def test_the_header_declares_the_integral_abi_and_capi_binds_it():
    names = ["pa_integral_create", "pa_integral_begin", "pa_integral_add_level", "pa_integral_read", "pa_integral_destroy"]
    declared = capi.declared_symbols()
    for n in names:
        assert n in declared, f"{n} is not declared in include/peleanalysis_amd.h"
    src = open(os.path.join(os.path.dirname(capi.__file__), "capi.py")).read()
    for n in names:
        assert f'"{n}"' in src, f"capi.py does not bind {n}"
    assert hasattr(capi, "IntegralAcc") and hasattr(capi.IntegralAcc, "__enter__") and hasattr(capi.IntegralAcc, "add_level")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(capi.__file__)), "include", "peleanalysis_amd.h")).read()
    assert "integral.cpp:" in hdr[hdr.index("pa_integral_create") - 600:hdr.index("pa_integral_destroy")]
