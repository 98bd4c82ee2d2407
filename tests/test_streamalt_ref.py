"""The CPU restatement of stream.cpp's alternate-surface mode (tests/streamalt_ref.py) pinned by answers that do not come from it,
and the case matrix (tests/streamalt_cases.py) held to its conditions: every branch of the search on some line of every query,
both signs of lIdx, no NaN among the outputs, and every planted mistake visible in some case."""
import math

import numpy as np
import pytest

import streamalt_cases as K
import streamalt_ref as A
from peleanalysis_amd.plotfile import read_mef
from util import bits_equal


def _straight(nRKsteps, step, v0, g, extra=()):
    """one line x(j) = x0 + j * step, component 3 = v0 + g * (arc length from j = 0), further components = extra(j)"""
    lo, hi = A.jrange(nRKsteps)
    j = np.arange(lo, hi + 1, dtype=np.float64)
    L = math.sqrt(sum(s * s for s in step))
    st = np.zeros((4 + len(extra), nRKsteps, 1))
    for d in range(3):
        st[d, :, 0] = 0.5 + step[d] * j
    st[3, :, 0] = v0 + g * L * j
    for c, f in enumerate(extra):
        st[4 + c, :, 0] = f(j)
    return st, L


@pytest.mark.parametrize("nRKsteps", [5, 8, 51])
@pytest.mark.parametrize("where", [-1.5, -0.25, 0.0, 0.5, 1.25])
def test_straight_line_linear_field_is_exact(nRKsteps, where):
    """power-of-two spacing (a 3-4-5 step: segment length 5 / 64) and a linear field: position, distance, carried value and
    thickness are exact"""
    step = (3 / 64, 4 / 64, 0.0)
    g = 8.0
    st, L = _straight(nRKsteps, step, 2.0, g, extra=(lambda j: 16.0 - 4.0 * j,))
    assert L == 5 / 64
    val = 2.0 + g * L * where
    thickLo, thickHi = val - 0.25 * g * L, val + 0.5 * g * L
    out, br, lidx = A.alt_surface([[st]], [[np.array([1])]], nRKsteps, 1, 3, val, carry=(3, 4), thickComp=3, thickLo=thickLo, thickHi=thickHi)
    assert br[:, 0].tolist() == [1, 1, 1]
    assert lidx[0, 0] == math.floor(where)
    assert out[:, 0].tolist() == [0.5 + step[0] * where, 0.5 + step[1] * where, 0.5, val, 16.0 - 4.0 * where, L * where, (thickHi - thickLo) / g]


def test_line_rising_in_z_gives_pi():
    st, _ = _straight(5, (0.0, 0.0, 0.125), 0.0, 1.0)
    out, _, _ = A.alt_surface([[st]], [[np.array([1])]], 5, 1, 3, 0.0625, carry=(3,), addAngle=True)
    assert out[-1, 0] == -1.0
    fin, names = A.post_step(out, A.surface_names(["X", "Y", "Z", "temp"], (3,), addAngle=True), 1, True, False)
    assert fin[-1, 0] == math.acos(-1) == math.pi and names[-1] == "angleWRTvert"
    st2, _ = _straight(4, (0.25, 0.0, 0.0), 0.0, 1.0)  # even nRKsteps: lo = -1, hi = 2, h = (int)(0.5 * 1) = 0: the points j = -1 and j = 1
    st2[2, 2, 0] += 1.0  # z(1) one higher; h = 1 would take j = 0 and j = 2, both at the old height
    out2, _, _ = A.alt_surface([[st2]], [[np.array([1])]], 4, 1, 3, 0.0625, carry=(3,), addAngle=True)
    assert out2[-1, 0] == -1.0 / math.sqrt(0.25 + 1.0)


def test_scan_exhausted_loses_its_last_segment():
    """val == v(hi): lIdx = rIdx = hi, frac = 0 -- the position is x(hi), the distance stops one segment short"""
    st, L = _straight(5, (0.0, 0.25, 0.0), 0.5, 1.0)
    val = float(st[3, 4, 0])
    out, br, lidx = A.alt_surface([[st]], [[np.array([1])]], 5, 1, 3, val, carry=(3,))
    assert br[0, 0] == 2 and lidx[0, 0] == 2
    assert out[:, 0].tolist() == [0.5, 0.5 + 2 * 0.25, 0.5, val, 1 * L]
    # above all values: the last segment with frac = 1 -- the same position, the whole distance
    out, br, _ = A.alt_surface([[st]], [[np.array([1])]], 5, 1, 3, val + 1.0, carry=(3,))
    assert br[0, 0] == 3 and out[:, 0].tolist() == [0.5, 1.0, 0.5, val, 2 * L]
    # at or below v(lo): the first point, the whole distance back
    out, br, _ = A.alt_surface([[st]], [[np.array([1])]], 5, 1, 3, float(st[3, 0, 0]), carry=(3,))
    assert br[0, 0] == 0 and out[:, 0].tolist() == [0.5, 0.0, 0.5, float(st[3, 0, 0]), -2 * L]


def test_first_up_crossing_wins_and_nan_is_walked_over():
    st, L = _straight(7, (0.5, 0.0, 0.0), 0.0, 1.0)
    st[3, :, 0] = [0.0, 2.0, 0.0, 2.0, 0.0, 2.0, 3.0]
    out, br, lidx = A.alt_surface([[st]], [[np.array([1])]], 7, 1, 3, 1.0, carry=(3,))
    assert br[0, 0] == 1 and lidx[0, 0] == -3 and out[:, 0].tolist() == [0.5 - 2.5 * 0.5, 0.5, 0.5, 1.0, -2.5 * L]
    st[3, :, 0] = [0.0, np.nan, 0.5, 0.75, 2.0, 3.0, 4.0]
    out, br, lidx = A.alt_surface([[st]], [[np.array([1])]], 7, 1, 3, 1.0, carry=(3,))
    assert br[0, 0] == 1 and lidx[0, 0] == 0 and out[:, 0].tolist() == [0.5 + 0.2 * 0.5, 0.5, 0.5, 0.75 + 1.25 * 0.2, 0.2 * L]


def test_cold_strain_is_read_where_T_crosses():
    st, _ = _straight(5, (0.0, 0.0, -0.5), 10.0, 2.0, extra=(lambda j: 300.0 + 100.0 * j, lambda j: 7.0 - 2.0 * j))
    out, br, _ = A.alt_surface([[st]], [[np.array([1])]], 5, 1, 3, 10.0, carry=(3,), TComp=4, TVal=350.0, strainComp=5)
    assert br[:, 0].tolist() == [1, 1] and out[-1, 0] == 7.0 - 2.0 * 0.5


@pytest.mark.parametrize("nRKsteps", K.NRK)
def test_case_matrix_conditions(nRKsteps):
    """the inputs of both tiers: every query takes each of the four branches on some line and locates on both sides of the seed;
    every node is written; no output is a NaN (see streamalt_cases.py for why)"""
    out, branch, lidx = K.reference(nRKsteps, "all")
    assert branch.shape[0] == 4
    for q in range(4):
        assert set(branch[q].tolist()) == {0, 1, 2, 3}, q
        assert (lidx[q] < 0).any() and (lidx[q] >= 0).any(), q
    assert not np.isnan(out).any() and not np.isnan(K.reference(nRKsteps, "same_comp")[0]).any()
    lines, ins, nNodes = K.build(nRKsteps)
    assert sorted(np.concatenate([i for per in ins for i in per]).tolist()) == list(range(1, nNodes + 1))
    assert [[0 if x is None else x.shape[2] for x in per] for per in lines] == [list(b) for b in K.BOXES]
    nan_lines = sum(int(np.isnan(x[K.ISO]).any(axis=0).sum()) for per in lines for x in per if x is not None)
    assert (nan_lines > 0) == (nRKsteps >= 5)
    assert any((np.diff(x[0:3], axis=1) == 0).all(axis=0).any() for per in lines for x in per if x is not None)  # dd = 0
    assert any(np.signbit(x[K.TCOMP][x[K.TCOMP] == 0]).any() for per in lines for x in per if x is not None)  # -0.0 meets T_VAL


@pytest.mark.parametrize("subset", [s for s in K.SUBSETS if s not in ("all", "same_comp")])
def test_subsets_are_columns_of_all(subset):
    full, fb, _ = K.reference(5, "all")
    cols = {"alt": [0, 1, 2, 6, 7], "thick": [0, 1, 2, 6, 7, 8], "strain": [0, 1, 2, 3, 4, 5, 6, 7, 9], "angle": [0, 1, 2, 6, 7, 10]}[subset]
    rows = {"alt": [0], "thick": [0, 1, 2], "strain": [0, 3], "angle": [0]}[subset]
    out, br, _ = K.reference(5, subset)
    assert bits_equal(out, full[cols]) and np.array_equal(br, fb[rows])


@pytest.mark.parametrize("mistake", A.MISTAKES)
def test_planted_mistake_changes_some_case(mistake):
    changed = [n for n in K.NRK if not bits_equal(K.reference(n, "all")[0], K.reference(n, "all", mistake)[0])]
    assert changed, mistake
    if mistake == "h_round_up":
        assert changed == [4]  # only an even nRKsteps has lo + hi odd


def test_post_step_and_mef_bytes(tmp_path):
    out = np.arange(12, dtype=np.float64).reshape(6, 2) / 8  # X Y Z temp distance cos
    out[5] = [0.5, -1.0]
    names = A.surface_names(["X", "Y", "Z", "temp"], (3,), addAngle=True)
    assert names == ["X", "Y", "Z", "temp", "distance_iso_to_alt", "angleWRTvert"]
    fin, fn = A.post_step(out, names, 1, True, False, iso_dist=np.array([10.0, 20.0]))
    assert fn[4] == "delta" and fin[4].tolist() == [10.0 + 8 / 8, 20.0 + 9 / 8] and fin[5].tolist() == [math.acos(0.5), math.pi]
    fin2, fn2 = A.post_step(out, names, 1, True, False)
    assert fn2[4] == "delta" and fin2[4].tolist() == out[4].tolist()
    adv = np.array([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0], [0.5, 0.25], [-1.0, 2.0], [4.0, -8.0], [9.0, 9.0], [0.0, 0.0]])
    an = A.surface_names(["X", "Y", "Z", "temp", "x_velocity", "y_velocity", "z_velocity"], (4, 5, 6, 3), advect=True)
    fin3, fn3 = A.post_step(adv, an, 4, False, True, dt=0.5)
    assert fn3 == ["X", "Y", "Z", "x_velocity", "y_velocity", "z_velocity", "temp", "distance_iso_to_alt"]
    assert fin3[0:3].tolist() == [[1.25, 2.125], [2.5, 5.0], [7.0, 2.0]]
    face = np.array([1, 2, 2, 2, 1, 1], np.int32)
    p = tmp_path / "s.mef"
    p.write_bytes(A.mef_bytes("advected alt surface", fn3, fin3, face, 2))
    label, rn, nodes, faces = read_mef(str(p))
    assert label == "advected alt surface" and list(rn) == fn3
    assert bits_equal(nodes, fin3.T) and faces.ravel().tolist() == face.tolist()
