"""CPU tier of the partStream tracer: the numpy restatement of StreamPC.cpp (tests/stream_ref.py, whole arrays of lines, FABs
cut from a dense array) against the plain-C oracle (oracle/pa_oracle_stream.c, one line at a time, the text the kernel
shares) -- positions and prepared field bit for bit, the number of redistributions, the failing line of a "bad RK" -- on the
case matrix the GPU tier runs kernel against oracle (tests/stream_cases.py).  Two texts by different routes from the same
source agree; a slip in one of them (a weight, a ghost layer, a constant) does not survive this."""
import numpy as np
import pytest

import stream_cases as SC
import stream_ref as R
from peleanalysis_amd.hierarchy import MultiFab


def _both(oracle, c, seeds=None):
    seeds = c["seeds"] if seeds is None else seeds
    want, wred = oracle.stream_trace(c["H"].levels, c["v"], seeds, c["nsteps"], c["dt"], vcomp=c["vcomp"])
    info = {}
    got, gred = R.trace(c["H"].levels, c["v"], seeds, c["nsteps"], c["dt"], vcomp=c["vcomp"], info=info)
    return want, wred, got, gred, info


@pytest.mark.parametrize("name", list(SC.CASES))
def test_restatement_matches_oracle(oracle, name):
    c = SC.build(SC.CASES[name], oracle)
    SC.assert_fields_equal(R.prepare_field(c["H"].levels, c["raw"], c["comps"], c["ngrow"]), c["v3"], name)
    want, wred, got, gred, info = _both(oracle, c)
    assert (2 * len(c["seeds"])) % 64 != 0 and (2 * len(c["seeds"])) % 256 != 0
    # the conditions of the matrix, on the oracle's result: re-assignments happen, lines are cut and clamped at the walls
    clamped, cut = SC.wall_events(want, c["H"], c["dt"])
    assert wred >= 1 and clamped >= 1 and cut >= 1, (wred, clamped, cut)
    for s in c["off"]:  # no grid: the line stays at its seed
        assert np.all(SC.bits(want[2 * s:2 * s + 2]) == SC.bits(c["seeds"][s])[None, None, :])
    assert gred == wred
    assert np.array_equal(SC.bits(got), SC.bits(want))
    assert info["nclamp"] == clamped and info["ncut"] >= cut  # the restatement's own count: scale < 1 / moved by the clamp


@pytest.mark.parametrize("name", list(SC.EDGE_CASES))
def test_edge_cases_match_oracle(oracle, name):
    """Nsteps = 1 (no step: the seeds), Nsteps = 2 (one step, no re-assignment possible), no seeds at all"""
    c = SC.build(SC.EDGE_CASES[name], oracle)
    SC.assert_fields_equal(R.prepare_field(c["H"].levels, c["raw"], c["comps"], c["ngrow"]), c["v3"], name)
    want, wred, got, gred, _ = _both(oracle, c)
    assert want.shape == got.shape == (2 * len(c["seeds"]), c["nsteps"], 3)
    assert gred == wred == 0
    assert np.array_equal(SC.bits(got), SC.bits(want))
    if len(c["seeds"]):
        assert np.array_equal(SC.bits(want[:, 0]), SC.bits(np.repeat(c["seeds"], 2, axis=0)))
    if name == "nsteps2":
        assert sum(SC.wall_events(want, c["H"], c["dt"])) >= 1 and np.any(want[:, 1] != want[:, 0])


@pytest.mark.parametrize("name", list(SC.BAD_RK_CASES))
def test_bad_rk_cases_fail_in_both(oracle, name):
    """both stop in the same step and name the same line: the lowest failing line of the first failing step"""
    c = SC.build(SC.BAD_RK_CASES[name], oracle)
    with pytest.raises(RuntimeError, match="bad RK") as eo:
        oracle.stream_trace(c["H"].levels, c["v"], c["seeds"], c["nsteps"], c["dt"])
    with pytest.raises(R.BadRK) as er:
        R.trace(c["H"].levels, c["v"], c["seeds"], c["nsteps"], c["dt"])
    assert str(eo.value) == str(er.value)


@pytest.mark.parametrize("which", ["a", "b"])
def test_zero_vector_is_bad_rk(oracle, which):
    """an exactly zero vector: vnrml gives NaN, the next position is not finite, ntrpv refuses it by an explicit test (the
    reference gets there through the int conversion of NaN on x86): "bad RK", naming the one line that ran into the zero region;
    without that seed the run completes"""
    H, raw, seeds, line = SC.zero_region_case(which)
    v = oracle.stream_field(H.levels, raw, (0, 1, 2), MultiFab, ngrow=SC.ZERO_NG)
    SC.assert_fields_equal(R.prepare_field(H.levels, raw, (0, 1, 2), SC.ZERO_NG), v)
    grown = H.levels[0].boxes[R.where(H.levels, seeds[(line - 1) // 2][None, :])[1][0]]
    assert bool(np.all(grown[:3] - SC.ZERO_NG <= 0)) == (which == "a")  # the failing line's FAB holds cell index 0, or not
    with pytest.raises(RuntimeError) as eo:
        oracle.stream_trace(H.levels, v, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert str(eo.value) == f"bad RK (line {line})"
    with pytest.raises(R.BadRK) as er:
        R.trace(H.levels, v, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert er.value.line == line
    rest = np.delete(seeds, (line - 1) // 2, axis=0)
    want, _ = oracle.stream_trace(H.levels, v, rest, SC.ZERO_NSTEPS, SC.ZERO_DT)
    got, _ = R.trace(H.levels, v, rest, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert np.array_equal(SC.bits(got), SC.bits(want)) and np.isfinite(want).all()


def test_zero_vector_in_the_last_stage_moves_the_line_to_the_corner(oracle):
    """the reference's other answer to a zero vector (see stream_cases.zero_region_case, "jump"): no error, the line lands on
    plo + 1e-10; the same bits in both"""
    H, raw, seeds, line = SC.zero_region_case("jump")
    v = oracle.stream_field(H.levels, raw, (0, 1, 2), MultiFab, ngrow=SC.ZERO_NG)
    want, wred = oracle.stream_trace(H.levels, v, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    got, gred = R.trace(H.levels, v, seeds, SC.ZERO_NSTEPS, SC.ZERO_DT)
    assert np.array_equal(SC.bits(got), SC.bits(want)) and gred == wred and np.isfinite(want).all()
    assert np.any(np.all(want[line - 1] == 1.0e-10, axis=1))
    others = np.delete(want, line - 1, axis=0)
    assert not np.any(np.all(others == 1.0e-10, axis=2))


def test_huge_vector_and_seeds_without_a_position(oracle):
    """|v|^2 >= 1e12: vnrml returns the zero vector and the line stays at its seed (StreamPC.cpp:150-156); a seed that is not
    finite lies on no grid (defined here) and stays what it is; bit for bit in both"""
    H = SC.hierarchy("nested")
    raw = []
    for lv in H.levels:
        m = MultiFab(lv, 3, 0)
        for c, val in enumerate((7.0e5, -7.0e5, 4.0e5)):  # 1.14e12
            for b in range(lv.nboxes):
                m.valid(b)[c] = val
        raw.append(m)
    v = oracle.stream_field(H.levels, raw, (0, 1, 2), MultiFab, ngrow=2)
    rng = np.random.default_rng(5)
    seeds = np.concatenate([0.1 + 0.8 * rng.random((50, 3)), [[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, -np.inf]]])
    want, wred = oracle.stream_trace(H.levels, v, seeds, 8, 0.01)
    got, gred = R.trace(H.levels, v, seeds, 8, 0.01)
    assert np.array_equal(SC.bits(got), SC.bits(want)) and gred == wred
    assert np.all(SC.bits(want) == SC.bits(np.repeat(seeds, 2, axis=0))[:, None, :])


def test_where_is_the_finest_level_holding_the_cell():
    """the restatement's Where() against a brute-force search, cell by cell, on the union-of-rectangles hierarchy"""
    H = SC.hierarchy("union")
    rng = np.random.default_rng(3)
    x = rng.random((400, 3))
    lev, grd = R.where(H.levels, x)
    for p in range(len(x)):
        want = (-1, -1)
        for l in range(H.nlev - 1, -1, -1):
            lv = H.levels[l]
            cell = np.floor(x[p] / lv.dx).astype(int)
            hit = [b for b in range(lv.nboxes) if np.all(cell >= lv.boxes[b, :3]) and np.all(cell <= lv.boxes[b, 3:])]
            if hit:
                want = (l, hit[0])
                break
        assert (lev[p], grd[p]) == want
    assert len(set(lev.tolist())) == H.nlev
