"""The restatement tests/streamsel_ref.py (streamScatter.cpp, stream2plt.cpp) held to answers worked out by hand -- none of them comes
from the restatement -- and the recalled random draw pinned against libstdc++'s <random>.  CPU tier; the GPU parity is in
test_gpu_streamsel.py."""
import math
import os
import subprocess

import numpy as np
import pytest

import streamsample_ref as S
import streamsel_cases as K
import streamsel_ref as R


def small():
    names, files = K.small_dir()
    return names, files, S.read_stream_dir(files)


def small_fab(extra=0):
    names, files, path = small()
    sel, nbox, _ = R.downsample(path, 3, 3)
    assert sel == [(0, 0, 0), (0, 0, 1), (0, 0, 2)] and nbox == [1]  # rval = 1: every line, in storage order whatever the node ids
    return R.final_array(path, sel, [0, 1, 2, 3, 4], -2, 2, extra=extra)


def test_truncation_toward_zero():
    # int ptOnStr = 0.5 * (lo + hi): -0.5 -> 0 and -1.5 -> -1 (floor would give -1 and -2)
    assert [R.trunc_mid(*r) for r in ((-3, 3), (-4, 3), (-5, 2), (0, 5), (-2, 2))] == [0, 0, -1, 2, 0]


def test_scatter_peaks_by_hand():
    """The scan starts at j = 0 (index 2).  Node 1 is line 1: c = 7 7 9 7 7, nothing exceeds the 9 at the start -> j = 0.  Node 2 is line 2:
    c = 9 1 1 1 9 starts from 1, the 9 at j = -2 replaces it, the 9 at j = 2 is not strictly greater -> j = -2.  Node 3 is line 0:
    c = 0 10 20 30 40 starts from 20, 30 and 40 replace it -> j = 2 (the last point)."""
    names, files, path = small()
    assert R.build_node_map(path) == [(0, 0, 1), (0, 0, 2), (0, 0, 0)]
    assert R.peaks(path, 4) == ([0, -2, 2], [9.0, 9.0, 40.0])
    # hiVal >= 9 && hiVal < 40: nodes 1 and 2 (9 == the lower bound is kept, 40 == the upper bound is dropped), in node order;
    # T and X at (line 1, j = 0) = 3, 3 and at (line 2, j = -2) = 1, 0
    assert R.run_scatter(files, vars=["T", "X"], condComp=4, condValMoreThan=9, condValLessThan=40) == "3 3 \n1 0 \n"
    assert R.run_scatter(files, vars=["T", "X"], condVar="c", condValMoreThan=9, condValLessThan=40.5) == "3 3 \n1 0 \n5 4 \n"
    assert R.run_scatter(files, vars=["X"], condComp=4, condValMoreThan=50, condValLessThan=60) == ""
    for kw, msg in ((dict(vars=["W"], condComp=4), "Variable not found: W"), (dict(vars=["X"], condVar="W"), "Conditioning variable not found: W"),
                    (dict(vars=["X"]), "no conditioning component"), (dict(condComp=4), "vars not found"), (dict(vars=["X"], condComp=4, ngpus=2), "ngpus")):
        with pytest.raises(R.SelAbort, match=msg):
            R.run_scatter(files, **kw)


def test_node_map_refuses_bad_ids():
    names, files = K.small_dir()
    path = S.read_stream_dir(files)
    for ids, msg in (([1, 2, 4], "outside 1 .. 3"), ([1, 2, 2], "node 3 has no inside_nodes entry"), ([0, 1, 2], "outside 1 .. 3")):
        path["ins"] = [[np.array(ids)]]
        with pytest.raises(R.SelAbort, match=msg):
            R.build_node_map(path)


def test_max_filter_and_line0_seed():
    fab = small_fab()
    # Max(c) < 35: the maxima are 40, 9, 9 (the seed, line 0's first c = 0, changes nothing here)
    assert R.filter_lines(fab, -2, 2, maxc=[(4, "lt", 35.0)]) == [0, 1, 1]
    # Min(c) > 0.5: the lines' own minima are 0, 7, 1 -- lines 1 and 2 would pass -- but every running minimum starts from line 0's
    # first point, c = 0 (:591): all three fail.  The quirk flips two decisions.
    own = [min(fab[4, :, i]) for i in range(3)]
    assert own == [0.0, 7.0, 1.0] and [int(m > 0.5) for m in own] == [0, 1, 1]
    assert R.filter_lines(fab, -2, 2, minc=[(4, "gt", 0.5)]) == [0, 0, 0]
    # an unknown sign string tests false
    assert R.filter_lines(fab, -2, 2, maxc=[(4, "smaller", 1e9)]) == [0, 0, 0]
    for sgn, want in (("ge", [1, 0, 0]), ("gt", [0, 0, 0]), ("le", [1, 1, 1]), ("eq", [1, 0, 0]), ("ne", [0, 1, 1])):
        assert R.filter_lines(fab, -2, 2, maxc=[(4, sgn, 40.0)]) == want, sgn


def test_at_test_switches_a_rejected_line_back_on():
    fab = small_fab()
    # T crosses 2.5 on line 0 in segment 1 (2 -> 3) and on line 1 in segment 2 (3 -> 2), alpha = 0.5 both; line 2 (T = 1) never.
    assert R.first_crossing(fab, 0, 5, 3, 2.5) == (1, 0.5) and R.first_crossing(fab, 1, 5, 3, 2.5) == (2, 0.5) and R.first_crossing(fab, 2, 5, 3, 2.5) is None
    # X there: line 0: 1 + 0.5 * (2 - 1) = 1.5; line 1: 3 + 0.5 * (3 - 3) = 3.  Max(c) < 35 has rejected line 0; the at-test X > 1 ASSIGNS
    # 1 to it (:646).  Line 2 has no crossing and keeps the 1 it had.
    assert R.filter_lines(fab, -2, 2, maxc=[(4, "lt", 35.0)], atc=[(3, 0.0, "gt", 1.0, 2.5)]) == [1, 1, 1]
    assert R.filter_lines(fab, -2, 2, maxc=[(4, "lt", 35.0)], atc=[(3, 0.7, "gt", 2.0, 2.5)]) == [0, 1, 1]  # compAt 0.7 -> 0; 1.5 > 2 fails
    # a line rejected and never crossed stays rejected: Max(c) < 5 rejects all, only lines 0 and 1 cross
    assert R.filter_lines(fab, -2, 2, maxc=[(4, "lt", 5.0)], atc=[(3, 0.0, "gt", 1.0, 2.5)]) == [1, 1, 0]
    # a value exactly on a point brackets nothing: T = 3 sits on index 2 of lines 0 and 1, so a test nothing could pass changes nothing
    assert R.first_crossing(fab, 0, 5, 3, 3.0) is None and R.first_crossing(fab, 1, 5, 3, 3.0) is None
    assert R.filter_lines(fab, -2, 2, atc=[(3, 0.0, "lt", -100.0, 3.0)]) == [1, 1, 1]


def test_radius_at_the_middle_point():
    fab = small_fab()
    # the point is index 2 (j = 0): (X, Y) = (2, 0), (3, 4), (0, 0) -> 2, 5, 0
    assert R.filter_lines(fab, -2, 2, RXY=2.5, RXYsgn="gt") == [0, 1, 0]
    assert R.filter_lines(fab, -2, 2, RXY=2.0, RXYsgn="le") == [1, 0, 1]
    assert R.filter_lines(fab, -2, 2, RXY=-1.0, RXYsgn="nonsense") == [1, 1, 1]  # RXY <= 0: no test at all


def test_arc_length_by_hand():
    fab = small_fab(extra=1)
    assert [R.segment_lengths(fab, i) for i in range(3)] == [[1.0, 1.0, 1.0, 1.0], [5.0, 0.0, 0.0, 4.0], [2.0, 2.0, 2.0, 2.0]]
    R.arc_length(fab, 5, 3, 2.5)
    # line 0: running sum 0 1 2 3 4, offset 1 + 0.5 * (2 - 1) = 1.5
    assert list(fab[5, :, 0]) == [-1.5, -0.5, 0.5, 1.5, 2.5]
    # line 1: running sum 0 5 5 5 9, crossing in segment 2 where both ends are 5: offset 5
    assert list(fab[5, :, 1]) == [-5.0, 0.0, 0.0, 0.0, 4.0]
    # line 2: no crossing -> 2 x the last running sum (8) at every point
    assert list(fab[5, :, 2]) == [16.0] * 5


def test_tool_output_by_hand():
    names, files, path = small()
    r = R.run_stream2plt(files, nLines=3, maxComps=[4], maxVals=[35.0], maxSgns=["lt"], distComp=3, distVal=2.5)
    assert r["stdout"] == "Reduced dataset has 3 lines \n" and r["write_lines"] == [0, 1, 1]
    assert r["dat"].decode() == ("VARIABLES = X Y Z T c distance_from_T_eq_2.5 \n"
                                 "ZONE T=id1 I=5 F=POINT\n" "0 0 0 5 7 -5 \n" "3 4 0 4 7 0 \n" "3 4 0 3 9 0 \n" "3 4 0 2 7 0 \n" "3 8 0 1 7 4 \n"
                                 "ZONE T=id2 I=5 F=POINT\n" "0 0 0 1 9 16 \n" "0 0 2 1 1 16 \n" "0 0 4 1 1 16 \n" "0 0 6 1 1 16 \n" "0 0 8 1 9 16 \n")
    r = R.run_stream2plt(files, nLines=5, comps=[3, 0], no_filter=1, maxComps=[0], maxVals=[-1.0], maxSgns=["lt"])  # no_filter: the test is not run
    assert r["write_lines"] == [1, 1, 1] and r["dat"].decode().split("\n")[:3] == ["VARIABLES = T X ", "ZONE T=id0 I=5 F=POINT", "1 0 "]
    for kw, msg in ((dict(nLines=0), "nLines"), (dict(nLines=3, finestLevel=1), "finestLevel"), (dict(nLines=3, distComp=3, distVal=1.0, no_filter=1), "no_filter"),
                    (dict(nLines=3, maxComps=[1, 2], maxVals=[1.0], maxSgns=["lt", "lt"]), "maxVals has 1 values"), (dict(nLines=3, comps=[0, 5]), "out of range"),
                    (dict(nLines=3, maxComps=[5], maxVals=[1.0], maxSgns=["lt"]), "out of range"), (dict(nLines=3, ngpus=2), "ngpus")):
        with pytest.raises(R.SelAbort, match=msg):
            R.run_stream2plt(files, **kw)


def test_fixture_sums_tell_serial_from_pairwise():
    """the coordinates of the GPU fixture make the running sqrt sum inexact: a pairwise (tree) sum of a line's segments differs from the
    serial one in the last bits for a good part of the lines, so a scanned or reordered sum on the device would show"""
    names, files, levels, ins = K.plt_dir()
    path = S.read_stream_dir(files)
    slo, shi, NLines = R.stream_extent(path)
    assert (slo, shi, NLines) == (-4, 3, 193)
    sel, _, _ = R.downsample(path, K.ALL, NLines)
    fab = R.final_array(path, sel, [0, 1, 2], slo, shi)
    differ = 0
    for i in range(fab.shape[2]):
        s = R.segment_lengths(fab, i)
        assert len(s) == 7
        serial = 0.0
        for v in s:
            serial = serial + v
        pairwise = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + s[6])
        differ += serial != pairwise
    assert differ >= 20


def test_fixtures_hold_the_edge_cases():
    names, files, levels, ins = K.scatter_dir()
    path = S.read_stream_dir(files)
    jp, hv = R.peaks(path, 4)
    where = R.build_node_map(path)
    node_of = {w: n for n, w in enumerate(where)}
    assert len(where) == 193 and [w for w in where] != sorted(where)  # node order is not storage order
    mids = {(0, 0): 0, (0, 2): 0, (1, 0): -1, (1, 1): 2}
    for (l, b), mid in mids.items():
        lo, hi, a = path["levels"][l][b]
        assert jp[node_of[(l, b, 0)]] == mid and hv[node_of[(l, b, 0)]] == 5.0  # the constant line stays at the truncated middle
        if hi[0] < 10:
            continue
        n = [node_of[(l, b, k)] for k in range(11)]
        assert jp[n[1]] == mid and jp[n[2]] == lo[1] + 1 and jp[n[3]] == lo[1] and jp[n[4]] == hi[1]
        assert hv[n[5]] == math.inf and hv[n[6]] == 0.0 and math.copysign(1.0, hv[n[6]]) == -1.0 and jp[n[6]] == mid
        assert math.isnan(hv[n[7]]) and jp[n[7]] == mid and hv[n[8]] == 6.0 and hv[n[9]] == K.MORE and hv[n[10]] == K.LESS
    out = [R.run_scatter(files, **kw) for kw in K.SCATTER_RUNS]
    assert "-0 " in out[2] and out[3] == "" and "nan" not in out[0]
    kept = [n for n in range(193) if hv[n] >= K.MORE and hv[n] < K.LESS]
    assert out[0].count("\n") == len(kept) and 20 < len(kept) < 193
    assert out[0].split("\n")[0].split()[0] == R.fmt(hv[kept[0]])  # the first row is the lowest kept node id


def test_recalled_random_draw_is_libstdcxx(tmp_path):
    """std::uniform_real_distribution<double>(0, 1) over std::mt19937(987654321) against the restatement over numpy's raw outputs.  This pins
    the generator as recalled; it does not pin AMReX's use of it."""
    src = tmp_path / "draws.cpp"
    src.write_text("#include <cstdio>\n#include <random>\nint main() {\n  std::mt19937 gen(987654321);\n  std::uniform_real_distribution<double> draw(0.0, 1.0);\n"
                   "  for (int i = 0; i < 1000; ++i) std::printf(\"%.17g\\n\", draw(gen));\n  return 0;\n}\n")
    exe = tmp_path / "draws"
    subprocess.run([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", str(src), "-o", str(exe)], check=True, timeout=300)
    got = [float(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.split()]
    want = R.random_draws(1000)
    assert len(got) == 1000 and got == want
    assert all(0.0 <= v < 1.0 for v in want) and 400 < sum(v < 0.5 for v in want) < 600


def test_partial_selection_follows_the_draw():
    names, files, levels, ins = K.plt_dir()
    path = S.read_stream_dir(files)
    d = R.random_draws(193)
    sel, nbox, text = R.downsample(path, 60, 193, verbose=True)
    order = [(l, b, i) for l, per in enumerate(path["ins"]) for b, ids in enumerate(per) for i in range(len(ids))]
    assert sel == [o for o, v in zip(order, d) if v < 60.0 / 193.0] and 30 < len(sel) < 90
    assert text.startswith("0 (%d):  ( 0 from %d ) " % (sum(1 for s in sel if s[:2] == (0, 0)), sel[0][2])) and text.count("src data has") == sum(nbox)
