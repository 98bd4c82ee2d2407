"""The CPU restatement of the gradient-streamline tool (tests/streamgrad_ref.py: stream.cpp + stream_nd.f90) pinned against
the reference's own arithmetic and against known answers.

golden/stream_vtrace_ref.npz holds inputs and outputs of the reference's `vtrace` (Src/stream_nd.f90 as it is, compiled by
flang -O0 -ffp-contract=off for plain x86-64 -- no FMA -- with a stub amrex_fort_module giving amrex_real = 8 and
amrex_spacedim = 3, and a stub bl_pd_myproc; called through bind(C) with the arguments stream.cpp:920-925 passes).  Six
cases on FABs of 4^3 valid cells with nGrow 4 (dx = 1/32, domain [0,1]^3): a tanh flame with two aux components; seeds at
the eight corners of the box with long steps (lines cut short at both ends); nRKsteps even; traceAlongV (computeVec = 0);
a constant gradient with g.g between (double)1.e-12f and 1e-12 (the default-real literal of vnrml decides whether the
vector is normalised); a FAB at the domain's corner with a rough velocity field, where a last RK4 step ends beyond phi and
the state is copied from the step before."""
import os

import numpy as np
import pytest

import streamgrad_ref as R
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, chop_box, fill_analytic, nested_hierarchy

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_vtrace_ref.npz")
CASES = ["tanh_aux2", "corners_cut", "even_steps", "trace_along_v", "eps_literal", "wall_copy"]


def golden_case(name):
    z = np.load(GOLD)
    return {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(name + "__")}


def run_case(c):
    F = R.Fab(c["T"], c["T_lo"])
    vc = int(c["vcomp"])
    return R.vtrace(F, F.a.shape[0], c["loc"], c["ids"], None if vc < 0 else F, None if vc < 0 else (vc, vc + 1, vc + 2), int(c["nRKsteps"]),
                    c["dx"], c["plo"], c["phi"], float(c["hRK"]))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_reference_vtrace(name):
    c = golden_case(name)
    strm, err = run_case(c)
    assert err == int(c["errFlag"])
    assert np.array_equal(strm.view(np.int64), c["strm"].view(np.int64))


def test_fixture_covers_the_quirks():
    """what each case is there for actually happens in the recorded data"""
    c = golden_case("corners_cut")
    pos = c["strm"][:3]
    assert np.all(pos[:, 0] == pos[:, 1], axis=0).any() and np.all(pos[:, -1] == pos[:, -2], axis=0).any()  # cut short both ways
    c = golden_case("wall_copy")
    s = c["strm"]
    moved = np.any(s[:3, 1:] != s[:3, :-1], axis=0)
    assert (moved & np.all(s[3:, 1:] == s[3:, :-1], axis=0)).any()  # a moved point with the state of the point before
    assert int(golden_case("even_steps")["nRKsteps"]) % 2 == 0
    old = R.EPS_VNRML
    try:  # a double 1e-12 does not normalise the eps case's vector: different lines
        R.EPS_VNRML = 1e-12
        strm, _ = run_case(golden_case("eps_literal"))
    finally:
        R.EPS_VNRML = old
    assert not np.array_equal(strm, golden_case("eps_literal")["strm"])


def _one_level(n, box, per=(0, 0, 0)):
    return Hierarchy([Level(chop_box((0, 0, 0), (n - 1,) * 3, box), (0, 0, 0), (n - 1,) * 3, per, np.zeros(3), np.ones(3))], 2)


def _raw(H, ng, fns):
    out = []
    for lv in H.levels:
        m = MultiFab(lv, len(fns), ng)
        for c, f in enumerate(fns):
            fill_analytic(m, c, f)
        out.append(m)
    return out


def test_linear_field_gives_straight_lines_spaced_hrk():
    H = nested_hierarchy(16, 2, 8, is_per=(0, 0, 0))
    raw = _raw(H, 4, [lambda x, y, z: 3.0 * x + 0 * y + 0 * z])
    nodes = np.array([[0.5, 0.3, 0.41], [0.5, 0.52, 0.49], [0.4375, 0.5, 0.5], [0.2, 0.8, 0.1]]).T
    r = R.run_tool(H.levels, raw, nodes, ["X", "Y", "Z"], np.array([1, 2, 3]), 1, nRKsteps=11, hRK=0.1)
    h = r["hRK"]
    assert h == 0.1 / 32
    n = 0
    for per in r["lines"]:
        for st in per:
            if st is None:
                continue
            for i in range(st.shape[2]):
                x = st[0, :, i]
                assert np.array_equal(st[1, :, i], np.full(11, st[1, 5, i])) and np.array_equal(st[2, :, i], np.full(11, st[2, 5, i]))
                assert np.abs(np.diff(x) - h).max() < 1e-15
                n += 1
    assert n == 4 and all(f == 0 for fl in r["flags"] for f in fl)


def test_radial_field_gives_lines_along_radii():
    H = _one_level(16, 16)
    c = np.array([0.5, 0.5, 0.5])
    raw = _raw(H, 4, [lambda x, y, z: (x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2])
    rng = np.random.default_rng(3)
    d = rng.normal(size=(3, 20))
    d /= np.linalg.norm(d, axis=0)
    nodes = c[:, None] + 0.25 * d
    r = R.run_tool(H.levels, raw, nodes, ["X", "Y", "Z"], np.array([1]), 1, nRKsteps=21, hRK=0.2)
    st = r["lines"][0][0]
    for i in range(st.shape[2]):
        v = st[:3, :, i] - c[:, None]
        u = v / np.linalg.norm(v, axis=0)
        assert np.abs(np.cross(u.T, d[:, i]).max()) < 1e-12  # on the ray of the seed
        rad = np.linalg.norm(v, axis=0)
        assert np.all(np.diff(rad) > 0)  # outwards, up the gradient


def test_membership_edges():
    H = nested_hierarchy(16, 2, 8, is_per=(0, 0, 0))
    lv0 = H.levels[0]
    dx = 1.0 / 16
    # (a) exactly on the hi face x = 8 dx of box 0 (cells 0..7): half-open, it belongs to the box that starts there
    # (b) inside the region level 1 covers (coarse cells 4..11): excluded on level 0, present on level 1
    # (c) a node placed outside every box of a one-box-per-level hierarchy with a hole is dropped
    nodes = np.array([[8 * dx, 0.1, 0.1], [0.5, 0.5, 0.5], [0.05, 0.95, 0.05]]).T
    ins = R.inside_nodes(H.levels, nodes)
    where = {}
    for l, per in enumerate(ins):
        for b, ids in enumerate(per):
            for i in ids:
                where.setdefault(int(i), []).append((l, b))
    assert len(where[1]) == 1 and where[1][0][0] == 0 and lv0.boxes[where[1][0][1], 0] == 8
    assert where[2] == [(1, where[2][0][1])]
    assert len(where[3]) == 1 and where[3][0][0] == 0
    holey = Level(np.array([[0, 0, 0, 7, 15, 15]]), (0, 0, 0), (15, 15, 15), (0, 0, 0), np.zeros(3), np.ones(3))
    ins = R.inside_nodes([holey], nodes)
    assert [list(x) for x in ins[0]] == [[3]]  # nodes 1 (x = 0.5 exactly, the hi face) and 2 lie in no box: dropped


def test_trim_surface_renumbers():
    nodes = np.array([[0.1, 0.5, 0.9, 0.5, 0.2], [0.1, 0.5, 0.5, 0.9, 0.3], [0.5] * 5])
    face = np.array([1, 2, 5, 2, 3, 4, 1, 5, 2], dtype=np.int32)
    nn, nf = R.trim_surface([0.0, 0.0, 0.0], [0.8, 1.0, 1.0], nodes, face, 3)  # drops node 3 (x = 0.9)
    assert nn.shape == (3, 4) and np.array_equal(nn[0], [0.1, 0.5, 0.5, 0.2])
    assert list(nf) == [1, 2, 4, 1, 4, 2]  # element 2 used node 3: gone; node 4 -> 3, node 5 -> 4


def test_writers_bytes_two_levels():
    """a hand-made two-level case: one box of level 0 holds two seeds, one box does not; level 1 holds one seed; nRKsteps 3"""
    st0 = np.arange(2 * 3 * 4, dtype=np.float64).reshape(4, 3, 2) * 0.5
    st1 = -np.arange(1 * 3 * 4, dtype=np.float64).reshape(4, 3, 1) / 3.0
    names = ["X", "Y", "Z", "temp"]
    ins = [[np.array([1, 3], np.int32), np.array([], np.int32)], [np.array([2], np.int32)]]
    files = R.stream_file_bytes(names, np.array([1, 2, 3], np.int32), 1, ins, [[st0, None], [st1]], 3)
    assert files["Header"] == b"Oddball-multilevel-connected-data-format\n2\n4\nX\nY\nZ\ntemp\n"
    assert files["Elements"] == b"1\n3\n1 2 3 \n1\n0 2 1 3\n1\n0 1 2\n"
    h = files["Level_0/Str_H"].decode()
    assert h.startswith("1\n1\n4\n0\n(2 0\n((0,-1,0) (1,1,0) (0,0,0))\n((0,0,0) (0,0,0) (0,0,0))\n)\n2\nFabOnDisk: Str_D_00000 0\n")
    d = files["Level_0/Str_D_00000"]
    hdr = b"FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))((0,-1,0) (1,1,0) (0,0,0)) 4\n"
    assert d.startswith(hdr) and d[len(hdr):len(hdr) + 24 * 8] == st0.tobytes()
    assert ("FabOnDisk: Str_D_00000 %d\n" % (len(hdr) + 24 * 8)) in h
    assert h.endswith("\n2,4\n%s\n0,0,0,0,\n" % "".join("%.17g," % st0[c].max() for c in range(4)))
    dat = R.out_file_bytes(names, [[st0, None], [st1]], 3).decode()
    lines = dat.split("\n")
    assert lines[0] == "VARIABLES = X Y Z temp "
    assert lines[1] == "ZONE I=1 J=3 k=1 FORMAT=POINT" and lines[2] == "0 3 6 9 " and lines[3] == "1 4 7 10 "
    assert dat.count("ZONE") == 3 and lines[10] == "-0 -1 -2 -3 " and lines[11] == "-0.333333 -1.33333 -2.33333 -3.33333 "
    # the null-box rule: one seed, nRKsteps 1 -> the Str box equals the null box and dump writes nothing
    one = np.zeros((4, 1, 1))
    assert R.out_file_bytes(names, [[one]], 1) is None


def test_is_per_has_no_effect_cpu():
    """FixOOB zeroes every periodic ghost cell after the last FillBoundary: the states (and so the lines) are the same"""
    res = []
    for per in ((0, 0, 0), (1, 1, 1)):
        H = nested_hierarchy(16, 2, 8, is_per=per)
        raw = _raw(H, 3, [lambda x, y, z: np.tanh((x - 0.2 + 0.3 * y - 0.1 * z) / 0.1), lambda x, y, z: np.sin(4 * x) + y * z])
        nodes = np.array([[0.02, 0.5, 0.5], [0.5, 0.97, 0.03], [0.4, 0.45, 0.6]]).T
        res.append(R.run_tool(H.levels, raw, nodes, ["X", "Y", "Z"], np.array([1, 2, 3]), 1, nRKsteps=15, hRK=0.5))
    for a, b in zip(res[0]["states"], res[1]["states"]):
        assert np.array_equal(a.data.view(np.int64), b.data.view(np.int64))
    for pa_, pb in zip(res[0]["lines"], res[1]["lines"]):
        for x, y in zip(pa_, pb):
            assert (x is None and y is None) or np.array_equal(x.view(np.int64), y.view(np.int64))
