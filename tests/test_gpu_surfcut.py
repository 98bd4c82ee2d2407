"""GPU tier: the surface cutting and trimming kernels (peleanalysis_amd/csrc/pa_surfcut.hip) through the C ABI, and sliceMEF3d.ex /
trimMEFgen3d.ex end to end, against the restatement tests/surfcut_ref.py.  For every case of tests/surfcut_cases.py: the contour
vertices as uint64 bits, the directed pairs, segments, source elements and the incidence CSR exactly; the trimmed nodes as bits and the
elements exactly; the area total, minimum and maximum as bits.  Output arrays start as the payload NaN of tests/util.py ("writes each
output"), and pa_surf_last_launch must report the case's counts."""
import functools
import os
import subprocess

import numpy as np
import pytest

import surfcut_cases as SC
import surfcut_ref as R
from peleanalysis_amd import capi
from util import SENT_GPU, sentinel_count

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
KEYS = ("verts", "pairs", "segs", "src", "csr_off", "csr_adj")


@functools.lru_cache(maxsize=None)
def ref_slice(name, k):
    nodes, e = SC.slice_surface(name)
    comp, loc = SC.SLICES[name][1][k]
    return R.slice_surface(nodes, e, comp, loc)


@functools.lru_cache(maxsize=None)
def ref_trim(name):
    nodes, e = SC.trim_surface(name)
    return R.trim_surface(nodes, e, **SC.trim_args(name))


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def bits(x):
    return np.float64(x).view(np.uint64)


def assert_slice(got, want, what):
    for g, key in zip(got, KEYS):
        w = want[key]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, w.shape)
        if g.dtype == np.float64:
            assert sentinel_count(g, SENT_GPU) == 0, (what, key, "never written")
            bad = np.argwhere(u64(g) != u64(w))
            assert len(bad) == 0, (what, key, len(bad), bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        else:
            assert np.array_equal(g, w), (what, key, int(np.sum(g != w)), g.ravel()[:8].tolist(), w.ravel()[:8].tolist())


def assert_surface(got, want_nodes, want_elts, what):
    assert got[0].shape == want_nodes.shape and got[1].shape == want_elts.shape, (what, got[0].shape, want_nodes.shape, got[1].shape, want_elts.shape)
    assert sentinel_count(got[0], SENT_GPU) == 0, what
    assert np.array_equal(u64(got[0]), u64(want_nodes)), what
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want_elts), what


def assert_area(got, nodes, e, what):
    want = R.area(nodes, e)
    assert [bits(g) for g in got] == [bits(w) for w in want], (what, got, want)


@pytest.mark.parametrize("name", list(SC.SLICES))
def test_slices_equal_restatement(ctx, name):
    nodes, e = SC.slice_surface(name)
    cuts = SC.SLICES[name][1]
    with capi.Surf(ctx, nodes, e) as s, capi.Surf(ctx, nodes, e) as s2:
        assert s.counts() == (len(nodes), len(e), nodes.shape[1])
        first = None
        for k, (comp, loc) in enumerate(cuts):
            want = ref_slice(name, k)
            assert s.slice(comp, loc) == (len(want["verts"]), len(want["segs"])), (name, k)
            got = s.slice_read(fill=SENT_GPU)
            assert_slice(got, want, "%s cut %d" % (name, k))
            rec = s.last_launch()
            ns, nv = len(want["segs"]), len(want["verts"])
            assert rec["op"] == "slice" and (rec["elements"], rec["segments"], rec["requests"], rec["vertices"], rec["values"], rec["csr_entries"]) == \
                (len(e), ns, 2 * ns, nv, nv * nodes.shape[1], 2 * ns), (name, k, rec)
            assert rec["kernels"] == (9 if ns else 1), rec  # a cut that misses stops after the classification
            s2.slice(comp, loc)  # a second handle: the same input gives the same bytes
            for a, b in zip(got, s2.slice_read(fill=SENT_GPU)):
                assert a.tobytes() == b.tobytes(), (name, k)
            first = first or got
        # after the other locations, the first again: the surface was not changed and nothing was uploaded
        s.slice(*cuts[0])
        for a, b in zip(first, s.slice_read(fill=SENT_GPU)):
            assert a.tobytes() == b.tobytes(), name
        assert_surface(s.read(fill=SENT_GPU), nodes, e, name + " surface after slicing")
        assert_area(s.area(), nodes, e, name)
        rec = s.last_launch()
        assert rec["op"] == "area" and rec["elements"] == rec["terms"] == len(e) and rec["kernels"] == 2


@pytest.mark.parametrize("name", list(SC.TRIMS))
def test_trims_equal_restatement(ctx, name):
    nodes, e = SC.trim_surface(name)
    n2, e2, unused = ref_trim(name)
    a = SC.trim_args(name)
    res = []
    for _ in range(2):
        with capi.Surf(ctx, nodes, e) as s:
            assert_area(s.area(), nodes, e, name + " before")
            assert s.trim(a["conds"], a["rxy"], a["sign_rxy"]) == unused
            rec = s.last_launch()
            assert rec["op"] == "trim" and (rec["nodes"], rec["elements"], rec["nodes_kept"], rec["nodes_out"], rec["elements_out"], rec["values"]) == \
                (len(nodes), len(e), len(n2) + unused, len(n2), len(e2), n2.size), (name, rec)
            assert rec["kernels"] == 4
            assert s.counts() == (len(n2), len(e2), nodes.shape[1])
            got = s.read(fill=SENT_GPU)
            assert_surface(got, n2, e2, name)
            assert_area(s.area(), n2, e2, name + " after")
            with pytest.raises(capi.PaError, match="no slice has been computed"):
                s.slice_read()
            res.append(got)
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()
    if "everything" in name:
        assert len(n2) == 0 and len(e2) == 0
    if "nothing" in name:
        assert n2.tobytes() == nodes.tobytes() and e2.tobytes() == e.tobytes()


@pytest.mark.parametrize("name,comp,loc", SC.TRIM_THEN_SLICE)
def test_trim_then_slice_stays_on_the_device(ctx, name, comp, loc):
    nodes, e = SC.trim_surface(name)
    n2, e2, _ = ref_trim(name)
    want = R.slice_surface(n2, e2, comp, loc)
    assert len(want["segs"]) > 0
    a = SC.trim_args(name)
    with capi.Surf(ctx, nodes, e) as s:
        s.slice(comp, loc)  # a slice of the untrimmed surface first: the trim must drop it
        s.trim(a["conds"], a["rxy"], a["sign_rxy"])
        assert_area(s.area(), n2, e2, name)
        assert s.slice(comp, loc) == (len(want["verts"]), len(want["segs"]))
        assert_slice(s.slice_read(fill=SENT_GPU), want, name + " trimmed, then cut")
        assert s.trim() == 0  # nothing left to remove: the same surface again
        assert_surface(s.read(fill=SENT_GPU), n2, e2, name + " second trim")


def test_bad_input_is_refused(ctx):
    nodes, e = SC.slice_surface("octahedron_z")
    bad = e.copy()
    bad[3, 1] = 7
    with pytest.raises(capi.PaError, match="element 4 names a node that does not exist"):
        capi.Surf(ctx, nodes, bad)
    bad[3, 1] = 0
    with pytest.raises(capi.PaError, match="element 4 names a node that does not exist"):
        capi.Surf(ctx, nodes, bad)
    with pytest.raises(capi.PaError, match="needs the node coordinates x, y, z"):
        capi.Surf(ctx, nodes[:, :2], e)
    import ctypes as C
    one = np.zeros(3)
    h = ctx.lib.pa_surf_create(ctx.h, 2 ** 31, 3, one.ctypes.data_as(C.POINTER(C.c_double)), 0, None)  # refused before any array is read
    assert not h and "more than 2^31 - 1 nodes or 3 * nelts" in ctx.lib.pa_last_error(ctx.h).decode()
    with capi.Surf(ctx, nodes, e) as s:
        with pytest.raises(capi.PaError, match="component 3 is not one of the 3 node components"):
            s.slice(3, 0.0)
        with pytest.raises(capi.PaError, match="not a number"):
            s.slice(0, float("nan"))
        with pytest.raises(capi.PaError, match="no slice has been computed"):
            s.slice_read()
        with pytest.raises(capi.PaError, match="component 5 is not one of"):
            s.trim([(5, "lt", 0.0)])
        with pytest.raises(capi.PaError, match=r"Use one of \[lt,le,gt,ge,eq\]"):
            s.trim([(0, "ne", 0.0)])
        assert_surface(s.read(fill=SENT_GPU), nodes, e, "refused calls leave the surface alone")


# ------------------------------------------------------------------------------------------------ the tools, end to end
def _names(nc):
    return ["X", "Y", "Z"] + ["f%d" % c for c in range(3, nc)]


def _write_mef(path, nodes, e, title="0.125"):
    with open(path, "wb") as fh:
        fh.write(R.mef_bytes(nodes, e, title, _names(nodes.shape[1])))


def _run(exe, args, cwd):
    return subprocess.run([os.path.join(BIN, exe)] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name,extra", [("octahedron_z", {}), ("grid8", {}), ("grid64", {}), ("ico1280_c4", {}), ("ico5120_c11", {}), ("fin_degree3", {}),
                                        ("duplicate_element", {}), ("two_spheres", {}), ("shared_edge_ba", {}), ("ico320_c3", dict(write_mef=0)),
                                        ("ico1283", dict(write_tec=0))])
def test_slice_tool_end_to_end(tmp_path, name, extra):
    """sliceMEF3d.ex: every .dat as text and every .mef byte for byte; the stderr lines; all locations of one direction in one run"""
    nodes, e = SC.slice_surface(name)
    names = _names(nodes.shape[1])
    _write_mef(tmp_path / "surf.iso.mef", nodes, e)
    by_dir = {}
    for comp, loc in SC.SLICES[name][1]:
        by_dir.setdefault(comp, []).append(loc)
    if name == "ico1280_c4":
        by_dir = {0: [-0.25, 0.0, 0.125], 3: [0.2]}  # a negative, a zero and a positive location in one run
    for comp, locs in by_dir.items():
        want, err = R.run_slice_tool("surf.iso.mef", nodes, e, "0.125", names, comp, locs, bool(extra.get("write_tec", 1)), bool(extra.get("write_mef", 1)))
        out = _run("sliceMEF3d.ex", ["infile=surf.iso.mef", "dir=%d" % comp, "locs=" + " ".join(repr(float(v)) for v in locs)] + ["%s=%d" % kv for kv in extra.items()],
                   tmp_path)
        assert out.returncode == 0, out.stderr
        assert out.stderr.split("\n")[:len(err)] == err
        for f, body in want.items():
            if f.endswith(".dat"):
                assert open(tmp_path / f).read() == body, f
            else:
                assert open(tmp_path / f, "rb").read() == body, f
            os.remove(tmp_path / f)
        assert sorted(os.listdir(tmp_path)) == ["surf.iso.mef"], "files the reference does not write"


def test_slice_tool_defaults_and_an_empty_cut(tmp_path):
    nodes, e = SC.slice_surface("miss")
    names = _names(nodes.shape[1])
    _write_mef(tmp_path / "s.mef", nodes, e)
    want, err = R.run_slice_tool("s.mef", nodes, e, "0.125", names)  # dir 0, one location, 0
    out = _run("sliceMEF3d.ex", ["infile=s.mef"], tmp_path)
    assert out.returncode == 0 and out.stderr.split("\n")[:len(err)] == err
    assert sorted(want) == ["s_X_0.dat", "s_X_0.mef"] and open(tmp_path / "s_X_0.mef", "rb").read() == want["s_X_0.mef"]
    assert open(tmp_path / "s_X_0.dat").read() == want["s_X_0.dat"]
    # a location that cuts nothing: the .dat with its VARIABLES line only, no .mef, a line on stderr
    want, err = R.run_slice_tool("s.mef", nodes, e, "0.125", names, 2, [5.0])
    out = _run("sliceMEF3d.ex", ["infile=s.mef", "dir=2", "locs=5"], tmp_path)
    assert out.returncode == 0 and out.stderr.split("\n")[:len(err)] == err and "cuts nothing" in err[-1]
    assert open(tmp_path / "s_Z_p5.dat").read() == 'VARIABLES = "X" "Y" "Z" \n' == want["s_Z_p5.dat"]
    assert not os.path.exists(tmp_path / "s_Z_p5.mef")
    assert _run("sliceMEF3d.ex", ["infile=s.mef", "dir=3"], tmp_path).returncode != 0


@pytest.mark.parametrize("name,extra", [("grid_gt", {}), ("grid_eq_unused", dict(do_area_stats=1)), ("ico_rxy_cond", dict(do_area_stats=1)),
                                        ("ico_two", dict(remComps=[3, 1])), ("grid_nothing", {}), ("grid64_two", dict(do_area_stats=1, remComps=[4])),
                                        ("ico_eq", {}), ("ico1283_unused", {})])
def test_trim_tool_end_to_end(tmp_path, name, extra):
    """trimMEFgen3d.ex writes, byte for byte, the MEF of the restatement; stdout carries the reference's lines"""
    nodes, e = SC.trim_surface(name)
    a = SC.trim_args(name)
    _write_mef(tmp_path / "in.mef", nodes, e, title="flame 7")
    want, lines = R.run_trim_tool(nodes, e, "flame 7", _names(nodes.shape[1]), a["conds"], a["rxy"], a["sign_rxy"], tuple(extra.get("remComps", ())),
                                  bool(extra.get("do_area_stats", 0)))
    args = ["infile=in.mef", "outfile=out.mef"]
    if a["conds"]:
        args += ["comps=" + " ".join(str(c[0]) for c in a["conds"]), "signs=" + " ".join(c[1] for c in a["conds"]), "vals=" + " ".join(repr(float(c[2])) for c in a["conds"])]
    if a["rxy"] >= 0:
        args += ["RXY=%r" % a["rxy"], "sign_RXY=" + a["sign_rxy"]]
    if "remComps" in extra:
        args.append("remComps=" + " ".join(str(c) for c in extra["remComps"]))
    if "do_area_stats" in extra:
        args.append("do_area_stats=1")
    out = _run("trimMEFgen3d.ex", args, tmp_path)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:len(lines)] == lines and out.stdout.count("\n") == len(lines)
    assert open(tmp_path / "out.mef", "rb").read() == want


def test_trim_tool_refusals(tmp_path):
    nodes, e = SC.trim_surface("grid_everything")
    _write_mef(tmp_path / "in.mef", nodes, e)
    out = _run("trimMEFgen3d.ex", ["infile=in.mef", "outfile=out.mef", "comps=1", "signs=ge", "vals=0"], tmp_path)  # removes everything
    assert out.returncode != 0 and "remove every element" in out.stderr and not os.path.exists(tmp_path / "out.mef")
    assert out.stdout.split("\n")[0] == "Surface area before: 1"
    out = _run("trimMEFgen3d.ex", ["infile=in.mef", "outfile=out.mef", "comps=1", "signs=ne", "vals=0"], tmp_path)
    assert out.returncode != 0 and "Bad signs data. Use one of [lt,le,gt,ge,eq]" in out.stderr and "i,signs[i] 0,ne" in out.stdout
    out = _run("trimMEFgen3d.ex", ["infile=in.mef", "outfile=out.mef", "RXY=0.5", "sign_RXY=xx"], tmp_path)
    assert out.returncode != 0 and "Bad sign data.  Use one of [lt,le,gt,ge,eq]" in out.stderr and "sign_RXY: xx" in out.stdout
    assert not os.path.exists(tmp_path / "out.mef")
    with open(tmp_path / "quad.mef", "wb") as fh:  # nodesPerElt = 4
        fh.write(R.mef_bytes(nodes, e[:4], "t", _names(nodes.shape[1])).replace(b"\n4 3\n", b"\n3 4\n", 1))
    for exe, args in (("trimMEFgen3d.ex", ["infile=quad.mef", "outfile=out.mef"]), ("sliceMEF3d.ex", ["infile=quad.mef"])):
        out = _run(exe, args, tmp_path)
        assert out.returncode != 0 and "needs 3 nodes per element" in out.stderr
