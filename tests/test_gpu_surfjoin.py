"""GPU tier: the surface joining kernels (peleanalysis_amd/csrc/pa_surfjoin.hip) through capi.Surf, and mergeMEF3d.ex / combineMEF3d.ex /
scaleMEF3d.ex / multMEF3d.ex end to end, against the restatement tests/surfjoin_ref.py.  For every case of tests/surfjoin_cases.py: the
nodes as uint64 bits and the elements exactly; output arrays start as the payload NaN of tests/util.py ("writes each output");
pa_surf_last_launch must report the case's counts and the path the case was written for.  Every merge case runs under method 0, 1 and
2: the results must be byte-identical to each other and to the restatement, and a case that cannot take the grid asserts the refusal."""
import functools
import os

import numpy as np
import pytest

import surfcut_ref as CR
import surfjoin_cases as JC
import surfjoin_ref as R
from peleanalysis_amd import capi
from test_gpu_surfcut import _names, _run, assert_slice, assert_surface
from util import SENT_GPU

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def ref_chain(name):
    """the surface after each step of a case: [(nodes, elts, info), ...]"""
    c = JC.merge_case(name)
    nodes, elts = c["M"]
    out = []
    for s in c["S"]:
        nodes, elts, info = R.merge_iso(nodes, elts, s[0], s[1], c["eps"], c["rem"], rows=True)
        out.append((nodes, elts, info))
    return out


def expected_kernels(n_m, n_s, ne_m, ne_s, rem, method, path, nnew):
    """what pa_surfjoin_merge launches (scans and sorts not counted)"""
    if n_s == 0:
        return 0
    k = 1  # flags
    if not rem:
        k += 1
    else:
        if method != 2:
            k += (1 if n_m else 0) + 1  # bounds of M, of S
        k += 3 if path == "grid" else 1  # keys, sorted coordinates, probe | brute force
    if nnew:
        k += (1 if n_m else 0) + 1 + (1 if ne_m else 0) + (1 if ne_s else 0)
    return k


def run_merge(ctx, name, method):
    """-> the final (nodes, elts), or None where the method is refused (asserted here)"""
    c = JC.merge_case(name)
    want = ref_chain(name)
    m_nodes, m_elts = c["M"]
    with capi.Surf(ctx, m_nodes, m_elts) as m:
        for step, s in enumerate(c["S"]):
            path = c["path"][step]
            w_nodes, w_elts, info = want[step]
            with capi.Surf(ctx, s[0], s[1]) as t:
                if method == 1 and path == "brute":
                    with pytest.raises(capi.PaError, match="the grid path cannot be taken"):
                        m.merge(t, c["eps"], c["rem"], 1)
                    assert_surface(m.read(fill=SENT_GPU), m_nodes, m_elts, name + ": a refused merge leaves M alone")
                    return None
                assert m.merge(t, c["eps"], c["rem"], method) == info["appended"], (name, step, method)
                assert_surface(t.read(fill=SENT_GPU), s[0], s[1], name + ": S is not changed")
            rec = m.last_launch()
            took = path if method == 0 or path == "append" else ("grid" if method == 1 else "brute")
            n_fin = int(np.isfinite(m_nodes[:, :3]).all(axis=1).sum())
            assert rec["op"] == "merge" and rec["path"] == took, (name, step, method, rec)
            assert (rec["nodes_in"], rec["table"]) == (len(s[0]), n_fin if took == "grid" else 0), (name, step, method, rec)
            if len(s[0]):
                assert (rec["duplicates"], rec["nodes_appended"], rec["elements_appended"]) == \
                    (info["duplicates"], info["nodes_appended"], info["elements_appended"]), (name, step, method, rec)
            assert rec["kernels"] == expected_kernels(len(m_nodes), len(s[0]), len(m_elts), len(s[1]), c["rem"], method, took, info["nodes_appended"]), (name, step, method, rec)
            assert m.counts() == (len(w_nodes), len(w_elts), w_nodes.shape[1])
            assert_surface(m.read(fill=SENT_GPU), w_nodes, w_elts, "%s step %d method %d" % (name, step, method))
            m_nodes, m_elts = w_nodes, w_elts
        return m.read(fill=SENT_GPU)


@pytest.mark.parametrize("name", list(JC.MERGES))
def test_merges_equal_restatement(ctx, name):
    c = JC.merge_case(name)
    res = [run_merge(ctx, name, method) for method in (0, 1, 2, 0)]  # the last: a second handle must give the same bytes
    assert res[0] is not None and res[2] is not None and (res[1] is None) == ("brute" in c["path"]), name
    for r in res[1:]:
        if r is not None:
            assert r[0].tobytes() == res[0][0].tobytes() and r[1].tobytes() == res[0][1].tobytes(), name


def test_merge_refusals(ctx):
    nodes, e = JC.merge_case("seam8")["M"]
    with capi.Surf(ctx, nodes, e) as m, capi.Surf(ctx, nodes[:, :4], e) as four, capi.Surf(ctx, nodes, e) as t:
        held = m.slice(0, 0.25)
        sl = m.slice_read(fill=SENT_GPU)
        with pytest.raises(capi.PaError, match="cannot be merged into itself"):
            m.merge(m, 1.0e-8, True)
        with pytest.raises(capi.PaError, match="the grid path cannot be taken: fewer than 2 cells span M"):
            m.merge(t, 2.0, True, 1)  # refused after the bounds kernels ran
        with pytest.raises(capi.PaError, match="5 and 4 node components"):
            m.merge(four)
        for eps in (1.0e200, float("inf"), float("nan")):
            with pytest.raises(capi.PaError, match=r"eps \* eps is not finite"):
                m.merge(t, eps, True)
        with pytest.raises(capi.PaError, match="method is 0"):
            m.merge(t, 1.0e-8, True, 3)
        two = m.select([(0, 0), (0, 3)])
        with two, t.select([(0, 0), (0, 3)]) as two_t:
            with pytest.raises(capi.PaError, match="remDupNodes needs the node coordinates"):
                two.merge(two_t, 1.0e-8, True)
            with pytest.raises(capi.PaError, match="pa_surf_area: needs the node coordinates"):
                two.area()
            with pytest.raises(capi.PaError, match="RXY needs the node coordinates"):
                two.trim([], 0.5, "lt")
            assert two.merge(two_t) and two.counts() == (2 * len(nodes), 2 * len(e), 2)  # a plain append compares nothing
            assert two.trim([(1, "lt", 0.0)]) >= 0 and two.slice(1, 0.25)[1] >= 0       # conditions and slices need no coordinates
        assert_surface(m.read(fill=SENT_GPU), nodes, e, "refused calls leave the surface alone")
        # ... and the slice it held and its launch record
        assert held[1] > 0 and m.last_launch()["op"] == "slice" and m.last_launch()["segments"] == held[1]
        for a, b in zip(sl, m.slice_read(fill=SENT_GPU)):
            assert a.tobytes() == b.tobytes()


def test_merge_scale_select_trim_slice_on_one_handle(ctx):
    """the chain stays on the device and equals the restatements composed; a slice M held is dropped by the merge"""
    c = JC.merge_case("seam64")
    (a, ea), (b, eb) = c["M"], c["S"][0]
    n1, e1, _ = ref_chain("seam64")[0]
    n2 = R.scale(n1, [3, 4, 3], [2.0, -0.5, 0.25])
    n3 = R.select(n2, None, [(0, 0), (0, 1), (0, 2), (0, 4), (0, 3)])
    n4, e4, unused = CR.trim_surface(n3, e1, conds=[(3, "gt", 0.3)])
    want = CR.slice_surface(n4, e4, 0, 0.3)
    assert len(want["segs"]) > 0 and len(n4) < len(n3)
    with capi.Surf(ctx, a, ea) as m, capi.Surf(ctx, b, eb) as t:
        m.slice(1, 0.5)
        assert m.merge(t, c["eps"], True)
        with pytest.raises(capi.PaError, match="no slice has been computed"):
            m.slice_read()
        m.scale([3, 4, 3], [2.0, -0.5, 0.25])
        assert m.last_launch() == dict(op="scale", values=3 * len(n1), kernels=3)
        assert_surface(m.read(fill=SENT_GPU), n2, e1, "merged, scaled")
        with m.select([(0, 0), (0, 1), (0, 2), (0, 4), (0, 3)]) as s:
            assert s.trim([(3, "gt", 0.3)]) == unused
            assert_surface(s.read(fill=SENT_GPU), n4, e4, "merged, scaled, selected, trimmed")
            assert s.slice(0, 0.3) == (len(want["verts"]), len(want["segs"]))
            assert_slice(s.slice_read(fill=SENT_GPU), want, "the chain's slice")
        # and on the ONE handle: merge -> scale (above) -> trim -> slice
        n5, e5, unused5 = CR.trim_surface(n2, e1, conds=[(4, "gt", 0.3)])
        want5 = CR.slice_surface(n5, e5, 0, 0.3)
        assert m.trim([(4, "gt", 0.3)]) == unused5
        assert_surface(m.read(fill=SENT_GPU), n5, e5, "merged, scaled, trimmed")
        assert m.slice(0, 0.3) == (len(want5["verts"]), len(want5["segs"])) and len(want5["segs"]) > 0
        assert_slice(m.slice_read(fill=SENT_GPU), want5, "one handle's slice")


@pytest.mark.parametrize("name", list(JC.SCALES))
def test_scale_equals_restatement(ctx, name):
    build, comps, vals = JC.SCALES[name]
    nodes, e = build()
    want = R.scale(nodes, comps, vals)
    res = []
    for _ in range(2):
        with capi.Surf(ctx, nodes, e) as s:
            s.scale(comps, vals)
            assert s.last_launch() == dict(op="scale", values=len(comps) * len(nodes), kernels=len(comps))
            got = s.read(fill=SENT_GPU)
            assert got[0].shape == want.shape and got[0].view(np.uint64).tolist() == want.view(np.uint64).tolist() and np.array_equal(got[1], e), name
            res.append(got)
            with pytest.raises(capi.PaError, match="component 9 is not one of"):
                s.scale([9], [1.0])
    assert res[0][0].tobytes() == res[1][0].tobytes()


@pytest.mark.parametrize("name", list(JC.PRODUCTS))
def test_product_equals_restatement(ctx, name):
    build, comps = JC.PRODUCTS[name]
    nodes, e = build()
    want = R.product(nodes, comps)
    with capi.Surf(ctx, nodes, e) as s:
        outs = []
        for _ in range(2):
            with s.product(comps) as p:
                assert p.counts() == (len(nodes), len(e), 1)
                assert p.last_launch() == dict(op="product", values=len(nodes), kernels=2) and s.last_launch() == {"op": None}  # the record is the new handle's
                got = p.read(fill=SENT_GPU)
                assert got[0].view(np.uint64).tolist() == want.view(np.uint64).tolist() and np.array_equal(got[1], e), name
                outs.append(got[0].tobytes())
        assert outs[0] == outs[1]
        with pytest.raises(capi.PaError, match="component 7 is not one of"):
            s.product([0, 7])
        with pytest.raises(capi.PaError, match="takes 1 to 32 components"):
            s.product([])
        assert_surface(s.read(fill=SENT_GPU), nodes, e, "the source is not changed")


@pytest.mark.parametrize("name", list(JC.SELECTS))
def test_select_equals_restatement(ctx, name):
    bl, br, sel = JC.SELECTS[name]
    (nl, e), r = bl(), (br() if br else None)
    want = R.select(nl, r[0] if r else None, sel)
    with capi.Surf(ctx, nl, e) as sl:
        sr = capi.Surf(ctx, r[0], r[1]) if r else None
        try:
            outs = []
            for _ in range(2):
                with sl.select(sel, sr) as o:
                    assert o.counts() == (len(nl), len(e), len(sel))
                    assert o.last_launch() == dict(op="select", values=len(sel) * len(nl), kernels=len(sel) + 1) and sl.last_launch() == {"op": None}
                    got = o.read(fill=SENT_GPU)
                    assert got[0].shape == want.shape and got[0].view(np.uint64).tolist() == want.view(np.uint64).tolist() and np.array_equal(got[1], e), name
                    outs.append(got[0].tobytes())
            assert outs[0] == outs[1]
        finally:
            if sr:
                sr.close()
        with pytest.raises(capi.PaError, match="there is no R"):
            sl.select([(1, 0)])
        with pytest.raises(capi.PaError, match=r"component 9 is not one of the \d node components of L"):
            sl.select([(0, 9)])
        with capi.Surf(ctx, nl, e[:-1]) as fewer_elts, capi.Surf(ctx, nl[:-1], np.minimum(e, len(nl) - 1)) as fewer_nodes:
            with pytest.raises(capi.PaError, match="MEF files not compible"):
                sl.select([(1, 0)], fewer_elts)
            with pytest.raises(capi.PaError, match="the node counts differ"):
                sl.select([(1, 0)], fewer_nodes)


# ------------------------------------------------------------------------------------------------ the tools, end to end
def _write(path, nodes, e, title="0.125", names=None):
    with open(path, "wb") as fh:
        fh.write(R.mef_bytes(nodes, e, title, names or _names(nodes.shape[1])))


@pytest.mark.parametrize("name,verbose", [("seam8", 1), ("append_coincident", 0), ("three_files", 1), ("all_duplicates", 0), ("eps_ge_extent", 0), ("coords_1e300", 0), ("nonfinite", 0), ("seam64", 0)])
def test_merge_tool_end_to_end(tmp_path, name, verbose):
    """mergeMEF3d.ex writes, byte for byte, the MEF of the restatement; stdout carries the reference's lines"""
    c = JC.merge_case(name)
    files = [("f0.mef",) + c["M"]] + [("f%d.mef" % (k + 1),) + s for k, s in enumerate(c["S"])]
    for f, n, e in files:
        _write(tmp_path / f, n, e, title="flame " + f)
    nodes, elts, lines, nothing = R.run_merge_tool(files, "out.mef", c["eps"], c["rem"], bool(verbose))
    args = ["infiles=" + " ".join(f for f, _, _ in files), "outfile=out.mef", "eps=%r" % c["eps"], "remDupNodes=%d" % c["rem"]] + (["verbose=1"] if verbose else [])
    out = _run("mergeMEF3d.ex", args, tmp_path)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split("\n")[:len(lines)] == lines and out.stdout.count("\n") == len(lines)
    assert out.stderr.count("nothing of it is appended") == nothing
    assert open(tmp_path / "out.mef", "rb").read() == R.mef_bytes(nodes, elts, "flame f0.mef", _names(nodes.shape[1]))


def test_merge_tool_defaults_and_refusals(tmp_path):
    c = JC.merge_case("seam8")
    (a, ea), (b, eb) = c["M"], c["S"][0]
    _write(tmp_path / "a.mef", a, ea)
    _write(tmp_path / "b.mef", b, eb)
    out = _run("mergeMEF3d.ex", ["infiles=a.mef b.mef", "outfile=out.mef"], tmp_path)  # the defaults: nothing is compared
    n, e, _ = R.merge_iso(a, ea, b, eb)
    assert out.returncode == 0 and out.stdout == "Writing out.mef\n" and open(tmp_path / "out.mef", "rb").read() == R.mef_bytes(n, e, "0.125", _names(5))
    os.remove(tmp_path / "out.mef")
    _write(tmp_path / "renamed.mef", b, eb, names=["X", "Y", "Z", "f3", "other"])
    _write(tmp_path / "four.mef", b[:, :4], eb)
    with open(tmp_path / "quad.mef", "wb") as fh:
        fh.write(R.mef_bytes(b, eb[:4], "t", _names(5)).replace(b"\n4 3\n", b"\n3 4\n", 1))
    for args, text in ((["infiles=a.mef renamed.mef"], "Incompatible files"), (["infiles=a.mef four.mef"], "Incompatible files"),
                       (["infiles=a.mef quad.mef"], "needs 3 nodes per element"), (["infiles=a.mef b.mef", "eps=1e200", "remDupNodes=1"], "eps * eps is not finite"),
                       (["infiles=a.mef missing.mef"], "Unable to open file")):
        out = _run("mergeMEF3d.ex", args + ["outfile=out.mef"], tmp_path)
        assert out.returncode != 0 and text in out.stderr and not os.path.exists(tmp_path / "out.mef"), (args, out.stderr)


def test_small_tools_end_to_end(tmp_path):
    """scaleMEF3d.ex, multMEF3d.ex and combineMEF3d.ex, the last also on the one-component file multMEF3d.ex writes"""
    build, comps, vals = JC.SCALES["twice"]
    nodes, e = build()
    names = _names(5)
    _write(tmp_path / "in.mef", nodes, e, title="t 1")
    out = _run("scaleMEF3d.ex", ["infile=in.mef", "outfile=s.mef", "comps=" + " ".join(map(str, comps)), "vals=" + " ".join(repr(v) for v in vals), "newNames=A B",
                                 "newComps=4 0"], tmp_path)
    assert out.returncode == 0 and out.stdout == "", out.stderr
    assert open(tmp_path / "s.mef", "rb").read() == R.mef_bytes(R.scale(nodes, comps, vals), e, "t 1", ["B", "Y", "Z", "f3", "A"])
    out = _run("scaleMEF3d.ex", ["infile=in.mef", "outfile=s2.mef", "sComp=3", "nComp=2", "vals=2 4"], tmp_path)
    assert out.returncode == 0 and open(tmp_path / "s2.mef", "rb").read() == R.mef_bytes(R.scale(nodes, [3, 4], [2.0, 4.0]), e, "t 1", names)
    out = _run("multMEF3d.ex", ["infile=in.mef", "outfile=p.mef", "comps=3 4 3"], tmp_path)
    assert out.returncode == 0 and out.stdout == "", out.stderr
    assert open(tmp_path / "p.mef", "rb").read() == R.mef_bytes(R.product(nodes, [3, 4, 3]), e, "t 1", ["product"])
    out = _run("multMEF3d.ex", ["infile=in.mef", "outfile=p1.mef", "sComp=4", "nameOut=sq"], tmp_path)
    assert out.returncode == 0 and open(tmp_path / "p1.mef", "rb").read() == R.mef_bytes(R.product(nodes, [4]), e, "t 1", ["sq"])
    # combine: reordered and repeated components of both files
    r_nodes, _ = JC.SELECTS["reorder"][1]()
    _write(tmp_path / "r.mef", r_nodes, e, title="other", names=["X", "Y", "Z", "g"])
    w_nodes, w_names, lines = R.run_combine_tool(nodes, names, r_nodes, ["X", "Y", "Z", "g"], [2, 0, 4], [3, 3])
    out = _run("combineMEF3d.ex", ["infileL=in.mef", "infileR=r.mef", "outfile=c.mef", "compsL=2 0 4", "compsR=3 3"], tmp_path)
    assert out.returncode == 0 and out.stdout.split("\n")[:-1] == lines, out.stderr
    assert open(tmp_path / "c.mef", "rb").read() == R.mef_bytes(w_nodes, e, "t 1", w_names)
    # the defaults take every component of both; R is the product written above
    w_nodes, w_names, lines = R.run_combine_tool(nodes, names, R.product(nodes, [3, 4, 3]), ["product"], range(5), [0])
    out = _run("combineMEF3d.ex", ["infileL=in.mef", "infileR=p.mef", "outfile=c2.mef"], tmp_path)
    assert out.returncode == 0 and out.stdout.split("\n")[:-1] == lines, out.stderr
    assert open(tmp_path / "c2.mef", "rb").read() == R.mef_bytes(w_nodes, e, "t 1", w_names)
    w_nodes, w_names, lines = R.run_combine_tool(nodes, names, r_nodes, ["X", "Y", "Z", "g"], [3, 4], [3])
    out = _run("combineMEF3d.ex", ["infileL=in.mef", "infileR=r.mef", "outfile=c3.mef", "sCompL=3", "nCompL=2", "sCompR=3", "nCompR=1"], tmp_path)
    assert out.returncode == 0 and open(tmp_path / "c3.mef", "rb").read() == R.mef_bytes(w_nodes, e, "t 1", w_names)
    # refusals: outfile stays absent
    _write(tmp_path / "fewer_elts.mef", nodes, e[:-1])
    _write(tmp_path / "fewer_nodes.mef", nodes[:-1], np.minimum(e, len(nodes) - 1))
    for exe, args, text in (("scaleMEF3d.ex", ["infile=in.mef", "comps=3 4", "vals=2"], "vals needs one value per component"),
                            ("scaleMEF3d.ex", ["infile=in.mef", "comps=5", "vals=2"], "5 is not a node variable"),
                            ("scaleMEF3d.ex", ["infile=in.mef", "vals=2", "newNames=a", "newComps=5"], "newComps: 5 is not a node variable"),
                            ("multMEF3d.ex", ["infile=in.mef", "comps=0 5"], "5 is not a node variable"),
                            ("scaleMEF3d.ex", ["infile=p.mef", "comps=0", "vals=2"], "needs the node coordinates x, y, z"),
                            ("multMEF3d.ex", ["infile=p.mef", "comps=0"], "needs the node coordinates x, y, z"),
                            ("combineMEF3d.ex", ["infileL=in.mef", "infileR=fewer_elts.mef"], "MEF files not compible"),
                            ("combineMEF3d.ex", ["infileL=in.mef", "infileR=fewer_nodes.mef"], "nodes"),
                            ("combineMEF3d.ex", ["infileL=in.mef", "infileR=r.mef", "compsR=4"], "4 is not a node variable")):
        out = _run(exe, args + ["outfile=no.mef"], tmp_path)
        assert out.returncode != 0 and text in out.stderr and not os.path.exists(tmp_path / "no.mef"), (exe, args, out.stderr)
