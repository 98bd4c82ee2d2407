"""GPU tier: the hex-element mesh kernels (peleanalysis_amd/csrc/pa_amrtofe.hip) through capi.FeMesh, and amrToFE3d.ex end to end,
against the plain-Python restatement of amrToFE.cpp (tests/amrtofe_ref.py, pinned by tests/test_amrtofe_ref.py).  Everything is an
integer or a copied / once-rounded double, so every comparison is for equality: node order, connectivity, node data, file bytes."""
import os
import subprocess

import numpy as np
import pytest

import amrtofe_cases as Cs
import amrtofe_ref as R
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab
from peleanalysis_amd.plotfile import write_plotfile
from util import bits_equal

pytestmark = pytest.mark.gpu


def run_mesh(ctx, levels, ratios, states=None, comps=(0, 1), **kw):
    """-> (nlev, nodes [ids][4], conn, node data or None)"""
    dls = [capi.DevLevel(ctx, l) for l in levels]
    mfs = []
    try:
        with capi.FeMesh(ctx, dls, ratios, **kw) as fe:
            nodes, conn = fe.nodes(), fe.connectivity()
            assert conn.shape == (fe.nelts, 8)
            data = None
            if states is not None:
                mfs = [capi.DevMF.from_host(ctx, dl, s) for dl, s in zip(dls[:fe.nlev], states)]
                data = fe.gather(mfs, comps)
            return fe.nlev, nodes, conn, data
    finally:
        for m in mfs:
            m.close()
        for dl in dls:
            dl.close()


def check(ctx, name, ref=None, levels=None, **kw):
    lv, ratios, key = Cs.case(name)
    levels = levels if levels is not None else lv
    ref = ref if ref is not None else Cs.reference(name)
    st = Cs.states(name)
    nlev, nodes, conn, data = run_mesh(ctx, levels, ratios, st, subbox=kw.pop("subbox", key), **kw)
    assert nlev == ref.nlev
    assert nodes.tolist() == [list(n[:4]) for n in ref.nodes], "node order"
    assert np.array_equal(conn, ref.conn), "connectivity"
    assert bits_equal(data, ref.node_data(st, [0, 1])), "node data"
    return nodes, conn, data


@pytest.mark.parametrize("name", list(Cs.KNOWN))
def test_known_cases(ctx, name):
    nodes, conn, _ = check(ctx, name)
    assert (len(nodes), len(conn)) == Cs.KNOWN[name][3:5]


@pytest.mark.parametrize("name", Cs.LARGER)
def test_larger_cases(ctx, name):
    """unions of rectangles with concave coarse-fine corners and boxes of different sizes side by side; three nested levels; base32:
    240 workgroups of cells, 32 key bits in the element sort"""
    check(ctx, name)


def test_same_input_same_bytes(ctx):
    a = check(ctx, "union9")
    b = check(ctx, "union9")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_shuffled_box_order_renumbers_as_the_reference(ctx):
    name = "union12"
    levels, ratios, _ = Cs.case(name)
    rng = np.random.default_rng(5)
    shuf = [Level(l.boxes[rng.permutation(l.nboxes)], l.domlo, l.domhi, l.is_per, l.prob_lo, l.prob_hi) for l in levels]
    ref = R.FeMeshRef(shuf, ratios)
    base = Cs.reference(name)
    assert ref.nodes != base.nodes and ref.elements == base.elements  # other ids, the same set of elements
    lv, rr, _ = Cs.case(name)
    dls_states = []
    for l in shuf:  # the states on the shuffled boxes
        m = MultiFab(l, 2, 0)
        dls_states.append(m)
    st0 = Cs.states(name)
    for m, s, l0 in zip(dls_states, st0, levels):
        for b in range(m.level.nboxes):
            src = int(np.nonzero((l0.boxes == m.level.boxes[b]).all(axis=1))[0][0])
            m.valid(b)[...] = s.valid(src)
    nlev, nodes, conn, data = run_mesh(ctx, shuf, ratios, dls_states)
    assert nodes.tolist() == [list(n[:4]) for n in ref.nodes]
    assert np.array_equal(conn, ref.conn)
    assert bits_equal(data, ref.node_data(dls_states, [0, 1]))


def test_finest_level_and_emptied_level(ctx):
    check(ctx, "three", ref=Cs.reference("three", finest_level=1), finest_level=1)
    check(ctx, "nested16", ref=Cs.reference("nested16", finest_level=0), finest_level=0)
    ref = Cs.reference("centred", box=(0, 0, 0, 1, 7, 7))  # no box of level 1 touches the refined box: the hierarchy ends (:445-451)
    assert ref.nlev == 1
    check(ctx, "centred", ref=ref, subbox=(0, 0, 0, 1, 7, 7))


def test_connect_cc_0(ctx):
    for name in ("centred", "union10"):
        levels, ratios, key = Cs.case(name)
        ref = Cs.reference(name, connect_cc=False)
        st = Cs.states(name)
        nlev, nodes, conn, data = run_mesh(ctx, levels, ratios, st, subbox=key, connect_cc=False)
        assert nodes.tolist() == [list(n[:4]) for n in ref.nodes]
        assert np.array_equal(conn, ref.conn) and conn.shape == (ref.nnodes, 8)
        assert bits_equal(data, ref.node_data(st, [0, 1]))


def test_gather_more_components_than_one_launch_takes(ctx):
    """19 components in a shuffled order: the gather runs in launches of 16, the later ones behind the coordinates and the first 16 rows"""
    name = "union10"
    levels, ratios, key = Cs.case(name)
    ref = Cs.reference(name)
    rng = np.random.default_rng(11)
    st = []
    for l in levels:
        m = MultiFab(l, 19, 0)
        m.data[:] = rng.uniform(-1.0, 1.0, size=m.data.shape)
        st.append(m)
    comps = [int(c) for c in rng.permutation(19)]
    _, _, _, data = run_mesh(ctx, levels, ratios, st, comps=comps, subbox=key)
    assert data.shape == (22, ref.nnodes) and bits_equal(data, ref.node_data(st, comps))


def test_refusals_of_the_library(ctx):
    with pytest.raises(capi.PaError, match="not aligned"):
        run_mesh(ctx, [Cs.lv(Cs.BASE, 8), Cs.lv([[5, 4, 4, 10, 11, 11]], 16)], [2])
    with pytest.raises(capi.PaError, match="Node not found"):
        run_mesh(ctx, [Cs.lv([[0, 0, 0, 3, 7, 7], [4, 0, 0, 7, 3, 7]], 8)], [])
    # ... but only as a corner of a kept cube: the same ghost cells, no cube (as the restatement, tests/test_amrtofe_ref.py)
    half = [Cs.lv([[0, 0, 0, 3, 7, 7]], 8)]
    nlev, nodes, conn, _ = run_mesh(ctx, half, [], subbox=(0, 4, 0, 4, 4, 7))
    ref = R.FeMeshRef(half, [], (0, 4, 0, 4, 4, 7))
    assert nodes.tolist() == [list(n[:4]) for n in ref.nodes] and len(nodes) == 32 and conn.shape == (0, 8)
    with pytest.raises(capi.PaError, match="Node not found"):
        run_mesh(ctx, half, [], subbox=(0, 4, 0, 4, 5, 7))
    with pytest.raises(capi.PaError, match="does not intersect"):
        run_mesh(ctx, [Cs.lv(Cs.BASE, 8)], [], subbox=(9, 9, 9, 12, 12, 12))
    levels, ratios, _ = Cs.case("centred")
    with pytest.raises(capi.PaError, match="component out of range"):
        run_mesh(ctx, levels, ratios, Cs.states("centred"), comps=(0, 2))


# ----------------------------------------------------------------------------- amrToFE3d.ex end to end
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")
VARS = ["temp", "Y(H2)"]


def _tool(args, cwd):
    return subprocess.run([os.path.join(BIN, "amrToFE3d.ex")] + args, cwd=cwd, capture_output=True, timeout=600)


@pytest.mark.parametrize("name", ["three", "ratio4"])
def test_tool_end_to_end(tmp_path, name):
    H, st, ref = Cs.hierarchy_of(name), Cs.states(name), Cs.reference(name)
    p = str(tmp_path / "plt")
    t = 0.000125
    write_plotfile(p, H, st, VARS, time=t)
    D = ref.node_data(st, [0, 1])
    r = _tool(["infile=" + p], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == "outfile: " + p + ".dat\n"
    progress = ["Before nodes allocated", "After nodes allocated", "After nodeMap built, size=%d" % ref.nnodes,
                "Before connData allocated %d elements" % ref.nelts, "After connData allocated %d elements" % ref.nelts, "Final elements built",
                "Final nodeVect built (%d nodes)" % ref.nnodes, "Temp nodes, elements cleared"]
    progress += ["My data set alloc'd at lev=%d" % l for l in range(ref.nlev)]
    progress += ["File data loaded", "Final node data allocated (size=%d)" % (5 * ref.nnodes)]
    assert [l for l in r.stderr.decode().splitlines() if l in progress] == progress  # in this order, each once (the runtime may add lines of its own)
    assert open(p + ".dat", "rb").read() == R.write_tec(p, t, VARS, D, ref.conn)
    r = _tool(["infile=" + p, "outType=flt"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout.decode() == "outfile: " + p + ".flt\n"
    flt = R.write_flt(p, t, VARS, D, ref.conn)
    assert open(p + ".flt", "rb").read() == flt
    r = _tool(["infile=" + p, "outType=flt", "outfile=-"], tmp_path)
    assert r.returncode == 0 and r.stdout == b"outfile: -\n" + flt
    # one component out of two, a box, a lower finest level, a named outfile
    ref2 = Cs.reference(name, finest_level=0, box=(1, 0, 2, 6, 7, 7))
    r = _tool(["infile=" + p, "outType=flt", "comps=1", "box=1 0 2 6 7 7", "finestLevel=0", "outfile=sub.flt"], tmp_path)
    assert r.returncode == 0 and r.stdout == b"outfile: sub.flt\n"
    assert open(tmp_path / "sub.flt", "rb").read() == R.write_flt(p, t, VARS[1:], ref2.node_data(st, [1]), ref2.conn)
    # connect_cc=0
    ref3 = Cs.reference(name, connect_cc=False)
    r = _tool(["infile=" + p, "sComp=0", "nComp=1", "connect_cc=0", "outfile=cc0.dat"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert open(tmp_path / "cc0.dat", "rb").read() == R.write_tec(p, t, VARS[:1], ref3.node_data(st, [0]), ref3.conn)


def test_tool_refusals(tmp_path):
    name = "centred"
    H, st = Cs.hierarchy_of(name), Cs.states(name)
    p = str(tmp_path / "plt")
    write_plotfile(p, H, st, VARS, time=0.0)
    ok = ["infile=" + p]
    for args, msg in ((ok + ["nGrowPer=1"], "nGrowPer > 0"),
                      (ok + ["doBin=1"], "doBin needs TECIO"),
                      (ok + ["ngpus=2"], "ngpus > 1 is not supported"),
                      (ok + ["comps=0 2"], "comps out of range"),
                      (ok + ["sComp=1", "nComp=2"], "sComp + nComp out of range"),
                      (ok + ["box=1 1 1 4"], "box needs six values"),
                      (ok + ["finestLevel=4"], "finestLevel out of range"),
                      (ok + ["outType=vtk"], "usage:"),
                      ([], "usage:")):
        r = _tool(args, tmp_path)
        assert r.returncode != 0 and msg in r.stderr.decode(), (args, r.stderr.decode()[-300:])
        assert not os.path.exists(p + ".dat")
    # a 2-D plotfile
    l2 = Level([[0, 0, 0, 7, 7, 0]], (0, 0, 0), (7, 7, 0), (0, 0, 0), np.zeros(3), np.ones(3))
    write_plotfile(str(tmp_path / "plt2d"), Hierarchy([l2], 2), [MultiFab(l2, 2, 0)], VARS, dim=2)
    r = _tool(["infile=" + str(tmp_path / "plt2d")], tmp_path)
    assert r.returncode != 0 and "only 3-D plotfiles are supported" in r.stderr.decode()
    # a fine box that is not aligned to its ratio
    un = Hierarchy([Cs.lv(Cs.BASE, 8), Cs.lv([[5, 4, 4, 10, 11, 11]], 16)], 2)
    write_plotfile(str(tmp_path / "pltun"), un, [MultiFab(l, 2, 0, fill=1.0) for l in un.levels], VARS)
    r = _tool(["infile=" + str(tmp_path / "pltun")], tmp_path)
    assert r.returncode != 0 and "not aligned to the refinement ratio" in r.stderr.decode()
    # Bad mf data: the first selected component only
    bad = [s.copy() for s in st]
    bad[1].valid(0)[1, 2, 3, 4] = 1.0e30
    write_plotfile(str(tmp_path / "pltbad"), H, bad, VARS)
    r = _tool(["infile=" + str(tmp_path / "pltbad"), "comps=1 0"], tmp_path)
    assert r.returncode != 0 and "Bad mf data" in r.stderr.decode() and not os.path.exists(str(tmp_path / "pltbad") + ".dat")
    assert not os.path.exists(tmp_path / "out.mfab")
    assert _tool(["infile=" + str(tmp_path / "pltbad"), "comps=0 1"], tmp_path).returncode == 0
    # counts beyond int: the Header of a one-box 1300^3 level (no data is read before the mesh is built)
    big = str(tmp_path / "pltbig")
    one = Hierarchy([Cs.lv(Cs.BASE, 8)], 2)
    write_plotfile(big, one, [MultiFab(one.levels[0], 2, 0)], VARS)
    for f in ("Header", os.path.join("Level_0", "Cell_H")):
        txt = open(os.path.join(big, f)).read().replace("(7,7,7)", "(1299,1299,1299)")
        open(os.path.join(big, f), "w").write(txt)
    r = _tool(["infile=" + big], tmp_path)
    assert r.returncode != 0 and "beyond int" in r.stderr.decode(), r.stderr.decode()[-300:]
