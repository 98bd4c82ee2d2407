"""GPU tier: the smoothing step (peleanalysis_amd/csrc/pa_surfsmooth.hip) through capi.Surf, and smoothMEF3d.ex end to end, against the
restatement tests/surfsmooth_ref.py.  For every case of tests/surfsmooth_cases.py: the nodes as uint64 bits and the elements exactly,
the neighbour CSR exactly, w and q as bits, and the launch record; output arrays start as the payload NaN of tests/util.py."""
import functools
import os

import numpy as np
import pytest

import surfcut_ref as CR
import surfjoin_cases as JC
import surfjoin_ref as JR
import surfsmooth_cases as SC
import surfsmooth_ref as R
from peleanalysis_amd import capi
from test_gpu_surfcut import _names, _run, assert_slice, assert_surface, u64
from util import SENT_GPU, sentinel_count

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def ref_structure(name, area_comp, nsmooth):
    nodes, e = SC.structure(name)
    return R.smooth(nodes, e, SC.COMP, area_comp, nsmooth, detail=True)


@functools.lru_cache(maxsize=None)
def ref_value(name):
    nodes, e, comp, area_comp, nsmooth = SC.value_case(name)
    return R.smooth(nodes, e, comp, area_comp, nsmooth, detail=True)


def expected_record(e, info, nsmooth):
    """what pa_surfsmooth_run reports: pairs, node offsets, count, weights, fill, one launch per iteration, nodes"""
    return dict(op="smooth", elements=len(e), incidence=3 * len(e), neighbours=int(info["nbr_off"][-1]), iterations=nsmooth, nodes_written=info["written"],
                max_neighbours=info["max_neighbours"], kernels=6 + nsmooth if len(e) else 0)


def check_smooth(ctx, nodes, e, comp, area_comp, nsmooth, want, info, what):
    """-> the bytes of the nodes read back"""
    with capi.Surf(ctx, nodes, e) as s:
        s.smooth(comp, area_comp, nsmooth)
        assert s.last_launch() == expected_record(e, info, nsmooth), (what, s.last_launch())
        got = s.read(fill=SENT_GPU)
        assert_surface(got, want, e, what)
        off, adj, w, q = s.smooth_read(fill=SENT_GPU)
        assert off.tolist() == info["nbr_off"].tolist() and adj.tolist() == info["nbr_adj"].tolist(), what
        assert sentinel_count(w, SENT_GPU) == 0 and sentinel_count(q, SENT_GPU) == 0, what
        assert u64(w).tolist() == u64(info["w"]).tolist(), what
        assert u64(q).tolist() == u64(info["q"]).tolist(), what
        assert s.counts() == (len(nodes), len(e), nodes.shape[1])
        return got[0].tobytes()


@pytest.mark.parametrize("name", list(SC.STRUCTURES))
def test_structures_equal_restatement(ctx, name):
    nodes, e = SC.structure(name)
    for area_comp in SC.WEIGHTS:
        for nsmooth in SC.NSMOOTH:
            want, info = ref_structure(name, area_comp, nsmooth)
            what = "%s areaComp %d nSmooth %d" % (name, area_comp, nsmooth)
            a = check_smooth(ctx, nodes, e, SC.COMP, area_comp, nsmooth, want, info, what)
            if nsmooth == 2:  # a second handle gives the same bytes
                assert check_smooth(ctx, nodes, e, SC.COMP, area_comp, nsmooth, want, info, what) == a


@pytest.mark.parametrize("name", list(SC.VALUES))
def test_value_cases_equal_restatement(ctx, name):
    nodes, e, comp, area_comp, nsmooth = SC.value_case(name)
    want, info = ref_value(name)
    check_smooth(ctx, nodes, e, comp, area_comp, nsmooth, want, info, name)


def test_hand_answers(ctx):
    nodes, e = SC.hand_surface()
    for (area_comp, nsmooth), field in SC.HAND.items():
        want = nodes.copy()
        want[:, SC.COMP] = field
        with capi.Surf(ctx, nodes, e) as s:
            s.smooth(SC.COMP, area_comp, nsmooth)
            assert_surface(s.read(fill=SENT_GPU), want, e, "by hand: areaComp %d nSmooth %d" % (area_comp, nsmooth))


def test_smooth_twice_on_one_handle_and_no_elements(ctx):
    nodes, e = SC.structure("grid12_permuted")
    w1, i1 = ref_structure("grid12_permuted", -1, 1)
    w2, i2 = R.smooth(w1, e, SC.COMP, 4, 2, detail=True)
    with capi.Surf(ctx, nodes, e) as s:
        s.smooth(SC.COMP, -1, 1)
        s.smooth(SC.COMP, 4, 2)
        assert s.last_launch() == expected_record(e, i2, 2)
        assert_surface(s.read(fill=SENT_GPU), w2, e, "smoothed twice")
        off, adj, w, q = s.smooth_read(fill=SENT_GPU)
        assert off.tolist() == i2["nbr_off"].tolist() and u64(w).tolist() == u64(i2["w"]).tolist() and u64(q).tolist() == u64(i2["q"]).tolist()
    none = np.zeros((0, 3), dtype=np.int32)
    with capi.Surf(ctx, nodes, none) as s:
        with pytest.raises(capi.PaError, match="the last operation on the surface was not a smooth"):
            s.smooth_read()
        s.smooth(SC.COMP, -1, 3)
        assert s.last_launch() == dict(op="smooth", elements=0, incidence=0, neighbours=0, iterations=3, nodes_written=0, max_neighbours=0, kernels=0)
        assert_surface(s.read(fill=SENT_GPU), nodes, none, "no elements: every node keeps its value")
        off, adj, w, q = s.smooth_read(fill=SENT_GPU)
        assert off.tolist() == [0] and len(adj) == len(w) == len(q) == 0


def test_refusals_leave_the_handle_alone(ctx):
    nodes, e = SC.structure("grid12_permuted")
    with capi.Surf(ctx, nodes, e) as s:
        held = s.slice(0, 0.3)
        sl = s.slice_read(fill=SENT_GPU)
        rec = s.last_launch()
        with pytest.raises(capi.PaError, match="component 5 is not one of the 5 node components"):
            s.smooth(5)
        with pytest.raises(capi.PaError, match="component -1 is not one of"):
            s.smooth(-1)
        with pytest.raises(capi.PaError, match="nSmooth is negative"):
            s.smooth(3, -1, -1)
        assert_surface(s.read(fill=SENT_GPU), nodes, e, "refused calls leave the surface alone")
        assert held[1] > 0 and s.last_launch() == rec and rec["op"] == "slice"
        for a, b in zip(sl, s.slice_read(fill=SENT_GPU)):
            assert a.tobytes() == b.tobytes()
        # fewer than three components: refused without an area component, and at work with one
        with s.select([(0, 4), (0, 3)]) as two:
            with pytest.raises(capi.PaError, match="need the node coordinates x, y, z"):
                two.smooth(1)
            with pytest.raises(capi.PaError, match="need the node coordinates x, y, z"):
                two.smooth(1, 2)
            assert two.last_launch()["op"] == "select"
            two.smooth(1, 0, 2)
            assert_surface(two.read(fill=SENT_GPU), R.smooth(nodes[:, [4, 3]], e, 1, 0, 2), e, "two components, areaComp 0")


def test_neighbour_lists_beyond_int_are_refused(ctx):
    """a hub of valence 46342 gives 46342 * 46341 = 2^31 + 14974 neighbour entries: refused after the count pass, the handle as it was"""
    k = 46342
    nodes, e = SC.fan(k)
    assert k * (k - 1) > 2 ** 31 - 1 >= (k - 1) * (k - 2)
    with capi.Surf(ctx, nodes, e) as s:
        held = s.slice(0, 0.3)
        sl = s.slice_read(fill=SENT_GPU)
        rec = s.last_launch()
        with pytest.raises(capi.PaError, match=r"more than 2\^31 - 1 entries \(%d\)" % (k * (k - 1))):
            s.smooth(3)
        assert_surface(s.read(fill=SENT_GPU), nodes, e, "a refused smooth leaves the surface alone")
        assert held[1] > 0 and s.last_launch() == rec
        for a, b in zip(sl, s.slice_read(fill=SENT_GPU)):
            assert a.tobytes() == b.tobytes()


def test_a_held_slice_is_dropped(ctx):
    nodes, e = SC.structure("grid12_permuted")
    with capi.Surf(ctx, nodes, e) as s:
        assert s.slice(0, 0.3)[1] > 0
        s.smooth(3)
        with pytest.raises(capi.PaError, match="no slice has been computed"):
            s.slice_read()
        want = CR.slice_surface(ref_structure("grid12_permuted", -1, 1)[0], e, 3, 0.0)
        assert s.slice(3, 0.0) == (len(want["verts"]), len(want["segs"])) and len(want["segs"]) > 0
        assert_slice(s.slice_read(fill=SENT_GPU), want, "a slice of the smoothed field")
        with pytest.raises(capi.PaError, match="the last operation on the surface was not a smooth"):
            s.smooth_read()


@functools.lru_cache(maxsize=None)
def ref_chain():
    c = JC.merge_case("seam64")
    (a, ea), (b, eb) = c["M"], c["S"][0]
    n1, e1, _ = JR.merge_iso(a, ea, b, eb, c["eps"], True, rows=True)
    n2 = R.smooth(n1, e1, 3, -1, 2)
    lo, hi = n2[:, 3].min(), n2[:, 3].max()
    cut = float(0.5 * (lo + hi))
    n3, e3, unused = CR.trim_surface(n2, e1, conds=[(3, "gt", cut)])
    x = float(np.median(n3[:, 0]))
    return n1, e1, n2, cut, n3, e3, unused, x, CR.slice_surface(n3, e3, 0, x)


def test_merge_smooth_trim_slice_on_one_handle(ctx):
    c = JC.merge_case("seam64")
    (a, ea), (b, eb) = c["M"], c["S"][0]
    n1, e1, n2, cut, n3, e3, unused, x, want = ref_chain()
    assert 0 < len(n3) < len(n2) and len(want["segs"]) > 0
    with capi.Surf(ctx, a, ea) as m, capi.Surf(ctx, b, eb) as t:
        assert m.merge(t, c["eps"], True)
        m.smooth(3, -1, 2)
        assert m.last_launch()["op"] == "smooth" and m.last_launch()["elements"] == len(e1)
        assert_surface(m.read(fill=SENT_GPU), n2, e1, "merged, smoothed")
        assert m.trim([(3, "gt", cut)]) == unused
        assert_surface(m.read(fill=SENT_GPU), n3, e3, "merged, smoothed, trimmed")
        assert m.slice(0, x) == (len(want["verts"]), len(want["segs"]))
        assert_slice(m.slice_read(fill=SENT_GPU), want, "the chain's slice")


# ------------------------------------------------------------------------------------------------ the tool, end to end
def _write(path, nodes, e, title="0.125", names=None):
    with open(path, "wb") as fh:
        fh.write(R.mef_bytes(nodes, e, title, names or _names(nodes.shape[1])))


@pytest.mark.parametrize("name,args,area_comp,nsmooth", [("grid12_permuted", [], -1, 1), ("grid12_permuted", ["areaComp=4", "nSmooth=5"], 4, 5),
                                                         ("fan65", ["nSmooth=0", "areaComp=7"], -1, 0), ("same_triple", ["nSmooth=2", "areaComp=-3"], -1, 2)])
def test_smooth_tool_end_to_end(tmp_path, name, args, area_comp, nsmooth):
    """smoothMEF3d.ex writes, byte for byte, the MEF of the restatement, and prints nothing; an areaComp that names no component means
    the triangles' own areas"""
    nodes, e = SC.structure(name)
    _write(tmp_path / "in.mef", nodes, e, title="flame 7")
    out = _run("smoothMEF3d.ex", ["infile=in.mef", "outfile=out.mef", "comp=3"] + args, tmp_path)
    assert out.returncode == 0 and out.stdout == "", out.stderr
    assert open(tmp_path / "out.mef", "rb").read() == R.mef_bytes(ref_structure(name, area_comp, nsmooth)[0], e, "flame 7", _names(5))


def test_smooth_tool_refusals(tmp_path):
    nodes, e = SC.structure("octahedron")
    _write(tmp_path / "in.mef", nodes, e)
    _write(tmp_path / "two.mef", nodes[:, [4, 3]], e, names=["area", "f"])
    with open(tmp_path / "quad.mef", "wb") as fh:
        fh.write(R.mef_bytes(nodes, e, "t", _names(5)).replace(b"\n8 3\n", b"\n6 4\n", 1))
    for args, text in ((["infile=in.mef", "comp=5"], "comp: 5 is not a node variable"), (["infile=in.mef", "comp=-1"], "comp: -1 is not a node variable"),
                       (["infile=in.mef"], "comp not found in table"), (["infile=in.mef", "comp=3", "nSmooth=-1"], "nSmooth must not be negative"),
                       (["infile=quad.mef", "comp=3"], "needs 3 nodes per element"), (["infile=two.mef", "comp=1"], "needs the node coordinates x, y, z"),
                       (["infile=missing.mef", "comp=3"], "Unable to open file")):
        out = _run("smoothMEF3d.ex", args + ["outfile=no.mef"], tmp_path)
        assert out.returncode != 0 and text in out.stderr and not os.path.exists(tmp_path / "no.mef"), (args, out.stderr)
    # a file of two components with its area column named: only its own two columns come back
    out = _run("smoothMEF3d.ex", ["infile=two.mef", "outfile=two_out.mef", "comp=1", "areaComp=0", "nSmooth=2"], tmp_path)
    assert out.returncode == 0 and out.stdout == "", out.stderr
    assert open(tmp_path / "two_out.mef", "rb").read() == R.mef_bytes(R.smooth(nodes[:, [4, 3]], e, 1, 0, 2), e, "0.125", ["area", "f"])


def test_size_case(ctx):
    """about 20 000 elements, several blocks: bit for bit"""
    nodes, e = SC.size_surface()
    want, info = R.smooth(nodes, e, SC.SIZE["comp"], SC.SIZE["area_comp"], SC.SIZE["nsmooth"], detail=True)
    assert len(e) == 20000
    check_smooth(ctx, nodes, e, SC.SIZE["comp"], SC.SIZE["area_comp"], SC.SIZE["nsmooth"], want, info, "100 x 100 grid")
