"""GPU parity of the stream subsetting (streamSub.cpp; pa_streamsub.hip): every pa_ssub_* entry point exactly -- the copied data as uint64 --
and streamSub3d.ex byte for byte, against the CPU restatement tests/streamsub_ref.py over the case matrix of tests/streamsub_cases.py.
The known answers that pin the restatement itself are in test_streamsub_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import streamsample_ref as S
import streamsel_cases as SK
import streamsel_ref as SR
import streamsub_cases as K
import streamsub_ref as R
from peleanalysis_amd import capi
from util import SENT_GPU, sentinel_count

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")
SENT_INT = -1163129375  # 0xBAAC0DE1 as int32: "never stored here"; no id, index or count of the matrix is near it
CHUNK = 2048


def tables(path):
    """the flat tables of pa_ssel_create from a read stream directory: box_desc, node_table, fabs [g] = [ncomp][nj][ni], g of (lev, box)"""
    box, fabs, node, gid, off = [], [], {}, {}, 0
    for l, lev in enumerate(path["levels"]):
        for b, (lo, hi, a) in enumerate(lev):
            ni, nj = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
            gid[(l, b)] = len(box)
            box.append((ni, nj, lo[1], off))
            off += ni * nj
            fabs.append(np.asarray(a))
            for k, v in enumerate(path["ins"][l][b]):
                node[int(v)] = (gid[(l, b)], k)
    return np.array(box, np.int64), np.array([node[n + 1] for n in range(len(node))], np.int32).reshape(-1, 2), fabs, gid


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def no_sentinel(*arrays):
    for a in arrays:
        a = np.asarray(a)
        n = int(np.count_nonzero(a == SENT_INT)) if a.dtype in (np.int32, np.int64) else sentinel_count(a, SENT_GPU)
        assert n == 0, "%d of %d outputs never written" % (n, a.size)


def check_plan(ctx, path, E, comp_idx, scan_path="one_workgroup", elts=None):
    """one plan and its copies against the restatement.  elts: (DevBuf, count) of a selection that stayed on the device"""
    want = R.subset(path, E, comp_idx)
    box, node, fabs, gid = tables(path)
    sel = capi.StreamSel(ctx, box, node, out_fill=SENT_GPU, int_fill=SENT_INT)
    npe, ncomp = path["npe"], len(path["names"])
    plan = capi.StreamSub(sel, path["face"], npe, E) if elts is None else capi.StreamSub(sel, path["face"], npe, elts[0], nElts=path["nElts"], nSel=elts[1])
    kept_g = [gid[k] for k in want["kept"]]
    pts = [int(box[g][0] * box[g][1]) for g in kept_g]
    assert plan.counts() == (len(kept_g), len(want["newNum"]), sum(pts))
    got = plan.read(fill=SENT_INT)
    no_sentinel(got["kept"], got["box_desc"], got["newNum"], got["faceSel"])
    assert got["kept"].tolist() == kept_g and kept_g == sorted(kept_g)
    assert got["box_desc"].tolist() == [[int(box[g][0]), int(box[g][1]), int(box[g][2]), sum(pts[:q])] for q, g in enumerate(kept_g)]
    assert got["newNum"].tolist() == [want["newNum"].get(n + 1, 0) for n in range(len(node))]
    assert got["faceSel"].ravel().tolist() == want["face"]
    chunks = sum((p + CHUNK - 1) // CHUNK for p in pts)
    rec = plan.last_launch()
    assert rec == dict(nElts=path["nElts"], nSel=len(E), boxes=len(box), kept_boxes=len(kept_g), chunks=chunks, path=scan_path, scan_blocks=(len(box) + 255) // 256, gather_blocks=0)
    flat = np.concatenate([np.asarray(a).ravel() for per in want["levels"] for _, _, a in per])  # kept box b' at ncompSel * off'
    whole = capi.Tube.flat(fabs)
    only = capi.Tube.flat([a[comp_idx] for a in fabs])
    for data, nc, comps, group in ((whole, ncomp, comp_idx, None), (only, len(comp_idx), list(range(len(comp_idx))), None), (whole, ncomp, comp_idx, 1)):
        out = plan.gather(data, nc, comps, group=group)
        no_sentinel(out)
        assert np.array_equal(u64(out), u64(flat)), (nc, group)
        assert plan.last_launch()["gather_blocks"] == chunks * (1 if group else len(comps))
    plan.close()
    sel.close()
    return want


# ------------------------------------------------------------------------------------------------ entry points
@pytest.mark.parametrize("case", range(len(K.EDGE_RUNS)))
def test_plan_and_gather_match_restatement(ctx, case):
    files, path = K.edge_dir()
    kw = {k: v for k, v in K.EDGE_RUNS[case].items() if k not in ("comps", "verbose")}
    E = R.element_list(path["nElts"], **kw)[1]
    want = check_plan(ctx, path, E, R.select_comps(path["names"], K.EDGE_RUNS[case].get("comps", ())))
    if case == K.EDGE_ONE_BOX:
        assert want["kept"] == [(1, 1)]
    if case == 1:
        assert len(want["kept"]) == 3


@pytest.mark.parametrize("npe", [1, 4])
def test_other_element_sizes(ctx, npe):
    files, path = K.edge_dir(npe=npe)
    for E in ([0], [1], [45, 3, 3, 1], list(range(46))):
        check_plan(ctx, path, E, list(range(6)))


@pytest.mark.parametrize("nboxes", K.MANY_BOXES)
def test_box_scan_beyond_one_workgroup(ctx, nboxes):
    files, path = K.many_boxes_dir(nboxes)
    want = check_plan(ctx, path, list(range(40)), [0, 1, 2, 3], scan_path="one_workgroup" if nboxes <= 256 else "block_sums")
    assert 60 < len(want["kept"]) <= 120  # kept and dropped boxes in every workgroup, runs of 3 doubles back to back
    check_plan(ctx, path, [39], [3], scan_path="one_workgroup" if nboxes <= 256 else "block_sums")


def seed_select(ctx, path, lo, hi, blocks):
    box, node, fabs, gid = tables(path)
    sel = capi.StreamSel(ctx, box, node, out_fill=SENT_GPU, int_fill=SENT_INT)
    node_map = R.check_tables(path, True)
    want = R.seed_elements(path, node_map, lo, hi)
    whole, xyz = capi.Tube.flat(fabs), capi.Tube.flat([a[0:3] for a in fabs])
    for data, nc in ((whole, len(path["names"])), (xyz, 3)):
        (buf, n), launch = capi.StreamSub.select_seedbox(sel, data, nc, path["face"], path["npe"], lo, hi, on_device=True)
        got = buf.to_numpy(np.int32, (max(2, path["nElts"]),))
        assert n == len(want) and got[:n].tolist() == want
        assert np.all(got[n:] == SENT_INT)  # nothing stored past the count
        assert launch == dict(elements=path["nElts"], blocks=blocks, scan_passes=1, kept=len(want))
    sel.close()
    return want, (buf, n)


@pytest.mark.parametrize("case", range(len(K.SEED_RUNS)))
def test_seed_boxes_match_restatement(ctx, case):
    files, path = K.seed_dir()
    kw = K.SEED_RUNS[case]
    want, _ = seed_select(ctx, path, kw["seedLo"], kw["seedHi"], blocks=1)
    if case == 0:
        assert 0 in want and 4 in want and not {1, 2, 3, 5, 6} & set(want)
    if case == 1:
        assert want == [6]
    if case == 2:
        assert len(want) >= path["nElts"] - 3 and 3 not in want


def test_seed_box_that_keeps_everything(ctx):
    files, path = K.edge_dir()  # no NaN among its seed points
    want, _ = seed_select(ctx, path, K.SEED_ALL["seedLo"], K.SEED_ALL["seedHi"], blocks=1)
    assert want == list(range(path["nElts"]))


@pytest.mark.parametrize("nelts", K.BIG_ELTS)
def test_element_compaction_beyond_one_workgroup(ctx, nelts):
    files, path = K.big_dir(nelts)
    want, elts = seed_select(ctx, path, K.BIG_SEED["seedLo"], K.BIG_SEED["seedHi"], blocks=(nelts + 255) // 256)
    assert nelts // 8 < len(want) < nelts - nelts // 8  # kept and dropped elements in every workgroup
    # the selection stays on the device: a fresh handle, the same list
    box, node, fabs, gid = tables(path)
    sel = capi.StreamSel(ctx, box, node, int_fill=SENT_INT)
    (buf, n), _ = capi.StreamSub.select_seedbox(sel, capi.Tube.flat(fabs), 5, path["face"], 3, K.BIG_SEED["seedLo"], K.BIG_SEED["seedHi"], on_device=True)
    sub = check_plan(ctx, path, want, [0, 1, 2, 3, 4], elts=(buf, n))
    assert sub["kept"] == [(0, 0), (0, 1)]  # runs of 2103 doubles (two chunks, the second of 55) and 987: odd, so the next run is 8 bytes off
    sel.close()


def test_refusals_leave_handle_and_plan_as_they_were(ctx):
    files, path = K.edge_dir()
    box, node, fabs, gid = tables(path)
    sel = capi.StreamSel(ctx, box, node, out_fill=SENT_GPU, int_fill=SENT_INT)
    face, data = path["face"], capi.Tube.flat(fabs)
    plan = capi.StreamSub(sel, face, 3, [1, 0])
    before, out_before = plan.read(), plan.gather(data, 6, [0, 5])
    for elts, msg in (([0, 46], "an element id lies outside 0 .. 45"), ([-1], "an element id lies outside 0 .. 45"), ([], "no element is selected")):
        with pytest.raises(capi.PaError, match=msg):
            capi.StreamSub(sel, face, 3, np.array(elts, np.int32))
    bad = np.array(face, np.int32)
    bad[4] = 194
    with pytest.raises(capi.PaError, match="names a node id outside 1 .. 193"):
        capi.StreamSub(sel, bad, 3, [1])
    bad[4] = 0
    with pytest.raises(capi.PaError, match="names a node id outside 1 .. 193"):
        capi.StreamSub.select_seedbox(sel, data, 6, bad, 3, (0, 0, 0), (1, 1, 1))
    dbad, ddat, delts, n = capi._dev(ctx, bad), capi._dev(ctx, data), sel._i32(46), capi.C.c_int64(-7)  # the refused call stored no element index
    assert ctx.lib.pa_ssub_select_seedbox(ctx.h, sel.h, ddat.ptr, 6, 46, 3, dbad.ptr, capi._d3((-9, -9, -9)), capi._d3((9, 9, 9)), delts.ptr, capi.C.byref(n), None) != 0
    assert np.all(delts.to_numpy(np.int32, (46,)) == SENT_INT) and n.value == 0
    assert capi.StreamSub(sel, bad, 3, [0]).counts()[0] == 1  # element 0 does not read the bad id
    with pytest.raises(capi.PaError, match="needs components 0, 1 and 2"):
        capi.StreamSub.select_seedbox(sel, data, 2, face, 3, (0, 0, 0), (1, 1, 1))
    ddata, dout = capi._dev(ctx, data), sel._f64(65 * plan.counts()[2])
    for comps, nc, msg in (([0, 6], 6, "component 6 out of range"), ([-1], 6, "component -1 out of range"), (list(range(65)), 65, "more than 64 components")):
        with pytest.raises(capi.PaError, match=msg):
            c = np.array(comps, np.int32)
            ctx.check(ctx.lib.pa_ssub_gather(ctx.h, plan.h, ddata.ptr, nc, len(c), c.ctypes.data_as(capi.C.POINTER(capi.C.c_int32)), dout.ptr, len(c), 0))
    with pytest.raises(capi.PaError, match="components outside the output buffer"):
        c = np.array([0, 1], np.int32)
        ctx.check(ctx.lib.pa_ssub_gather(ctx.h, plan.h, ddata.ptr, 6, 2, c.ctypes.data_as(capi.C.POINTER(capi.C.c_int32)), dout.ptr, 2, 1))
    assert sentinel_count(dout.to_numpy(np.float64, (65 * plan.counts()[2],)), SENT_GPU) == 65 * plan.counts()[2]  # no refused call stored anything
    after = plan.read()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    assert np.array_equal(u64(plan.gather(data, 6, [0, 5])), u64(out_before))
    gj, gh = sel.peaks(data, 6, 4)  # the handle still serves its other calls
    assert gj.tolist() == SR.peaks(path, 4)[0]
    plan.close()
    sel.close()
    # a box with lines but no seed point; tables whose ids do not sit on the first lines of their box
    p2 = S.read_stream_dir(K.no_seed_dir())
    box2, node2, fabs2, _ = tables(p2)
    sel2 = capi.StreamSel(ctx, box2, node2)
    with pytest.raises(capi.PaError, match=r"Str box 2 \(j = 1 .. 8\) has lines but no seed point j = 0"):
        capi.StreamSub.select_seedbox(sel2, capi.Tube.flat(fabs2), 6, p2["face"], 1, (0, 0, 0), (1, 1, 1))
    assert capi.StreamSub(sel2, p2["face"], 1, [2]).counts()[0] == 1
    sel2.close()
    holes = node.copy()
    holes[int(path["ins"][0][0][0]) - 1] = (0, 64)
    sel3 = capi.StreamSel(ctx, box, holes)
    with pytest.raises(capi.PaError, match="two node ids on line 64 of box 0"):
        capi.StreamSub(sel3, face, 3, [0])
    sel3.close()


# ------------------------------------------------------------------------------------------------ the tool
def write_dir(d, files):
    for rel, data in files.items():
        os.makedirs(os.path.dirname(os.path.join(d, rel)), exist_ok=True)
        with open(os.path.join(d, rel), "wb") as f:
            f.write(data)


def read_dir(d):
    out = {}
    for root, _, names in os.walk(d):
        for n in names:
            p = os.path.join(root, n)
            with open(p, "rb") as f:
                out[os.path.relpath(p, d)] = f.read()
    return out


def tool(exe, args, cwd):
    return subprocess.run([os.path.join(BIN, exe)] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def key_args(kw):
    out = []
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            if len(v):
                out.append(k + "=" + " ".join(repr(x) if isinstance(x, float) else str(x) for x in v))
        else:
            out.append("%s=%s" % (k, v))
    return out


TOOL_DIRS = {"edge": lambda: K.edge_dir()[0], "edge1": lambda: K.edge_dir(npe=1)[0], "edge4": lambda: K.edge_dir(npe=4)[0], "seed": lambda: K.seed_dir()[0],
             "big": lambda: K.big_dir(2100)[0], "boxes": lambda: K.many_boxes_dir(1100)[0], "noseed": K.no_seed_dir, "hand.v1.str": lambda: K.hand_dir()[1],
             "badid": lambda: SK.small_dir(ids=(3, 1, 4))[1], "noentry": lambda: SK.small_dir(ids=(1, 2, 2))[1]}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    d = tmp_path_factory.mktemp("streamsub")
    files = {}
    for name, make in TOOL_DIRS.items():
        files[name] = make()
        write_dir(str(d / name), files[name])
    return d, files


TOOL_RUNS = [("edge", kw, []) for kw in K.EDGE_RUNS] + [("edge", K.EDGE_RUNS[9], ["nCompsPerPass=1"]), ("edge", K.EDGE_RUNS[7], ["nCompsPerPass=2"])] + \
            [("edge1", dict(eltIDs=[1, 0, 45]), []), ("edge4", dict(sElt=40, nElt=6, comps=["T", "Y"]), [])] + [("seed", kw, []) for kw in K.SEED_RUNS] + [("edge", K.SEED_ALL, [])] + \
            [("big", K.BIG_SEED, []), ("boxes", dict(sElt=0, nElt=40), []), ("boxes", dict(eltIDs=[39], comps=["T"]), []), ("noseed", dict(eltIDs=[2, 0]), []),
             ("hand.v1.str", dict(), []), ("hand.v1.str", dict(eltIDs=[1], verbose=1), [])]


@pytest.mark.parametrize("n", range(len(TOOL_RUNS)))
def test_streamsub_tool(dirs, n):
    d, files = dirs
    name, kw, extra = TOOL_RUNS[n]
    named = name != "hand.v1.str"  # the default name: hand.v1.str -> hand.v1_new
    want = R.run(files[name], infile=name, **kw)
    out = "out%d" % n if named else want["outfile"]
    if not named:
        assert out == "hand.v1_new"
        if (d / out).exists():
            os.rename(str(d / out), str(d / (out + ".seen%d" % n)))
    r = tool("streamSub3d.ex", ["infile=" + name] + (["outfile=" + out] if named else []) + key_args(kw) + extra, d)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout.splitlines() == want["stdout"].splitlines() and r.stderr.splitlines() == want["stderr"].splitlines()
    got = read_dir(str(d / out))
    assert sorted(got) == sorted(want["files"])
    for rel in sorted(want["files"]):
        assert got[rel] == want["files"][rel], rel


def test_tool_moves_an_existing_output_away(dirs):
    d, files = dirs
    want = R.run(files["edge"], eltIDs=[1])["files"]
    assert tool("streamSub3d.ex", ["infile=edge", "outfile=again", "sElt=0", "nElt=46"], d).returncode == 0
    first = read_dir(str(d / "again"))
    assert tool("streamSub3d.ex", ["infile=edge", "outfile=again", "eltIDs=1"], d).returncode == 0
    assert read_dir(str(d / "again")) == want
    old = [p for p in os.listdir(str(d)) if p.startswith("again.old.")]
    assert len(old) == 1 and read_dir(str(d / old[0])) == first


def test_tool_aborts_with_a_message_and_writes_nothing(dirs):
    d, files = dirs
    cases = [("edge", ["eltIDs=46"], "element id 46 outside 0 .. 45"), ("edge", ["eltIDs=3 -1"], "element id -1 outside 0 .. 45"), ("edge", ["sElt=44", "nElt=3"], "element id 46 outside 0 .. 45"),
             ("edge", ["nElt=0"], "nElt = 0: no element is selected"), ("edge", ["comps=W"], "Component not found: W"), ("edge", ["comps=X X"], "Component given twice: X"),
             ("edge", ["seedLo=0 0 0"], "seedLo and seedHi must come together"), ("edge", ["seedLo=0 0 0", "seedHi=1 1 1", "nElt=1"], "seedLo / seedHi exclude eltIDs, sElt and nElt"),
             ("edge", ["seedLo=0 0", "seedHi=1 1 1"], "seedLo and seedHi take three values each"), ("edge", ["ngpus=2"], "ngpus"),
             ("seed", key_args(K.SEED_NONE), "no element has all its seed points inside seedLo .. seedHi"),
             ("noseed", key_args(K.SEED_RUNS[0]), "Str box 2 of level 0 (j = 1 .. 8) has lines but no seed point j = 0"),
             ("badid", [], "inside_nodes id 4 outside 1 .. 3"), ("noentry", [], "node 3 has no inside_nodes entry"), ("nothere", [], "Unable to open nothere/Header")]
    for name, args, msg in cases:
        r = tool("streamSub3d.ex", ["infile=" + name, "outfile=no_out"] + args, d)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
        assert "amrex::Abort" in r.stderr and r.stdout == ""  # a message of the tool, not a fault
        assert not (d / "no_out").exists()


def test_tube_statistics_take_a_subset_with_a_placeholder_level(dirs):
    """triangles whose nodes all lie on level 1: level 0 is written as the placeholder box; streamTubeStats3d integrates over the subset and gives
    what its restatement gives for the restated directory"""
    import tubestats_ref as T
    d, files = dirs
    path = S.read_stream_dir(files["boxes"])
    level_of = {int(ids[0]): l for l, per in enumerate(path["ins"]) for ids in per}
    E = [e for e in range(40) if all(level_of[int(v)] == 1 for v in path["face"][3 * e:3 * e + 3])]
    assert 5 < len(E) < 35
    sub = R.run(files["boxes"], eltIDs=E)
    assert sub["files"]["Level_0/Str_D_00000"] == R.placeholder_bytes(4) and len(sub["sub"]["kept"]) > 10
    assert tool("streamSub3d.ex", ["infile=boxes", "outfile=tube.sub"] + key_args(dict(eltIDs=E)), d).returncode == 0
    want = T.run_tool(sub["files"], "tube.sub", intComps=[3])
    r = tool("streamTubeStats3d.ex", ["infile=tube.sub", "intComps=3"], d)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout == want["stdout"] and (d / (T.out_root("tube.sub") + "_volInt.mef")).read_bytes() == want["mef"]


def test_round_trip_through_the_stream_tools(dirs):
    d, files = dirs
    # all elements: every box with lines is kept, renumbered; streamScatter prints the rows the restatement predicts for that directory
    want = R.run(files["edge"], **K.EDGE_RUNS[K.EDGE_ALL])["files"]
    assert tool("streamSub3d.ex", ["infile=edge", "outfile=rt_all"] + key_args(K.EDGE_RUNS[K.EDGE_ALL]), d).returncode == 0
    for kw in SK.SCATTER_RUNS[:3]:
        rows = SR.run_scatter(want, **kw)
        r = tool("streamScatter3d.ex", ["infile=rt_all"] + key_args(kw), d)
        assert r.returncode == 0 and r.stdout == rows and len(rows) > 0, r.stderr
    # one box of level 1: level 0 is written as the placeholder box, and the downstream tools take the directory
    one = R.run(files["edge"], **K.EDGE_RUNS[K.EDGE_ONE_BOX])["files"]
    assert one["Level_0/Str_D_00000"] == R.placeholder_bytes(6)
    assert tool("streamSub3d.ex", ["infile=edge", "outfile=rt_one"] + key_args(K.EDGE_RUNS[K.EDGE_ONE_BOX]), d).returncode == 0
    kw = dict(vars=["X", "H2"], condComp=4, condValMoreThan=-1.0, condValLessThan=100.0)
    r = tool("streamScatter3d.ex", ["infile=rt_one"] + key_args(kw), d)
    assert r.returncode == 0 and r.stdout == SR.run_scatter(one, **kw) and r.stdout.count("\n") > 40, r.stderr
    kw = dict(nLines=1000, comps=[0, 1, 3])
    p = SR.run_stream2plt(one, **kw)
    r = tool("stream2plt3d.ex", ["infile=rt_one", "outfile=rt_one.dat"] + key_args(kw), d)
    assert r.returncode == 0 and r.stdout == p["stdout"] and (d / "rt_one.dat").read_bytes() == p["dat"], r.stderr
    assert len(p["sel"]) == 64
