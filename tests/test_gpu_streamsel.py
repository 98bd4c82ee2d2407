"""GPU parity of the stream selection (streamScatter.cpp, stream2plt.cpp; pa_streamsel.hip): every pa_ssel_* entry point bit for bit,
and streamScatter3d.ex / stream2plt3d.ex byte for byte, against the CPU restatement tests/streamsel_ref.py over the case matrix of
tests/streamsel_cases.py.  The known answers that pin the restatement itself are in test_streamsel_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import streamsample_ref as S
import streamsel_cases as K
import streamsel_ref as R
from peleanalysis_amd import capi
from util import SENT_GPU, sentinel_count

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")


SENT_INT = -1163129375  # 0xBAAC0DE1 as int32: "the kernel never stored here", for jpeak and write_lines (no j and no flag is near it)


def sentinel_sel(ctx, box, node=()):
    """every output of every call starts as a sentinel (SENT_GPU in the doubles, SENT_INT in the ints), freshly uploaded before the
    call: a row, a column or a line a kernel skips cannot compare equal through what an earlier call left in the allocation"""
    return capi.StreamSel(ctx, box, node, out_fill=SENT_GPU, int_fill=SENT_INT)


def no_sentinel(*arrays):
    for a in arrays:
        a = np.asarray(a)
        n = int(np.count_nonzero(a == SENT_INT)) if a.dtype == np.int32 else sentinel_count(a, SENT_GPU)
        assert n == 0, "%d of %d outputs never written by the kernel" % (n, a.size)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


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


def big_dir(seed=3):
    """more than one workgroup of lines: boxes of 700 and 330 lines, 3 points; `a` holds small integers (ties, many kept and dropped)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(1030) + 1
    fabs, per, at = [], [], 0
    for n in (700, 330):
        a = rng.normal(size=(5, 3, n))
        a[3] = rng.integers(-2, 4, size=(3, n))
        fabs.append(((0, -1, 0), (n - 1, 1, 0), a))
        per.append(perm[at:at + n])
        at += n
    return R.write_files(K.PLT_NAMES, [fabs], [per])


@pytest.fixture(scope="module")
def scatter_case():
    names, files, levels, ins = K.scatter_dir()
    return files, S.read_stream_dir(files)


@pytest.fixture(scope="module")
def plt_case():
    names, files, levels, ins = K.plt_dir()
    return files, S.read_stream_dir(files)


# ------------------------------------------------------------------------------------------------ entry points
@pytest.mark.parametrize("which", ["edge", "big"])
def test_peaks_and_scatter_match_restatement(ctx, scatter_case, which):
    path = scatter_case[1] if which == "edge" else S.read_stream_dir(big_dir())
    box, node, fabs, _ = tables(path)
    ncomp = len(path["names"])
    sel = sentinel_sel(ctx, box, node)
    data = capi.DevBuf.from_numpy(ctx, capi.Tube.flat(fabs))
    runs = [(4, [4, 0, 2, 3], K.MORE, K.LESS), (5, [2, 1], -1.0, float("inf")), (4, [4], 0.0, 0.5), (4, [0], 100.0, 200.0), (4, [], K.MORE, K.LESS)] if which == "edge" else \
        [(3, [0, 3, 4], 0.0, 2.0), (3, [1], -10.0, 10.0), (3, [2, 2], 3.0, 3.5)]
    for cond, comps, more, less in runs:
        wj, wh = R.peaks(path, cond)
        gj, gh = sel.peaks(data, ncomp, cond)
        no_sentinel(gj, gh)
        assert np.array_equal(gj, np.array(wj, np.int32)) and np.array_equal(bits(gh), bits(wh))
        rows = R.scatter_rows(path, comps, cond, more, less)
        want = np.array(rows, np.float64).reshape(len(rows), len(comps))
        for group in (None, 1, 3):
            got = sel.scatter(data, ncomp, comps, gj, gh, more, less, group=group)
            no_sentinel(got)
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (cond, comps, group)
    if which == "big":
        assert 256 < len(R.scatter_rows(path, [0], 3, 0.0, 2.0)) < 1030 - 256  # kept and dropped nodes in every workgroup
    sel.close()


def test_scatter_refuses_bad_tables_and_components(ctx, scatter_case):
    path = scatter_case[1]
    box, node, fabs, _ = tables(path)
    sel = capi.StreamSel(ctx, box, node)
    data = capi.Tube.flat(fabs)
    with pytest.raises(capi.PaError, match="out of range"):
        sel.peaks(data, 6, 6)
    gj, gh = sel.peaks(data, 6, 4)
    with pytest.raises(capi.PaError, match="out of range"):
        sel.scatter(data, 6, [0, 6], gj, gh, 0.0, 1.0)
    with pytest.raises(capi.PaError, match="outside its line"):  # a j no line holds: refused by the kernel's own check, nothing read there
        sel.scatter(data, 6, [0], np.full(len(gj), 99, np.int32), gh, -1.0, 100.0)
    sel.close()
    bad = node.copy()
    bad[5] = (-1, 0)
    with pytest.raises(capi.PaError, match="node id 6 is listed by no box"):
        capi.StreamSel(ctx, box, bad)
    bad[5] = (1, 1)  # the zero box has one line
    with pytest.raises(capi.PaError, match="outside its box"):
        capi.StreamSel(ctx, box, bad)
    bad[5] = (5, 0)
    with pytest.raises(capi.PaError, match="box 5 out of range"):
        capi.StreamSel(ctx, box, bad)


def conds_of(kw):
    """the condition table of one run, in the reference's order"""
    out = [(capi.SSEL_MAX, c, 0, s, v, 0.0) for c, s, v in zip(kw.get("maxComps", ()), kw.get("maxSgns", ()), kw.get("maxVals", ()))]
    out += [(capi.SSEL_MIN, c, 0, s, v, 0.0) for c, s, v in zip(kw.get("minComps", ()), kw.get("minSgns", ()), kw.get("minVals", ()))]
    if kw.get("RXY", -1.0) > 0:
        out.append((capi.SSEL_RXY, 0, 0, kw.get("RXYsgn", ""), kw["RXY"], 0.0))
    out += [(capi.SSEL_AT, ac, int(ca), s, va, av) for ac, ca, s, va, av in zip(kw.get("atComps", ()), kw.get("compAt", ()), kw.get("atSgns", ()), kw.get("valAt", ()),
                                                                              kw.get("atVal", ()))]
    return out


def check_kernels(ctx, files, path, kw):
    want = R.run_stream2plt(files, **kw)
    box, node, fabs, gid = tables(path)
    sel = sentinel_sel(ctx, box)
    comps = kw["comps"] if "comps" in kw else [kw.get("sComp", 0) + i for i in range(kw.get("nComp", len(path["names"])))]
    pairs = [(gid[(l, b)], i) for l, b, i in want["sel"]]
    slo, shi, extra = want["slo"], want["shi"], int(kw.get("distComp", -1) >= 0)
    final = sel.gather_lines(capi.Tube.flat(fabs), len(path["names"]), comps, pairs, slo, shi, extra=extra, on_device=True)
    shape = (len(comps) + extra, shi - slo + 1, len(pairs))
    if not kw.get("no_filter"):
        w = sel.filter(final, len(comps), slo, shi, len(pairs), conds_of(kw))
        no_sentinel(w)
        assert list(w) == want["write_lines"]
        if extra:
            sel.arclength(final, len(comps), shi - slo + 1, len(pairs), kw["distComp"], kw["distVal"])
    got = final.to_numpy(np.float64, shape)
    no_sentinel(got)
    assert np.array_equal(np.isnan(got), np.isnan(want["fab"]))
    assert np.array_equal(bits(got), bits(want["fab"]))  # the NaNs of the fixture are copies of one positive quiet NaN
    sel.close()
    return want


@pytest.mark.parametrize("case", range(len(K.PLT_RUNS)))
def test_lines_filters_and_arc_length_match_restatement(ctx, plt_case, case):
    kw = {k: v for k, v in K.PLT_RUNS[case].items() if k not in ("verbose", "finestLevel")}
    want = check_kernels(ctx, plt_case[0], plt_case[1], kw)
    if case == 0:
        assert want["write_lines"] == [1] * 193
    if case == 6:
        assert want["write_lines"] == [0] * 193
    if case == 12:  # crossings and lines without one
        d = want["fab"][5]
        assert (d[0] < 0).any() and (d[0] == d[-1]).any()


def test_more_than_one_workgroup_of_lines(ctx):
    files = big_dir()
    path = S.read_stream_dir(files)
    kw = dict(nLines=5000, maxComps=[4], maxVals=[0.5], maxSgns=["gt"], minComps=[3], minVals=[-2.0], minSgns=["eq"], RXY=1.0, RXYsgn="lt", atComps=[3], compAt=[4.0],
              valAt=[0.0], atVal=[0.5], atSgns=["ge"], distComp=3, distVal=0.5)
    want = check_kernels(ctx, files, path, kw)
    assert len(want["sel"]) == 1030 and 100 < sum(want["write_lines"]) < 930


def test_lines_refuse_a_box_with_another_range(ctx, scatter_case):
    path = scatter_case[1]
    box, node, fabs, gid = tables(path)
    sel = capi.StreamSel(ctx, box)
    data = capi.Tube.flat(fabs)
    with pytest.raises(capi.PaError, match=r"Str box 2 \(j = -4 .. 3\) does not span the directory's j = -3 .. 3"):
        sel.gather_lines(data, 6, [0], [(0, 0), (2, 0)], -3, 3)
    for args, msg in ((([6], [(0, 0)]), "component 6 out of range"), (([0], [(5, 0)]), "box 5 out of range"), (([0], [(0, 65)]), "outside its box")):
        with pytest.raises(capi.PaError, match=msg):
            sel.gather_lines(data, 6, args[0], args[1], -3, 3)
    final = np.zeros((3, 7, 2))
    for conds, msg in (([(capi.SSEL_MAX, 3, 0, "lt", 0.0, 0.0)], "component out of range"), ([(capi.SSEL_AT, 0, 3, "lt", 0.0, 0.0)], "component out of range"),
                       ([(capi.SSEL_MIN, 0, 0, "lt", 0.0, 0.0), (capi.SSEL_MAX, 0, 0, "lt", 0.0, 0.0)], "out of order"), ([(7, 0, 0, "lt", 0.0, 0.0)], "unknown kind")):
        with pytest.raises(capi.PaError, match=msg):
            sel.filter(final, 3, -3, 3, 2, conds)
    with pytest.raises(capi.PaError, match="distComp 3 out of range"):
        sel.arclength(np.zeros((4, 7, 2)), 3, 7, 2, 3, 0.0)
    with pytest.raises(capi.PaError, match="components 0, 1 and 2"):
        sel.arclength(np.zeros((3, 7, 2)), 2, 7, 2, 0, 0.0)
    sel.close()


# ------------------------------------------------------------------------------------------------ the tools
def write_dir(d, files):
    for rel, data in files.items():
        os.makedirs(os.path.dirname(os.path.join(d, rel)), exist_ok=True)
        with open(os.path.join(d, rel), "wb") as f:
            f.write(data)


def tool(exe, args, cwd):
    return subprocess.run([os.path.join(BIN, exe)] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def key_args(kw):
    out = []
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            if len(v):
                out.append(k + "=" + " ".join(str(x) for x in v))
        else:
            out.append("%s=%s" % (k, v))
    return out


@pytest.fixture(scope="module")
def dirs(tmp_path_factory, scatter_case, plt_case):
    d = tmp_path_factory.mktemp("streamsel")
    write_dir(str(d / "scat"), scatter_case[0])
    write_dir(str(d / "plt"), plt_case[0])
    write_dir(str(d / "badid"), K.small_dir(ids=(3, 1, 4))[1])
    write_dir(str(d / "noentry"), K.small_dir(ids=(1, 2, 2))[1])
    return d


@pytest.mark.parametrize("case,extra", [(0, []), (0, ["nVarsPerPass=1"]), (1, ["verbose=1"]), (2, []), (3, [])])
def test_streamscatter_tool(dirs, scatter_case, case, extra):
    kw = K.SCATTER_RUNS[case]
    want = R.run_scatter(scatter_case[0], **kw)
    r = tool("streamScatter3d.ex", ["infile=scat"] + key_args(kw) + extra, dirs)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout == want
    if case == 3:
        assert r.stdout == ""
    if case == 2:
        assert "-0 \n" in r.stdout


# the driver's own code -- key parsing, the repack of the selected components, the sign and compAt decoding, the writer -- runs only here:
# comps / sComp + nComp / no_filter (1, 14, 15, 19), every sign string between them (gt le, ge gt lt, ne eq and an unknown one in 19), a
# fractional compAt whose rounding would name a component that is not there (9), the arc length with and without a crossing, the partial
# selection, the cap.  The other cases of the matrix differ from these in values only and run through capi above.
PLT_TOOL_CASES = [1, 3, 7, 9, 11, 12, 13, 14, 15, 16, 17, 18, 19]


@pytest.mark.parametrize("case", PLT_TOOL_CASES)
def test_stream2plt_tool(dirs, plt_case, case):
    kw = K.PLT_RUNS[case]
    want = R.run_stream2plt(plt_case[0], **kw)
    out = dirs / ("out%d.dat" % case)
    r = tool("stream2plt3d.ex", ["infile=plt", "outfile=" + out.name] + key_args(kw), dirs)
    assert r.returncode == 0, r.stderr + r.stdout
    assert r.stdout == want["stdout"]
    assert out.read_bytes() == want["dat"]
    if case == 17:
        assert 30 < len(want["sel"]) < 90  # rval < 1
    if case == 18:
        assert len(want["sel"]) == 193


def test_tools_abort_with_a_message(dirs):
    s2p, sc = "stream2plt3d.ex", "streamScatter3d.ex"
    cases = [(sc, ["infile=scat", "vars=W", "condComp=4"], "Variable not found: W"),
             (sc, ["infile=scat", "vars=X", "condVar=W"], "Conditioning variable not found: W"),
             (sc, ["infile=scat", "vars=X"], "no conditioning component"),
             (sc, ["infile=scat", "condComp=4"], "ParmParse::getarr(): vars not found in table"),
             (sc, ["infile=scat", "vars=X", "condComp=6"], "out of range"),
             (sc, ["infile=scat", "vars=X", "condComp=4", "ngpus=2"], "ngpus"),
             (sc, ["infile=badid", "vars=X", "condComp=4"], "inside_nodes id 4 outside 1 .. 3"),
             (sc, ["infile=noentry", "vars=X", "condComp=4"], "node 3 has no inside_nodes entry"),
             (s2p, ["infile=plt", "outfile=no.dat"], "nLines = 0"),
             (s2p, ["infile=plt", "outfile=no.dat", "nLines=10", "finestLevel=0"], "finestLevel = 0 is below the file's 1"),
             (s2p, ["infile=plt", "outfile=no.dat", "nLines=10", "distComp=3", "distVal=0", "no_filter=1"], "distComp with no_filter"),
             (s2p, ["infile=plt", "outfile=no.dat", "nLines=10", "atComps=3", "compAt=4", "valAt=1", "atVal=1 2", "atSgns=lt"], "atVal has 2 values, atComps has 1"),
             (s2p, ["infile=plt", "outfile=no.dat", "nLines=10", "comps=0 5"], "component 5 out of range"),
             (s2p, ["infile=plt", "outfile=no.dat", "nLines=10", "ngpus=2"], "ngpus"),
             (s2p, ["infile=scat", "outfile=no.dat", "nLines=1000"], "does not span the directory's j = -3 .. 3")]
    for exe, args, msg in cases:
        r = tool(exe, args, dirs)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
        assert "amrex::Abort" in r.stderr  # a message of the tool, not a fault
        assert not (dirs / "no.dat").exists()
        if exe == sc:
            assert r.stdout == ""
