"""GPU tier: the decimation kernels (peleanalysis_amd/csrc/pa_decimate.hip) through the C ABI, and decimateMEF3d.ex end to end, against
the restatement tests/decimate_ref.py.  For every case of tests/decimate_cases.py the state after EVERY round -- positions and quadrics
as uint64 bits, faces and flags exactly, the round's record -- equals the restatement's; so do the final surface, pa_decimate_run and
the tool's file.  Output arrays start as the payload NaN of tests/util.py ("writes each output")."""
import functools
import os
import subprocess

import numpy as np
import pytest

import decimate_cases as DC
import decimate_ref as R
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import field_flame, nested_hierarchy
from peleanalysis_amd.plotfile import read_mef, write_plotfile
from util import SENT_GPU, make_states, sentinel_count

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
NAMES = list(DC.CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement of a case, computed once and shared: ([(state, record) after every round], output, message, rounds)"""
    x, e = DC.mesh(name)
    d = R.Decimator(x, e, **DC.options(name))
    trace = [(d.state(), d.record())]
    while d.round(DC.CASES[name][1]):
        trace.append((d.state(), d.record()))
    last = d.record()  # a round that found no candidate leaves its record
    return trace, d.output(), d.message, d.rounds, last


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def assert_state(got, want, what):
    for g, w, part in zip(got, want, ("xyz", "faces", "valid", "quadrics")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, part)
        if g.dtype == np.float64:
            assert sentinel_count(g, SENT_GPU) == 0, (what, part, "never written")
            bad = np.argwhere(u64(g) != u64(w))
            assert len(bad) == 0, (what, part, len(bad), bad[:3].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
        else:
            assert np.array_equal(g, w), (what, part, int(np.sum(g != w)))


def assert_output(got, want, what):
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (what, got[0].shape, want[0].shape, got[1].shape, want[1].shape)
    assert sentinel_count(got[0], SENT_GPU) == 0, what
    assert np.array_equal(u64(got[0]), u64(want[0])), what
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("name", NAMES)
def test_every_round_equals_restatement(ctx, name):
    trace, out, message, rounds, last = reference(name)
    x, e = DC.mesh(name)
    target = DC.CASES[name][1]
    with capi.Decimate(ctx, x, e, **DC.options(name)) as d:
        assert_state(d.read_state(fill=SENT_GPU), trace[0][0], name + " initial")
        n = 0
        while d.round(target):
            n += 1
            assert n < len(trace), (name, "more rounds than the restatement", n)
            assert d.last_round() == trace[n][1], (name, n, d.last_round(), trace[n][1])
            assert_state(d.read_state(fill=SENT_GPU), trace[n][0], "%s round %d" % (name, n))
        assert n == rounds == len(trace) - 1, (name, n, rounds)
        assert d.last_round() == last, (name, d.last_round(), last)
        got = d.read(fill=SENT_GPU)
        assert_output(got, out, name)
        assert d.counts() == (len(out[0]), len(out[1]), rounds)
        again = d.read(fill=SENT_GPU)  # reading does not disturb the surface
        assert_output(again, out, name + " second read")
    if name == "tetrahedron":
        assert rounds == 0 and message == "no valid contraction left at 4 faces" and np.array_equal(got[1], e) and np.array_equal(u64(got[0]), u64(x))


@pytest.mark.parametrize("name", NAMES)
def test_run_equals_rounds_and_repeats(ctx, name):
    """pa_decimate_run == the round-by-round result, and two runs on the same input give the same bytes"""
    _, out, _, rounds, last = reference(name)
    x, e = DC.mesh(name)
    res = []
    for _ in range(2):
        with capi.Decimate(ctx, x, e, **DC.options(name)) as d:
            assert d.run(DC.CASES[name][1]) == rounds
            assert d.last_round() == last
            res.append((d.read(fill=SENT_GPU), d.read_state(fill=SENT_GPU)))
    assert_output(res[0][0], out, name)
    assert res[0][0][0].tobytes() == res[1][0][0].tobytes() and res[0][0][1].tobytes() == res[1][0][1].tobytes()
    for a, b in zip(res[0][1], res[1][1]):
        assert a.tobytes() == b.tobytes()


def test_max_rounds_caps_the_loop(ctx):
    trace = reference("ico320_half")[0]
    x, e = DC.mesh("ico320_half")
    with capi.Decimate(ctx, x, e) as d:
        assert d.run(160, max_rounds=2) == 2
        assert_state(d.read_state(fill=SENT_GPU), trace[2][0], "two rounds")


def test_create_refuses_bad_input(ctx):
    x, e = DC.mesh("octahedron_to_6")
    bad = e.copy()
    bad[3, 1] = 7
    with pytest.raises(capi.PaError, match="element 4 names a node that does not exist"):
        capi.Decimate(ctx, x, bad)
    bad = e.copy()
    bad[2, 2] = bad[2, 0]
    with pytest.raises(capi.PaError, match="element 3 names a node twice"):
        capi.Decimate(ctx, x, bad)
    with pytest.raises(capi.PaError, match="weighting"):
        capi.Decimate(ctx, x, e, weighting=2)
    with pytest.raises(capi.PaError, match="placement"):
        capi.Decimate(ctx, x, e, placement=2)


def _mef(path, x, e, extra=0):
    nodes = np.hstack([x] + [np.full((len(x), 1), 7.0 + c) for c in range(extra)])
    names = ["X", "Y", "Z"] + ["f%d" % c for c in range(extra)]
    with open(path, "wb") as fh:
        fh.write(R.mef_bytes(nodes, e, title="0.125", names=names))
    return nodes


def _tool(args, cwd):
    return subprocess.run([os.path.join(BIN, "decimateMEF3d.ex")] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True)


@pytest.mark.parametrize("name", ["tetrahedron", "ico1280_tenth", "grid8_O1", "cylinder_W0", "cylinder_B0", "fin_locked_edge", "target_ge_nfaces", "ico320_O0"])
def test_tool_end_to_end(tmp_path, name):
    """decimateMEF3d.ex writes, byte for byte, the MEF of the restatement; stderr carries the two count lines (and the stop message)"""
    x, e = DC.mesh(name)
    o = DC.options(name)
    nodes = _mef(tmp_path / "in.mef", x, e, extra=2)  # only the first three components are used
    want, err = R.run_tool(nodes, e, DC.CASES[name][1], **o)
    out = _tool(["-t", DC.CASES[name][1], "-o", "out.mef", "-B", repr(o["boundary_weight"]), "-W", o["weighting"], "-O", o["placement"], "in.mef"], tmp_path)
    assert out.returncode == 0, out.stderr
    assert open(tmp_path / "out.mef", "rb").read() == want
    assert out.stderr.split("\n")[:len(err)] == err
    if name == "tetrahedron":
        assert "no valid contraction left at 4 faces" in err
        quiet = _tool(["-q", "-t", 2, "-o", "q.mef", "in.mef"], tmp_path)
        assert quiet.returncode == 0 and "model" not in quiet.stderr and open(tmp_path / "q.mef", "rb").read() == want


def test_tool_refuses_what_it_does_not_do(tmp_path):
    x, e = DC.mesh("octahedron_to_6")
    _mef(tmp_path / "in.mef", x, e)
    base = ["-t", 6, "-o", "out.mef"]
    for extra, word in ((["-W", 2], "-W 2"), (["-O", 2], "-O 2"), (["-F"], "-F"), (["-r"], "-r"), (["-j"], "-j"), (["-I", "x.smf"], "-I"), (["-m", 2.0], "-m"),
                        (["-c", 0.5], "-c"), (["-T", "smf"], "-T smf"), (["-M", "smf"], "-M smf")):
        out = _tool(base + extra + ["in.mef"], tmp_path)
        assert out.returncode != 0 and ("option " + word + " is not supported") in out.stderr, (extra, out.stderr)
        assert not os.path.exists(tmp_path / "out.mef")
    assert _tool(base + ["-T", "mef", "-M", "mef", "in.mef"], tmp_path).returncode == 0
    with open(tmp_path / "quad.mef", "wb") as fh:  # nodesPerElt = 4
        fh.write(R.mef_bytes(x, e[:6], names=("X", "Y", "Z")).replace(b"\n6 3\n", b"\n4 4\n", 1) + b"\0" * 8)
    out = _tool(base + ["quad.mef"], tmp_path)
    assert out.returncode != 0 and "needs 3 nodes per element" in out.stderr
    bad = e.copy()
    bad[0, 0] = 9
    with open(tmp_path / "bad.mef", "wb") as fh:
        fh.write(R.mef_bytes(x, bad))
    out = _tool(base + ["bad.mef"], tmp_path)
    assert out.returncode != 0 and "names a node that does not exist" in out.stderr


def test_chain_isosurface_decimate_checkiso(tmp_path):
    """isosurface3d.ex on a 32^3 plotfile -> decimateMEF3d.ex to a quarter of the faces -> checkIso3d.ex (also with strict=1, which
    the isosurface itself passes) accepts the result (the bytes are compared with the restatement's in test_tool_end_to_end)"""
    H = nested_hierarchy(32, 1, 16, is_per=(0, 0, 0))
    mfs = make_states(H, 1, 0, field_flame)
    p = str(tmp_path / "plt00005")
    write_plotfile(p, H, mfs, ["temp"], time=0.125, level_steps=[5])
    iso = subprocess.run([os.path.join(BIN, "isosurface3d.ex"), "infile=" + p, "isoCompName=temp", "isoVal=1150"], cwd=tmp_path, capture_output=True, text=True)
    assert iso.returncode == 0, iso.stderr
    f = p + "_temp_1150.mef"
    _, _, nodes, faces = read_mef(f)
    assert len(faces) > 1000
    target = len(faces) // 4
    out = _tool(["-t", target, "-o", "dec.mef", f], tmp_path)
    assert out.returncode == 0, out.stderr
    _, names, dn, df = read_mef(str(tmp_path / "dec.mef"))
    assert names == ["X", "Y", "Z"] and len(df) in (target, target - 1)
    assert out.stderr.split("\n")[:2] == ["+ Initial model    (%dv/%df)" % (len(nodes), len(faces)), "+ Simplified model (%dv/%df)" % (len(dn), len(df))]
    for src in (f, "dec.mef"):
        for extra in ([], ["strict=1"]):
            chk = subprocess.run([os.path.join(BIN, "checkIso3d.ex"), "isoFile=" + src] + extra, cwd=tmp_path, capture_output=True, text=True)
            assert chk.returncode == 0 and "All shared edges are consistently numbered." in chk.stdout, (src, extra, chk.stderr)
