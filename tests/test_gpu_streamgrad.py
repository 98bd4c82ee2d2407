"""GPU parity of the gradient streamlines (stream.cpp / stream_nd.f90, pa_streamgrad.hip): pa_vtrace_fab against the
reference's own vtrace (golden/stream_vtrace_ref.npz, see test_streamgrad_ref.py), and the hierarchy preparation + trace
and the stream3d tool against the CPU restatement tests/streamgrad_ref.py, bit for bit / byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import streamgrad_ref as R
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, chop_box, field_flame, fill_analytic, nested_hierarchy, union_hierarchy
from peleanalysis_amd.plotfile import read_mef, write_plotfile
from stream_cases import ratio4_hierarchy as _ratio4_hierarchy
from test_streamgrad_ref import CASES, golden_case

pytestmark = pytest.mark.gpu

BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")


@pytest.mark.parametrize("name", CASES)
def test_vtrace_fab_reproduces_reference(ctx, name):
    c = golden_case(name)
    vc = int(c["vcomp"])
    strm, g, err = capi.vtrace_fab(ctx, c["T"], c["T_lo"], c["loc"], c["ids"], int(c["nRKsteps"]), c["dx"], c["plo"], c["phi"], float(c["hRK"]),
                                   vcomp=None if vc < 0 else vc)
    assert err == int(c["errFlag"])
    assert np.array_equal(strm.view(np.int64), c["strm"].view(np.int64))
    if vc < 0:  # the materialised gradient of stream_nd.f90:33-44
        T = c["T"][0]
        assert np.array_equal(g[0], T[1:-1, 1:-1, 2:] - T[1:-1, 1:-1, :-2])


def _hier(kind, per):
    if kind == "nested":
        return nested_hierarchy(16, 3, 8, is_per=per)
    if kind == "union":
        return union_hierarchy(11, nlev=3, n0=(16, 20, 16), is_per=per)
    return _ratio4_hierarchy(per)


def _raw(H, ng, ncomp):
    """the file's data in the valid cells; NaN in every ghost cell (the preparation must overwrite all of them)"""
    out = []
    for lv in H.levels:
        m = MultiFab(lv, ncomp, ng, fill=np.nan)
        fill_analytic(m, 0, lambda x, y, z: np.tanh((np.sqrt((x - 0.5) ** 2 + (y - 0.45) ** 2 + (z - 0.55) ** 2) - 0.2) / 0.06))
        for c in range(1, ncomp):
            fill_analytic(m, c, lambda x, y, z, c=c: np.sin((3 + c) * x + c * y) * np.cos(2 * z) + 0.3 * c * (x - 0.5))
        out.append(m)
    return out


def _seeds(H, rng, n=300):
    """random nodes, nodes on coarse-fine faces (the coarsened fine boxes' faces) and next to the domain walls"""
    pts = [rng.random((3, n))]
    for l in range(1, H.nlev):
        lv = H.levels[l]
        dx = R.level_dx(lv)
        for b in lv.boxes[:6]:
            for d in range(3):
                for face in (b[d], b[3 + d] + 1):
                    p = (b[:3] + rng.random((4, 3)) * (b[3:] - b[:3] + 1)) * dx
                    p[:, d] = face * dx[d]
                    pts.append(p.T)
    w = rng.random((3, 12))
    w[np.arange(12) % 3, np.arange(12)] = np.where(np.arange(12) % 2, 0.9995, 0.0004)
    pts.append(w)
    return np.concatenate(pts, axis=1)


def _device_run(ctx, H, raw, nodes, ins, nRKsteps, hRK, vcomp):
    dls = [capi.DevLevel(ctx, lv) for lv in H.levels]
    dms = [capi.DevMF.from_host(ctx, dl, m) for dl, m in zip(dls, raw)]
    capi.streamgrad_prepare(ctx, dms)
    states = [d.download() for d in dms]
    lines, flags = capi.streamgrad_trace(ctx, dms, nodes, ins, nRKsteps, hRK, vcomp)
    for d in dms:
        d.close()
    for dl in dls:
        dl.close()
    return states, lines, flags


def _check(want, states, lines, flags):
    for l, (a, b) in enumerate(zip(want["states"], states)):
        for q in range(a.level.nboxes):  # every cell of every FAB, ghost cells included (not the padding between components)
            fa, fb = np.ascontiguousarray(a.fab(q)), np.ascontiguousarray(b.fab(q))
            assert np.array_equal(fa.view(np.int64), fb.view(np.int64)), f"prepared state differs on level {l} box {q}"
    n = 0
    for l, (pw, pg) in enumerate(zip(want["lines"], lines)):
        for b, (x, y) in enumerate(zip(pw, pg)):
            assert (x is None) == (y is None)
            if x is not None:
                assert np.array_equal(x.view(np.int64), y.view(np.int64)), f"lines of level {l} box {b} differ"
                n += x.shape[2]
    assert flags == want["flags"]
    return n


@pytest.mark.parametrize("kind,ng,nRKsteps,hrk,vcomp,ncomp", [
    ("nested", 4, 51, 0.1, None, 1),
    ("nested", 2, 30, 0.6, None, 3),
    ("union", 6, 41, 1.5, None, 2),
    ("union", 4, 21, 0.8, 1, 4),
    ("ratio4", 4, 25, 0.5, None, 3),
    ("ratio4", 6, 26, 1.2, 1, 5),
    ("nested", 2, 16, 0.7, 1, 4),
])
def test_hierarchy_matches_restatement(ctx, kind, ng, nRKsteps, hrk, vcomp, ncomp):
    H = _hier(kind, (0, 0, 0))
    raw = _raw(H, ng, ncomp)
    nodes = _seeds(H, np.random.default_rng(ng * 100 + nRKsteps))
    want = R.run_tool(H.levels, raw, nodes, ["X", "Y", "Z"], np.array([1]), 1, nRKsteps=nRKsteps, hRK=hrk, vcomp=vcomp)
    states, lines, flags = _device_run(ctx, H, raw, want["nodes"], want["ins"], nRKsteps, want["hRK"], vcomp)
    n = _check(want, states, lines, flags)
    assert n > 100
    if hrk >= 1.0:  # long steps: some lines are cut short
        assert any(f for fl in flags for f in fl)


def test_is_per_gives_identical_output(ctx):
    out = []
    for per in ((0, 0, 0), (1, 1, 1)):
        H = nested_hierarchy(16, 2, 8, is_per=per)
        raw = _raw(H, 4, 2)
        nodes = _seeds(H, np.random.default_rng(5))
        want = R.run_tool(H.levels, raw, nodes, ["X", "Y", "Z"], np.array([1]), 1, nRKsteps=31, hRK=0.9)
        got = _device_run(ctx, H, raw, want["nodes"], want["ins"], 31, want["hRK"], None)
        _check(want, *got)
        out.append(got)
    for a, b in zip(out[0][0], out[1][0]):
        for q in range(a.level.nboxes):
            assert np.array_equal(np.ascontiguousarray(a.fab(q)).view(np.int64), np.ascontiguousarray(b.fab(q)).view(np.int64))
    for pa_, pb in zip(out[0][1], out[1][1]):
        for x, y in zip(pa_, pb):
            assert (x is None and y is None) or np.array_equal(x.view(np.int64), y.view(np.int64))


# ------------------------------------------------------------------------------------------------ the tool
NAMES = ["temp", "x_velocity", "y_velocity", "z_velocity", "density"]


def _plotfile(tmp_path):
    H = nested_hierarchy(16, 3, 8, is_per=(0, 0, 0))
    mfs = []
    for lv in H.levels:
        m = MultiFab(lv, len(NAMES), 0)
        fill_analytic(m, 0, lambda x, y, z: field_flame(x, y, z, 0))
        fill_analytic(m, 1, lambda x, y, z: np.sin(3 * y) + 0.2 * z + 0 * x)
        fill_analytic(m, 2, lambda x, y, z: np.cos(2 * x) - 0.1 * z + 0 * y)
        fill_analytic(m, 3, lambda x, y, z: 0.5 + 0.3 * x * y + 0 * z)
        fill_analytic(m, 4, lambda x, y, z: 1.0 / (1.0 + x + y * z))
        mfs.append(m)
    p = str(tmp_path / "plt00000")
    write_plotfile(p, H, mfs, NAMES, time=0.125)
    return p, H, mfs


def _tool(args, cwd):
    return subprocess.run([os.path.join(BIN, "stream3d.ex")] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def _want(H, mfs, comps, nodes, names, face, nElts, ng, nRKsteps=51, hRK=0.1, vcomp=None, bounds=None):
    raw = []
    for l, lv in enumerate(H.levels):
        m = MultiFab(lv, len(comps), ng)
        for q, c in enumerate(comps):
            for b in range(lv.nboxes):
                m.valid(b)[q] = mfs[l].valid(b)[c]
        raw.append(m)
    return R.run_tool(H.levels, raw, nodes, names, face, nElts, nRKsteps=nRKsteps, hRK=hRK, vcomp=vcomp, bounds=bounds)


def _compare_stream_dir(d, want, names, nRKsteps):
    files = R.stream_file_bytes(names, want["face"], want["nElts"], want["ins"], want["lines"], nRKsteps)
    for rel, data in files.items():
        got = open(os.path.join(d, rel), "rb").read()
        assert got == data, f"{rel} differs"


@pytest.mark.parametrize("variant", ["iso", "iso_aux_bounds", "iso_along_v", "rake", "seedloc"])
def test_tool_end_to_end(tmp_path, variant):
    p, H, mfs = _plotfile(tmp_path)
    base = ["plotfile=" + p]
    comps, vcomp, bounds, extra = [0], None, None, []
    if variant.startswith("iso"):
        iso = subprocess.run([os.path.join(BIN, "isosurface3d.ex"), "infile=" + p, "isoCompName=temp", "isoVal=1150", "comps=0 4"], cwd=tmp_path,
                             capture_output=True, text=True, timeout=600)
        assert iso.returncode == 0, iso.stderr
        mef = p + "_temp_1150.mef"
        label, mnames, mnodes, faces = read_mef(mef)
        nodes = np.ascontiguousarray(mnodes[:, :3].T)
        snames, face, nElts = mnames[:3], faces.ravel().astype(np.int32), faces.shape[0]
        base.append("isoFile=" + mef)
        assert nElts > 100
    elif variant == "rake":
        nodes = np.array([[0.3, 0.35, 0.5], [0.7, 0.62, 0.45]])
        nodes = (nodes[0][:, None] + (np.arange(7) / 6.0)[None, :] * (nodes[1] - nodes[0])[:, None])
        snames, face, nElts = ["X", "Y", "Z"], np.array([1], np.int32), 1
        base += ["seedRakeL=0.3 0.35 0.5", "seedRakeR=0.7 0.62 0.45", "seedRakeNum=7"]
    else:
        nodes = np.array([[0.41], [0.5], [0.47]])
        snames, face, nElts = ["X", "Y", "Z"], np.array([1], np.int32), 1
        base += ["seedLoc=0.41 0.5 0.47"]
    if variant == "iso_aux_bounds":
        comps = [0, 4, 2]
        bounds = np.array([0.3, 0.3, 0.3, 0.6, 0.7, 0.65])
        extra = ["aux_comps=4 2", "bounds=0.3 0.3 0.3 0.6 0.7 0.65", "nRKsteps=30", "hRK=0.4"]
    if variant == "iso_along_v":
        comps, vcomp = [0, 1, 2, 3, 4], 1
        extra = ["traceAlongV=1", "aux_sComp=4", "aux_nComp=1", "nGrow=3"]
    kw = dict(nRKsteps=30, hRK=0.4) if variant == "iso_aux_bounds" else {}
    ng = 3 if variant == "iso_along_v" else int(kw.get("hRK", 0.1) * ((kw.get("nRKsteps", 51) - 1) // 2)) + 2
    want = _want(H, mfs, comps, nodes, snames + [NAMES[c] for c in comps], face, nElts, ng, vcomp=vcomp, bounds=bounds, **kw)
    names = snames + [NAMES[c] for c in comps]
    nRK = kw.get("nRKsteps", 51)
    out = _tool(base + extra + ["streamFile=" + str(tmp_path / "lines")], tmp_path)
    assert out.returncode == 0, out.stderr + out.stdout
    _compare_stream_dir(str(tmp_path / "lines"), want, names, nRK)
    out = _tool(base + extra + ["outFile=" + str(tmp_path / "dump")], tmp_path)
    assert out.returncode == 0, out.stderr + out.stdout
    dat = R.out_file_bytes(names, want["lines"], nRK)
    assert dat is not None and open(tmp_path / "dump" / "str_00000.dat", "rb").read() == dat
    # is_per cannot change a byte
    out = _tool(base + extra + ["is_per=1 1 1", "streamFile=" + str(tmp_path / "lines_per")], tmp_path)
    assert out.returncode == 0, out.stderr
    for rel in R.stream_file_bytes(names, want["face"], want["nElts"], want["ins"], want["lines"], nRK):
        assert open(tmp_path / "lines_per" / rel, "rb").read() == open(tmp_path / "lines" / rel, "rb").read()


def test_tool_rejects(tmp_path):
    p, H, mfs = _plotfile(tmp_path)
    seed = ["plotfile=" + p, "seedLoc=0.41 0.5 0.47"]
    for args, msg in ((seed + ["buildAltSurf=1", "altVal=0.5", "outFile=o"], "buildAltSurf"),
                      (seed + ["progressName=nope", "outFile=o"], "Cannot find required data"),
                      (seed, "streamFile / outFile"),
                      (seed + ["outFile=o", "streamFile=s"], "streamFile / outFile")):
        out = _tool(args, tmp_path)
        assert out.returncode != 0 and msg in out.stderr, (args, out.stderr)
