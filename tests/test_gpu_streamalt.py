"""GPU tier of the alternate-surface mode of stream3d (stream.cpp buildAltSurf; pa_streamalt.hip): the kernel on every case of
tests/streamalt_cases.py against the plain-Python restatement tests/streamalt_ref.py, as int64 views, bit for bit (the angle's
cosine and the branch codes too), and the tool on the small plotfile of test_gpu_streamgrad.py against the restatement applied to
streamgrad_ref's lines, byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import streamalt_cases as K
import streamalt_ref as A
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import MultiFab
from peleanalysis_amd.plotfile import read_mef, write_plotfile
from test_gpu_streamgrad import BIN, NAMES, _compare_stream_dir, _plotfile, _tool, _want
from util import SENT_GPU, bits_equal, sentinel_count

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("subset", list(K.SUBSETS))
@pytest.mark.parametrize("nRKsteps", K.NRK)
def test_kernel_matches_restatement(ctx, nRKsteps, subset):
    lines, ins, nNodes = K.build(nRKsteps)
    want, wbranch, _ = K.reference(nRKsteps, subset)
    got, branch = capi.streamalt_run(ctx, lines, ins, nRKsteps, nNodes, K.ISO, K.ALT_VAL, out_fill=SENT_GPU, **K.SUBSETS[subset])
    assert got.shape == want.shape and branch.shape == wbranch.shape
    assert sentinel_count(got, SENT_GPU) == 0, "a node was never written"
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert len(bad) == 0, f"{len(bad)} values differ, first (component, node) {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    assert np.array_equal(branch, wbranch)
    # the codes are optional: the same bits without them
    got2, none = capi.streamalt_run(ctx, lines, ins, nRKsteps, nNodes, K.ISO, K.ALT_VAL, out_fill=SENT_GPU, with_branch=False, **K.SUBSETS[subset])
    assert none is None and bits_equal(got2, want)


def test_kernel_leaves_nodes_without_a_line_alone(ctx):
    """twice as many nodes as lines: the other columns keep the bits they had"""
    lines, ins, nNodes = K.build(5)
    want, _, _ = K.reference(5, "all")
    ins2 = [[(2 * np.asarray(i)).astype(np.int32) for i in per] for per in ins]
    got, branch = capi.streamalt_run(ctx, lines, ins2, 5, 2 * nNodes, K.ISO, K.ALT_VAL, out_fill=SENT_GPU, **K.SUBSETS["all"])
    assert bits_equal(got[:, 1::2], want)
    assert sentinel_count(got[:, 0::2], SENT_GPU) == got[:, 0::2].size and (branch[:, 0::2] == -1).all()


def test_kernel_argument_checks(ctx):
    lines, ins, nNodes = K.build(5)
    ok = dict(K.SUBSETS["all"])
    for kw, msg in ((dict(isoComp=K.NCS), "progress component"), (dict(isoComp=-1), "progress component"), (dict(carry=(K.NCS,)), "carried component"),
                    (dict(thickComp=K.NCS), "thickness component"), (dict(TComp=K.NCS), "T component"), (dict(strainComp=-1), "strain component"),
                    (dict(strainComp=K.NCS), "strain component"), (dict(carry=tuple(range(9))), "8 carried")):
        args = dict(ok, isoComp=K.ISO)
        args.update(kw)
        iso = args.pop("isoComp")
        with pytest.raises(capi.PaError, match=msg):
            capi.streamalt_run(ctx, lines, ins, 5, nNodes, iso, K.ALT_VAL, **args)
    two = [[None if x is None else x[:, :2] for x in per] for per in lines]
    with pytest.raises(capi.PaError, match="nRKsteps"):
        capi.streamalt_run(ctx, two, ins, 2, nNodes, K.ISO, K.ALT_VAL, **ok)
    for bad in (0, nNodes + 1):  # a node id outside 1 .. nNodes: refused before anything is written
        ins2 = [[np.array(i, np.int32) for i in per] for per in ins]
        ins2[1][3][200] = bad
        with pytest.raises(capi.PaError, match="node id"):
            capi.streamalt_run(ctx, lines, ins2, 5, nNodes, K.ISO, K.ALT_VAL, **ok)


# ------------------------------------------------------------------------------------------------ the tool
ISO_C, VEL_C, DENS_C = 3, 4, 7  # line components of the tool with buildAltSurf and aux_comps=4: X Y Z temp x/y/z_velocity density


@pytest.fixture(scope="module")
def flame(tmp_path_factory):
    """the plotfile of test_gpu_streamgrad.py, its temp = 1150 surface as isosurface3d writes it, the same surface with a
    distance_iso_to_alt column, and a plotfile without z_velocity"""
    d = tmp_path_factory.mktemp("streamalt")
    p, H, mfs = _plotfile(d)
    iso = subprocess.run([os.path.join(BIN, "isosurface3d.ex"), "infile=" + p, "isoCompName=temp", "isoVal=1150", "comps=0 4"], cwd=d, capture_output=True,
                         text=True, timeout=600)
    assert iso.returncode == 0, iso.stderr
    mef = p + "_temp_1150.mef"
    label, mnames, mnodes, faces = read_mef(mef)
    face, nElts = faces.ravel().astype(np.int32), faces.shape[0]
    dist = np.random.default_rng(3).normal(0.0, 0.01, mnodes.shape[0])
    mef_d = str(d / "with_distance.mef")
    with open(mef_d, "wb") as f:
        f.write(A.mef_bytes(label, list(mnames[:3]) + [A.DISTANCE_NAME, "density"], np.stack([mnodes[:, 0], mnodes[:, 1], mnodes[:, 2], dist, mnodes[:, 4]]), face, nElts))
    keep = [0, 1, 2, 4]
    sub = []
    for m in mfs:
        s = MultiFab(m.level, len(keep), 0)
        for b in range(m.level.nboxes):
            s.valid(b)[:] = m.valid(b)[keep]
        sub.append(s)
    p_nov = str(d / "plt_noz")
    write_plotfile(p_nov, H, sub, [NAMES[c] for c in keep], time=0.125)
    return dict(dir=d, plt=p, H=H, mfs=mfs, mef=mef, mef_d=mef_d, snames=list(mnames[:3]), nodes=np.ascontiguousarray(mnodes[:, :3].T), face=face, nElts=nElts,
                dist=dist, plt_noz=p_nov, want={})


def _lines(flame, comps):
    """streamgrad_ref's run of the tool for these plotfile components (once per module; nobody writes into it)"""
    key = tuple(comps)
    if key not in flame["want"]:
        names = flame["snames"] + [NAMES[c] for c in comps]
        flame["want"][key] = (_want(flame["H"], flame["mfs"], list(comps), flame["nodes"], names, flame["face"], flame["nElts"], 4), names)
    return flame["want"][key]


VARIANTS = {
    # name: (tool keys, restatement options, advect, dt, surface with a distance column, aux components)
    "plain": (["altVal=1300"], dict(carry=(ISO_C,)), False, 0.0, False, []),
    "plain_with_distance": (["altVal=1300"], dict(carry=(ISO_C,)), False, 0.0, True, []),
    "advect": (["altVal=700", "advectColdIso=1", "dt=0.0078125"], dict(carry=(VEL_C, VEL_C + 1, VEL_C + 2, ISO_C)), True, 0.0078125, False, []),
    "thick_strain_angle": (["altVal=1300", "thickCompName=temp", "thickLo=800", "thickHi=1500", "strainCompName=density", "TCompName=temp", "TVal=600", "addAngle=1",
                            "aux_comps=4"],
                           dict(carry=(ISO_C,), thickComp=ISO_C, thickLo=800.0, thickHi=1500.0, TComp=ISO_C, TVal=600.0, strainComp=DENS_C, addAngle=True), False, 0.0,
                           False, [4]),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tool_builds_the_alternate_surface(flame, tmp_path, variant):
    keys, opts, advect, dt, with_dist, aux = VARIANTS[variant]
    altVal = float(keys[0].split("=")[1])
    comps = [0, 1, 2, 3] + aux  # buildAltSurf puts the velocities among the line components although the trace follows the gradient
    w, names = _lines(flame, comps)
    nN = w["nodes"].shape[1]
    out, branch, _ = A.alt_surface(w["lines"], w["ins"], 51, nN, ISO_C, altVal, **opts)
    assert not np.isnan(out).any() and (branch[0] == 1).any()  # some line meets the surface
    fin, fnames = A.post_step(out, A.surface_names(names, opts["carry"], opts.get("thickComp", -1), opts.get("TComp", -1), opts.get("addAngle", False), advect),
                              len(opts["carry"]), opts.get("addAngle", False), advect, dt, flame["dist"] if with_dist else None)
    label = "advected alt surface" if advect else "new flame surface from advected alt"
    want_mef = A.mef_bytes(label, fnames, fin, w["face"], w["nElts"])
    base = ["plotfile=" + flame["plt"], "isoFile=" + (flame["mef_d"] if with_dist else flame["mef"]), "buildAltSurf=1"] + keys
    # the default name, in the working directory, next to the streamFile tree
    r = _tool(base + ["streamFile=" + str(tmp_path / "lines")], tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    got = open(tmp_path / ("surf_alt.mef" if advect else "surf_new_flame.mef"), "rb").read()
    assert got == want_mef
    _compare_stream_dir(str(tmp_path / "lines"), w, names, 51)
    for msg in ("building new surface at level: 2", "New surface built, communicating info to ioproc", "Data sent, building new iso", "New iso built on ioproc",
                "Finished writing streamline data"):
        assert msg in r.stderr
    if variant == "thick_strain_angle":
        for msg in ("Thermal thickness computed, communicating info to ioproc", "Cold Strain computed, communicating info to ioproc",
                    "Angle computed, communicating info to ioproc"):
            assert msg in r.stderr
        assert "Thermal thickness component id: 3" in r.stdout and "Strain component id: 7" in r.stdout and "T component for strain eval at id: 3" in r.stdout
        assert fnames == ["X", "Y", "Z", "temp", "delta", "thermalThickness_notAdv", "coldStrain", "angleWRTvert"]
    # altIsoFile=
    r = _tool(base + ["altIsoFile=" + str(tmp_path / "named.mef"), "outFile=" + str(tmp_path / "dump"), "verbose=1"], tmp_path)
    assert r.returncode == 0, r.stderr + r.stdout
    assert open(tmp_path / "named.mef", "rb").read() == want_mef
    assert "building new surface where temp = " in r.stdout


def test_tool_new_aborts_and_skips(flame, tmp_path):
    base = ["plotfile=" + flame["plt"], "isoFile=" + flame["mef"], "buildAltSurf=1", "altVal=1300", "outFile=o"]
    for args, msg in ((["plotfile=" + flame["plt"], "seedLoc=0.41 0.5 0.47", "buildAltSurf=1", "altVal=1300", "outFile=o"], "buildAltSurf"),
                      (["plotfile=" + flame["plt"], "seedRakeL=0.3 0.35 0.5", "seedRakeR=0.7 0.62 0.45", "buildAltSurf=1", "altVal=1300", "outFile=o"], "buildAltSurf"),
                      (base + ["nRKsteps=2"], "nRKsteps"),
                      (["plotfile=" + flame["plt_noz"]] + base[1:], "z_velocity"),
                      (base + ["strainCompName=nope", "TCompName=temp", "TVal=600"], "strainCompName=nope"),
                      (base[:3] + ["outFile=o"], "altVal")):
        r = _tool(args, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (args, r.stderr)
        assert not os.path.exists(tmp_path / "surf_new_flame.mef")
    # a thickness or T component that is not among the line components: skipped as in the reference, named on stderr
    r = _tool(base + ["thickCompName=nope", "thickLo=1", "thickHi=2", "strainCompName=temp", "TCompName=nada", "TVal=1"], tmp_path)
    assert r.returncode == 0 and "thickCompName=nope" in r.stderr and "TCompName=nada" in r.stderr, r.stderr
    assert read_mef(str(tmp_path / "surf_new_flame.mef"))[1] == ["X", "Y", "Z", "temp", "delta"]
    # the keys of the mode without buildAltSurf=1 are read by nobody
    r = _tool(["plotfile=" + flame["plt"], "isoFile=" + flame["mef"], "altVal=1300", "dt=1", "addAngle=1", "advectColdIso=1", "thickCompName=temp",
               "altIsoFile=never.mef", "streamFile=" + str(tmp_path / "plain")], tmp_path)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(tmp_path / "never.mef") and not os.path.exists(tmp_path / "surf_alt.mef")
    w, names = _lines(flame, [0])
    _compare_stream_dir(str(tmp_path / "plain"), w, names, 51)
