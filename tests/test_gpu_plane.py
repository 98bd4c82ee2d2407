"""GPU tier of the plane tools: pa_plane_* through the C ABI and avgToPlane3d.ex / slicePlot3d.ex end to end, every case of
tests/plane_cases.py and every direction against the dense numpy restatement (tests/plane_ref.py), bit for bit and byte for byte."""
import os
import subprocess

import numpy as np
import pytest

import plane_cases as PC
import plane_ref as PR
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Level, MultiFab, disjoint_cover, regrid_copy, retile_level
from peleanalysis_amd.plotfile import write_plotfile
from util import SENT_GPU, bits_equal, sentinel_count

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")


def sentinel_plane(shape):
    """a host output that starts as the payload NaN of tests/util.py: a pixel the library never stored shows"""
    return np.full(shape, SENT_GPU, dtype=np.uint64).view(np.float64)


class Device:
    """the levels 0 .. finestLevel of a case on the device, optionally on another tiling of the same cells"""

    def __init__(self, ctx, c, retile=None):
        self.ctx, self.dls, self.mfs = ctx, [], []
        for l in range(c.nlev):
            m = c.mfs[l]
            if retile is not None:
                lv = retile(m.level, l)
                m2 = MultiFab(lv, m.ncomp, 0, fill=np.nan)
                regrid_copy(m, m2)
                m = m2
            dl = capi.DevLevel(ctx, m.level)
            self.dls.append(dl)
            self.mfs.append(capi.DevMF.from_host(ctx, dl, m))

    def close(self):
        for m in self.mfs:
            m.close()
        for dl in self.dls:
            dl.close()


def run_plane(ctx, c, dev, dir, comps, slice_=False):
    """-> (plane [len(comps)][height][width], nosrc, (mn, mx) of row 0, its pixel levels)"""
    box = c.slicebox(dir) if slice_ else c.subbox(dir)
    with capi.Plane(ctx, len(comps), dir, box, 0 if slice_ else c.max_grid_size) as P:
        P.run(dev.mfs, c.ratios[:c.finest], comps)
        out, nosrc = P.read(sentinel_plane((len(comps), P.height, P.width)))
        mn, mx = P.minmax(0)
        pix = P.pixelize(0, mn, mx)
    assert sentinel_count(out, SENT_GPU) == 0
    return out, nosrc, (mn, mx), pix


def assert_bits(got, want, what):
    if not bits_equal(got, want):
        bad = np.argwhere(np.ascontiguousarray(got).view(np.int64) != np.ascontiguousarray(want).view(np.int64))
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first at (comp, j', i') = {tuple(bad[0])}: got {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")


@pytest.mark.parametrize("dir", PC.DIRS)
@pytest.mark.parametrize("name", PC.CASES)
def test_abi_matches_reference(ctx, name, dir):
    c = PC.case(name)
    ref = PC.reference(name, dir)
    dev = Device(ctx, c)
    try:
        for what, slice_ in (("sum", False), ("slice", True)):
            out, nosrc, mm, pix = run_plane(ctx, c, dev, dir, [0, 1, 2], slice_)
            assert nosrc == 0
            assert_bits(out, ref[what], f"{name} dir {dir} {what}")
            assert mm == ref[what + "_minmax"]
            assert pix.dtype == np.uint8 and np.array_equal(pix, ref[what + "_pix"]), f"{name} dir {dir} {what}: pixel levels"
        if name == "nan_inf":  # a finite range of the user's: the +inf pixel is 255, the NaN pixel 0
            fin = ref["sum"][0][np.isfinite(ref["sum"][0])]
            with capi.Plane(ctx, 1, dir, c.subbox(dir), c.max_grid_size) as P:
                P.run(dev.mfs, c.ratios, [0])
                pix = P.pixelize(0, float(fin.min()), float(fin.max()))
            want = PR.pixelize(ref["sum"][0], float(fin.min()), float(fin.max()))
            assert np.array_equal(pix, want) and pix[np.isposinf(ref["sum"][0])] == 255 and pix[np.isnan(ref["sum"][0])] == 0
    finally:
        dev.close()


def _shuffled(level, l):
    perm = np.random.default_rng(11 + l).permutation(level.nboxes)
    return Level(level.boxes[perm], level.domlo, level.domhi, level.is_per, level.prob_lo, level.prob_hi)


def _chopped(level, l):
    """merged into the largest boxes the cell set allows, then chopped to 3 cells: odd sizes, boxes that do not start on a coarse cell's edge"""
    merged = retile_level(level, (64, 64, 64), 1)
    return Level(disjoint_cover(merged.boxes, 3), level.domlo, level.domhi, level.is_per, level.prob_lo, level.prob_hi)


@pytest.mark.parametrize("dir", PC.DIRS)
@pytest.mark.parametrize("name", ["three_levels", "wide"])
def test_same_bits_on_other_tilings_orders_and_groupings(ctx, name, dir):
    c = PC.case(name)
    ref = PC.reference(name, dir)
    for what, retile in (("shuffled boxes", _shuffled), ("boxes of 3 cells", _chopped)):
        dev = Device(ctx, c, retile)
        try:
            if retile is _chopped:
                assert any((dl.level.boxes[:, :3] % 2 != 0).any() for dl in dev.dls[1:])
            for kind, slice_ in (("sum", False), ("slice", True)):
                out, nosrc, _, pix = run_plane(ctx, c, dev, dir, [0, 1, 2], slice_)
                assert nosrc == 0
                assert_bits(out, ref[kind], f"{name} dir {dir} {kind}, {what}")
                assert np.array_equal(pix, ref[kind + "_pix"])
        finally:
            dev.close()
    dev = Device(ctx, c)
    try:
        for kind, slice_ in (("sum", False), ("slice", True)):
            out, nosrc, _, _ = run_plane(ctx, c, dev, dir, [2, 0, 1], slice_)
            assert nosrc == 0
            assert_bits(out, ref[kind][[2, 0, 1]], f"{name} dir {dir} {kind}, components in another order")
            for comp in range(3):
                out, nosrc, _, _ = run_plane(ctx, c, dev, dir, [comp], slice_)
                assert nosrc == 0
                assert_bits(out, ref[kind][[comp]], f"{name} dir {dir} {kind}, component {comp} alone")
        # more components than one launch of the sum kernels takes (4): rows repeat, every row its component's bits
        comps = [0, 1, 2, 2, 1, 0, 1]
        out, nosrc, _, _ = run_plane(ctx, c, dev, dir, comps)
        assert nosrc == 0
        assert_bits(out, ref["sum"][comps], f"{name} dir {dir} sum, seven rows")
    finally:
        dev.close()


def test_cells_no_level_holds_are_counted(ctx):
    c = PC.case("uneven_chunks")
    lv0 = c.levels[0]
    part = Level(np.array([[0, 0, 0, 7, 7, 3]], dtype=np.int32), lv0.domlo, lv0.domhi, lv0.is_per, lv0.prob_lo, lv0.prob_hi)  # k = 4 .. 7 missing
    m0 = MultiFab(part, 3, 0, fill=1.0)
    dl0, dl1 = capi.DevLevel(ctx, part), capi.DevLevel(ctx, c.levels[1])
    d0, d1 = capi.DevMF.from_host(ctx, dl0, m0), capi.DevMF.from_host(ctx, dl1, c.mfs[1])
    try:
        # fine cells without a source: the fine domain's upper half in z (16 x 16 x 8) minus the fine box's part there (8 x 8 x 4)
        for dir in PC.DIRS:
            with capi.Plane(ctx, 1, dir, c.domain(), 6) as P:
                P.run([d0, d1], c.ratios, [0])
                out, nosrc = P.read()
            assert nosrc == 16 * 16 * 8 - 8 * 8 * 4
            assert np.isnan(out).all() if dir == 2 else np.isnan(out[0, 8:]).all() and not np.isnan(out[0, :8]).any()  # every column along z meets them
    finally:
        for x in (d0, d1, dl0, dl1):
            x.close()


def test_invalid_arguments(ctx):
    c = PC.case("three_levels")
    dev = Device(ctx, c)
    dom = c.domain()
    try:
        for args, msg in (((1, 3, dom, 4), "dir must be"), ((1, -1, dom, 4), "dir must be"), ((0, 0, dom, 4), "no component"),
                          ((1, 2, (0, 0, 3, 31, 31, 4), 0), "one cell thick"), ((1, 0, (5, 0, 0, 4, 31, 31), 4), "empty sub-box")):
            with pytest.raises(capi.PaError, match=msg):
                capi.Plane(ctx, *args)
        def refused(P, levels, ratios, comps, msg):
            out = sentinel_plane((1, 32, 32))
            with pytest.raises(capi.PaError, match=msg):
                P.run(levels, ratios, comps)
            with pytest.raises(capi.PaError, match="no completed pa_plane_run"):
                P.read(out)
            assert sentinel_count(out, SENT_GPU) == out.size  # the output is untouched

        with capi.Plane(ctx, 1, 2, dom, 4) as P:
            refused(P, dev.mfs, c.ratios, [3], "component out of range")
            refused(P, dev.mfs, c.ratios, [-1], "component out of range")
            refused(P, dev.mfs * 3, c.ratios * 4 + [2], [0], "1 to 8 levels")
            refused(P, dev.mfs, [2, 4], [0], "not the coarser one refined")
            refused(P, [dev.mfs[0], dev.mfs[2]], [2], [0], "not the coarser one refined")
            refused(P, dev.mfs[:2], c.ratios[:1], [0], "not inside the finest level's domain")  # the box is level 2's domain
            P.run(dev.mfs, c.ratios, [0])  # and the object still works
            got, nosrc = P.read(sentinel_plane((1, 32, 32)))
            assert nosrc == 0 and sentinel_count(got, SENT_GPU) == 0
        with capi.Plane(ctx, 1, 0, (0, 0, 0, 32, 31, 31), 4) as P:
            refused(P, dev.mfs, c.ratios, [0], "not inside the finest level's domain")
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ the tools, end to end
def _tool(exe, args, cwd):
    return subprocess.run([os.path.join(BIN, exe)] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def _written(c, d):
    p = str(d / "in" / "plt00042")
    os.makedirs(d / "in")
    write_plotfile(p, c.hier, c.mfs, PC.NAMES, time=0.5)
    (d / "pal").write_bytes(PC.palette_bytes(alpha=True))
    return p


@pytest.mark.parametrize("name", ["three_levels", "subbox_odd"])
def test_avgtoplane_end_to_end(tmp_path, name):
    c = PC.case(name)
    plt = _written(c, tmp_path)
    pal = PR.load_palette(PC.palette_bytes(alpha=True))
    for dir in PC.DIRS:
        ref = PC.reference(name, dir)
        args = ["infile=" + plt, "palette=pal", "dir=%d" % dir, "max_grid_size=%d" % c.max_grid_size, "sumfile=sums.bin"]
        if name == "subbox_odd":
            args.append("box=" + " ".join(str(x) for x in c.subbox(dir)))
        (tmp_path / "plt00042.ppm").write_bytes(b"old" * 100000)  # overwritten
        r = _tool("avgToPlane3d.ex", args, tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert r.stdout.split("\n")[:3] == ["Filling %s on level 2" % n for n in PC.NAMES]
        assert (tmp_path / "plt00042.ppm").read_bytes() == PR.ppm_bytes(ref["sum_pix"], pal)  # the default name, the first component
        assert (tmp_path / "sums.bin").read_bytes() == PR.sumfile_bytes(ref["sum"])
        # the user's range and another choice of components: the image is the first one's
        mn, mx = -3.5e3, 1.25e5
        r = _tool("avgToPlane3d.ex", args + ["comps=2 0", "min=%r" % mn, "max=%r" % mx], tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert (tmp_path / "plt00042.ppm").read_bytes() == PR.ppm_bytes(PR.pixelize(ref["sum"][2], mn, mx), pal)
        assert (tmp_path / "sums.bin").read_bytes() == PR.sumfile_bytes(ref["sum"][[2, 0]])
    # finestLevel below the file's: the coarser domain, the finer level unread
    if name == "three_levels":
        ref = PC.reference("below_finest", 1)
        b = PC.case("below_finest")
        plt2 = str(tmp_path / "in" / "plt00043")
        write_plotfile(plt2, b.hier, b.mfs, PC.NAMES)
        r = _tool("avgToPlane3d.ex", ["infile=" + plt2, "palette=pal", "dir=1", "max_grid_size=7", "finestLevel=1", "sComp=1", "nComp=1", "sumfile=s1.bin"], tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert r.stdout.split("\n")[0] == "Filling b on level 1"
        assert (tmp_path / "s1.bin").read_bytes() == PR.sumfile_bytes(ref["sum"][[1]])
        mn, mx = PR.minmax(ref["sum"][1])
        assert (tmp_path / "plt00043.ppm").read_bytes() == PR.ppm_bytes(PR.pixelize(ref["sum"][1], mn, mx), pal)


@pytest.mark.parametrize("name", ["three_levels", "subbox_odd"])
def test_sliceplot_end_to_end(tmp_path, name):
    c = PC.case(name)
    plt = _written(c, tmp_path)
    pal = PR.load_palette(PC.palette_bytes(alpha=True))
    dom = c.domain()
    for dir in PC.DIRS:
        loc = c.sliceloc(dir)
        box = list(dom)
        box[dir] = box[3 + dir] = loc
        F, nosrc = PR.composite(c.levels, c.mfs, c.ratios, box[:3], box[3:], (1,))
        want = PR.plane_slice(F, dir)[0]
        mn, mx = PR.minmax(want)
        args = ["file=" + plt, "slicedir=%d" % dir, "sliceloc=%d" % loc, "varname=b"]
        r = _tool("slicePlot3d.ex", args + ["palette=pal"], tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert r.stdout.split("\n")[0] == "min,max: %s, %s" % ("%g" % mn, "%g" % mx)
        assert (tmp_path / "plt00042.ppm").read_bytes() == PR.ppm_bytes(PR.pixelize(want, mn, mx), pal)
        r = _tool("slicePlot3d.ex", args + ["outtype=gray", "min=-10", "max=2.5e4"], tmp_path)  # no palette needed
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert (tmp_path / "plt00042.pgm").read_bytes() == PR.pgm_bytes(PR.pixelize(want, -10.0, 2.5e4))
        r = _tool("slicePlot3d.ex", args + ["outtype=gray", "outfile=named.pgm"], tmp_path)
        assert r.returncode == 0 and (tmp_path / "named.pgm").read_bytes() == PR.pgm_bytes(PR.pixelize(want, mn, mx))
    before = sorted(os.listdir(tmp_path))
    r = _tool("slicePlot3d.ex", ["file=" + plt, "slicedir=0", "sliceloc=3", "varname=a", "outtype=fab", "outfile=never"], tmp_path)
    assert r.returncode == 0 and r.stdout.startswith("min,max: ") and sorted(os.listdir(tmp_path)) == before


def test_tools_refuse_before_they_write(tmp_path):
    c = PC.case("three_levels")
    plt = _written(c, tmp_path)
    before = sorted(os.listdir(tmp_path))
    (tmp_path / "short").write_bytes(PC.palette_bytes()[:700])
    before = sorted(os.listdir(tmp_path))
    for exe, args, msg in (("avgToPlane3d.ex", ["infile=" + plt, "sumfile=s.bin"], "palette not found"),
                           ("avgToPlane3d.ex", ["infile=" + plt, "palette=pal", "dir=3", "sumfile=s.bin"], "dir must be 0, 1 or 2"),
                           ("avgToPlane3d.ex", ["infile=" + plt, "palette=short", "sumfile=s.bin"], "shorter than 768 bytes"),
                           ("avgToPlane3d.ex", ["infile=" + plt, "palette=pal", "box=0 0 0 32 31 31", "sumfile=s.bin"], "not inside the domain"),
                           ("slicePlot3d.ex", ["file=" + plt, "slicedir=1", "sliceloc=32", "varname=a", "palette=pal"], "sliceloc is outside the domain"),
                           ("slicePlot3d.ex", ["file=" + plt, "slicedir=1", "sliceloc=3", "varname=a"], "palette not found"),
                           ("slicePlot3d.ex", ["file=" + plt, "slicedir=1", "sliceloc=3", "varname=nosuch", "palette=pal"], "is not a variable")):
        r = _tool(exe, args, tmp_path)
        assert r.returncode != 0 and msg in r.stderr, (exe, args, r.returncode, r.stderr[-500:])
        assert sorted(os.listdir(tmp_path)) == before, (exe, args)
