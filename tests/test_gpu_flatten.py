"""GPU tier of flattenAMRFile3d: pa_flatten_level through the C ABI and flattenAMRFile3d.ex end to end, every case of
tests/flatten_cases.py at every output level it has against the dense numpy restatement (tests/flatten_ref.py), compared as
uint64: the file's own cells keep their bits, the others are the interpolant in the kernels' operation order."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

import flatten_cases as FC
import flatten_ref as FR
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, chop_box, regrid_copy
from peleanalysis_amd.plotfile import read_plotfile, write_plotfile
from util import SENT_GPU, sentinel_count, sentinel_mf, sentinel_out

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin")


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def run_abi(ctx, c, L, interp_type, out_boxes=None, crse_mgs=None, check_ghosts=False):
    """V(file, L) of case c through pa_flatten_level: (host multifab on the output boxes, cells without source data, launch record
    of the output level's call).  The levels below L are work multifabs on chop(domain, crse_mgs or the case's grid size) with the
    ghost layers of Flatten.ghosts; out_boxes: the output level's boxes (any disjoint list: a slab, shuffled, another tiling)"""
    nvar = len(c.names)
    ratios = [c.ratio] * L
    lev_out = c.out_level(L, out_boxes)
    result = MultiFab(lev_out, nvar, 0, fill=np.nan)
    nosrc, launch = 0, None
    fl = capi.Flatten(ctx)
    fdev = []
    for l in range(L + 1):
        dl = capi.DevLevel(ctx, c.mfs[l].level)
        fdev.append((dl, capi.DevMF.from_host(ctx, dl, c.mfs[l])))
    V, _ = FC.reference(c.name, interp_type)
    for v0 in range(0, nvar, 16):
        vs = list(range(v0, min(nvar, v0 + 16)))
        keep, crse = [], None
        for l in range(L + 1):
            last = l == L
            lv = lev_out if last else c.out_level(l, c.out_boxes(l, crse_mgs))
            dl = capi.DevLevel(ctx, lv)
            out = sentinel_out(ctx, dl, len(vs), 0 if last else capi.Flatten.ghosts(L + 1, l, ratios, interp_type))
            nosrc += fl.level(fdev[l][1], [c.comps[v] for v in vs], crse, c.ratio, interp_type, out, len(vs))
            keep.append((dl, out))
            if last:
                launch = fl.last_launch()
                got = out.download()
                for b in range(lv.nboxes):
                    result.valid(b)[v0:v0 + len(vs)] = got.valid(b)
            elif check_ghosts and out.ng > 0:  # a work multifab: every valid AND ghost cell holds its canonical cell's value
                got = out.download()
                for b in range(lv.nboxes):
                    want = FR.canonical_fab(V[l][vs], lv.boxes[b], out.ng, c.is_per)
                    assert np.array_equal(u64(got.fab(b)), u64(want)), f"{c.name} level {l} box {b}: valid or ghost cells differ"
            crse = out
        for dl, m in keep:
            m.close()
            dl.close()
    for dl, m in fdev:
        m.close()
        dl.close()
    return result, nosrc, launch


def check(c, got, L, interp_type, what):
    V, _ = FC.reference(c.name, interp_type)
    want = FC.dense_to_mf(V[L], got.level)
    for b in range(got.level.nboxes):
        g, w = u64(got.valid(b)), u64(want.valid(b))
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            v, k, j, i = bad[0]
            raise AssertionError(f"{what}: box {b} {got.level.boxes[b]}: {len(bad)} cells differ, first var {v} at (i,j,k)=({i},{j},{k}) local: got "
                                 f"{got.valid(b)[v, k, j, i]!r} ({g[v, k, j, i]:#x}) want {want.valid(b)[v, k, j, i]!r} ({w[v, k, j, i]:#x}); "
                                 f"{sentinel_count(got.valid(b), SENT_GPU)} cells never written")


PAIRS = [(n, l) for n in FC.CASES for l in FC.case(n).outs]


@pytest.mark.parametrize("interp_type", FC.INTERP_TYPES)
@pytest.mark.parametrize("name,L", PAIRS, ids=[f"{n}-L{l}" for n, l in PAIRS])
def test_abi_matches_reference(ctx, name, L, interp_type):
    c = FC.case(name)
    got, nosrc, launch = run_abi(ctx, c, L, interp_type, check_ghosts=True)
    check(c, got, L, interp_type, f"{name} level {L} interp {interp_type}")
    assert launch == c.expected_launch(L), (launch, c.expected_launch(L))
    if c.general_only or L == 0:
        assert launch[0] == 0 and launch[2] == 0 and launch[1] == got.level.nboxes
    want_nosrc = FR.no_source_cells(c.mfs, L, c.n0, c.ratio)
    assert nosrc == want_nosrc * -(-len(c.names) // 16)  # cells, once per pass of at most 16 variables
    if name == "hole0":
        assert nosrc == 8 * 8 * 4
        assert sum(int(np.isnan(got.valid(b)[0]).sum()) for b in range(got.level.nboxes)) == nosrc
    if name == "rawbits":
        allbits = np.concatenate([u64(got.valid(b)).ravel() for b in range(got.level.nboxes)])
        assert int((allbits == FC.NEG_ZERO).sum()) == 4 and int((allbits == FC.NAN_PAYLOAD).sum()) == 4


@pytest.mark.parametrize("interp_type", FC.INTERP_TYPES)
@pytest.mark.parametrize("name", ["coverage", "coverage_r4", "mixed_routes", "avg_periodic_wall_f0", "wide80_r2"])
def test_same_bits_for_slabs_shuffles_and_coarse_tilings(ctx, name, interp_type):
    c = FC.case(name)
    L = c.nlev - 1
    ob = c.out_boxes(L)
    # a slab: a sub-list of the level's boxes
    sub = ob[len(ob) // 3: 2 * len(ob) // 3 + 1]
    got, nosrc, launch = run_abi(ctx, c, L, interp_type, out_boxes=sub)
    assert nosrc == 0 and launch == c.expected_launch(L, sub)
    check(c, got, L, interp_type, f"{name}: a slab of {len(sub)} boxes")
    # the boxes in another order
    perm = np.random.default_rng(5).permutation(len(ob))
    got, nosrc, launch = run_abi(ctx, c, L, interp_type, out_boxes=ob[perm])
    assert nosrc == 0 and launch == c.expected_launch(L)
    check(c, got, L, interp_type, f"{name}: shuffled boxes")
    # the coarser work multifabs on another tiling (pieces of 6 and 7 cells: coarse boxes that end inside an output box)
    got, nosrc, _ = run_abi(ctx, c, L, interp_type, crse_mgs=7)
    assert nosrc == 0
    check(c, got, L, interp_type, f"{name}: coarse level in pieces of 7")
    # both routes give the same bits: boxes of 5 cells in x (general) against the case's own
    got, nosrc, launch = run_abi(ctx, c, L, interp_type, out_boxes=c.out_boxes(L, 5))
    assert nosrc == 0 and launch[1] > 0
    check(c, got, L, interp_type, f"{name}: output boxes of 5 cells")


@pytest.mark.parametrize("name", ["rawbits", "avg_three_files_f0"])
def test_same_values_as_a_one_file_average(ctx, name):
    """pa_resample_* with one file on the same boxes: equal bits, except that 0.0 + (-0.0) is +0.0 there"""
    c = FC.case(name)
    L = c.nlev - 1
    nvar = len(c.names)
    got, _, _ = run_abi(ctx, c, L, 1)
    levels = [c.out_level(l) for l in range(L + 1)]
    dls = [capi.DevLevel(ctx, lv) for lv in levels]
    fdev = []
    for l in range(L + 1):
        dl = capi.DevLevel(ctx, c.mfs[l].level)
        fdev.append((dl, capi.DevMF.from_host(ctx, dl, c.mfs[l])))
    ratios = [c.ratio] * L
    with capi.Resample(ctx) as rs:
        run = [sentinel_out(ctx, dl, nvar, 0) for dl in dls]
        work = [sentinel_out(ctx, dls[l], nvar, capi.Resample.ghosts(L + 1, l, ratios, 1)) if l < L else None for l in range(L + 1)]
        rs.begin(run, nvar)
        for l in range(L + 1):
            rs.add_file_level(l, fdev[l][1], c.comps, work[l - 1] if l else None, c.ratio, 1, work[l])
        assert rs.finish(1) == 0
        avg = run[L].download()
        for m in run + [w for w in work if w is not None]:
            m.close()
    for dl, m in fdev:
        m.close()
        dl.close()
    for dl in dls:
        dl.close()
    zeros = 0
    for b in range(levels[L].nboxes):
        g, a = got.valid(b), avg.valid(b)
        same = (u64(g) == u64(a)) | ((g == 0.0) & (a == 0.0)) | (np.isnan(g) & np.isnan(a))
        assert same.all(), f"{name} box {b}: {int((~same).sum())} cells differ from the one-file average"
        zeros += int(((u64(g) != u64(a)) & (g == 0.0)).sum())
    if name == "rawbits":
        assert zeros == 4  # the file's -0.0 cells: +0.0 in the average


def _level1_setup(ctx, c, interp_type):
    """case c flattened at level 1 by hand: (file level 1 on the device, the coarse work multifab, everything to close)"""
    nvar = len(c.names)
    fl = capi.Flatten(ctx)
    f0l = capi.DevLevel(ctx, c.mfs[0].level)
    f0 = capi.DevMF.from_host(ctx, f0l, c.mfs[0])
    wl = capi.DevLevel(ctx, c.out_level(0))
    work = sentinel_out(ctx, wl, nvar, capi.Flatten.ghosts(2, 0, [c.ratio], interp_type))
    assert fl.level(f0, c.comps, None, c.ratio, interp_type, work, nvar) == 0
    f1l = capi.DevLevel(ctx, c.mfs[1].level)
    f1 = capi.DevMF.from_host(ctx, f1l, c.mfs[1])
    return fl, f1, work, [f1, f1l, work, wl, f0, f0l]


def test_plans_are_reused_and_evicted(ctx):
    """the launch tables are kept with the output level by file level: a second call on the same pair reuses them, the ninth file
    level evicts them all, and a call after that builds them again -- the same bits and the same record every time"""
    c = FC.case("coverage")
    nvar = len(c.names)
    fl, f1, work, keep = _level1_setup(ctx, c, 1)
    lv = c.out_level(1)
    dl = capi.DevLevel(ctx, lv)
    want = c.expected_launch(1)

    def once(fmf, what):
        out = sentinel_out(ctx, dl, nvar, 0)  # a new multifab on the SAME level: the level's tables serve it
        assert fl.level(fmf, c.comps, work, c.ratio, 1, out, nvar) == 0
        assert fl.last_launch() == want, what
        got = out.download()
        out.close()
        check(c, got, 1, 1, what)

    once(f1, "first call")
    once(f1, "second call on the same pair")
    others = []
    for k in range(9):  # nine more file levels with the same boxes in other orders: more than the eight sets a level keeps
        m = c.mfs[1]
        perm = np.random.default_rng(100 + k).permutation(m.level.nboxes)
        l2 = Level(m.level.boxes[perm], m.level.domlo, m.level.domhi, m.level.is_per, m.level.prob_lo, m.level.prob_hi)
        m2 = MultiFab(l2, m.ncomp, 0, fill=np.nan)
        regrid_copy(m, m2)
        fdl = capi.DevLevel(ctx, l2)
        fm = capi.DevMF.from_host(ctx, fdl, m2)
        others += [fm, fdl]
        once(fm, f"file level {k} in another box order")
    once(f1, "the first pair again, after its tables were evicted")
    once(others[0], "an evicted pair again")
    for x in others + [dl] + keep:
        x.close()


@pytest.mark.parametrize("name", ["coverage", "wide80_r2"])
def test_unaligned_output_takes_the_general_route(ctx, name):
    """an output multifab on a caller's pointer that is 8 bytes off a 16-byte boundary: no row can be stored as 16-byte vectors,
    every box must be reported on the general route, with the same bits"""
    c = FC.case(name)
    nvar = len(c.names)
    fl, f1, work, keep = _level1_setup(ctx, c, 1)
    lv = c.out_level(1)
    dl = capi.DevLevel(ctx, lv)
    assert c.expected_launch(1)[0] > 0  # aligned, the case takes the wide route
    backing = capi.DevMF(ctx, dl, nvar + 1, 0)  # one component more: room for the multifab shifted by one double
    out = capi.DevMF(ctx, dl, nvar, 0, devptr=backing.ptr + 8)
    assert out.ptr % 16 == 8 and out.size + 1 <= backing.size
    out.upload(sentinel_mf(lv, nvar, 0, SENT_GPU))
    assert fl.level(f1, c.comps, work, c.ratio, 1, out, nvar) == 0
    assert fl.last_launch() == (0, lv.nboxes, 0, 0)
    got = out.download()
    check(c, got, 1, 1, f"{name}: output 8 bytes off")
    for x in [out, backing, dl] + keep:
        x.close()


# ------------------------------------------------------------------------------------------------ the tool, end to end
def _tool(args, cwd):
    return subprocess.run([os.path.join(BIN, "flattenAMRFile3d.ex")] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def _write_case(c, d, name="plt00123"):
    p = str(d / name)
    write_plotfile(p, c.hier, c.mfs, c.names, time=0.625, level_steps=[11] * c.nlev)
    return p


def _same_tree(a, b):
    for f in ("Header", "Level_0/Cell_H", "Level_0/Cell_D_00000"):
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), (a, b, f)
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["Header", "Level_0"]
    assert sorted(os.listdir(os.path.join(a, "Level_0"))) == sorted(os.listdir(os.path.join(b, "Level_0"))) == ["Cell_D_00000", "Cell_H"]


def _check_tool_output(c, out, L, interp_type, mgs):
    P = read_plotfile(out, c.is_per)
    assert P.names == c.names and P.hier.nlev == 1 and P.time == 0.625 and P.level_steps[:1] == [0]
    lv = P.hier.levels[0]
    lo, hi = c.domain(L)
    assert tuple(lv.domlo) == lo and tuple(lv.domhi) == hi
    assert np.array_equal(lv.boxes, chop_box(lo, hi, mgs))  # domain(output_level).maxSize(output_max_grid_size)
    with open(os.path.join(out, "Header")) as f:
        lines = f.read().split("\n")
    dx_line = lines[2 + len(c.names) + 8].split()  # the cell size of the output level
    assert [float(x) for x in dx_line] == [1.0 / (h + 1) for h in hi]
    check(c, P.mfs[0], L, interp_type, f"tool {c.name} level {L} interp {interp_type}")


TOOL_PAIRS = [(n, l) for n in ("avg_three_files_f0", "avg_ratio4_f1", "coverage", "mixed_routes", "vars17", "rawbits", "offalign7") for l in FC.case(n).outs]


@pytest.mark.parametrize("interp_type", FC.INTERP_TYPES)
@pytest.mark.parametrize("name,L", TOOL_PAIRS, ids=[f"{n}-L{l}" for n, l in TOOL_PAIRS])
def test_tool_every_output_level(tmp_path, name, L, interp_type):
    c = FC.case(name)
    p = _write_case(c, tmp_path)
    out = str(tmp_path / "flat")
    r = _tool(["infile=" + p, "output_file=" + out, "output_level=%d" % L, "output_max_grid_size=%d" % c.mgs, "interp_type=%d" % interp_type,
               "is_per=%d %d %d" % c.is_per], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _check_tool_output(c, out, L, interp_type, c.mgs)


def test_tool_defaults(tmp_path):
    """output_file=<root>_flatten, output_level=0, output_max_grid_size=64, interp_type=1"""
    c = FC.case("avg_same_level1_f0")
    p = _write_case(c, tmp_path)
    r = _tool(["infile=" + p + "/", "verbose=1"], tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " Reading data from pltfile " + p + "/" in r.stdout and " Interpolate data " in r.stdout and " Writting data " in r.stdout
    c0 = FC.Case.__new__(FC.Case)
    c0.__dict__.update(c.__dict__)
    c0.is_per = (0, 0, 0)  # level 0 is the file's own data: periodicity does not matter
    _check_tool_output(c0, str(tmp_path / "plt00123_flatten"), 0, 1, 64)


@pytest.mark.parametrize("name", ["coverage", "vars17"])
def test_tool_slabs_batches_and_writers_give_one_tree(tmp_path, name):
    c = FC.case(name)
    p = _write_case(c, tmp_path)
    base = ["infile=" + p, "output_level=1", "output_max_grid_size=%d" % c.mgs, "is_per=%d %d %d" % c.is_per]
    outs = {}
    for tag, extra in (("default", []), ("small", ["slab_boxes=1", "comp_batch=1"]), ("odd", ["slab_boxes=3", "comp_batch=5"]), ("whole", ["stream_write=0"])):
        outs[tag] = str(tmp_path / ("flat_" + tag))
        r = _tool(base + ["output_file=" + outs[tag]] + extra, tmp_path)
        assert r.returncode == 0, (tag, r.stdout[-2000:] + r.stderr[-2000:])
    for tag in ("small", "odd", "whole"):
        _same_tree(outs["default"], outs[tag])
    _check_tool_output(c, outs["default"], 1, 1, c.mgs)


def test_tool_moves_an_old_output_away(tmp_path):
    c = FC.case("coverage")
    p = _write_case(c, tmp_path)
    out = str(tmp_path / "flat")
    for _ in range(2):
        r = _tool(["infile=" + p, "output_file=" + out, "output_level=1"], tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
    assert len([q for q in os.listdir(tmp_path) if q.startswith("flat.old.")]) == 1


def _edit_header(path, fn):
    with open(os.path.join(path, "Header")) as f:
        lines = f.read().split("\n")
    fn(lines)
    with open(os.path.join(path, "Header"), "w") as f:
        f.write("\n".join(lines))


def test_tool_aborts_before_anything_is_written(tmp_path):
    c = FC.case("avg_three_files_f0")  # three levels, two variables
    p = _write_case(c, tmp_path)
    n = [0]

    def aborts(args, msg, infile=p):
        n[0] += 1
        out = str(tmp_path / f"o{n[0]}")
        r = _tool(["infile=" + infile, "output_file=" + out] + args, tmp_path)
        assert r.returncode == 134 and msg in r.stderr, (args, r.returncode, r.stderr[-1000:])
        assert not os.path.exists(out), args

    aborts(["output_level=3"], "output_level < pltData.getNlev()")
    aborts(["output_level=-1"], "output_level < pltData.getNlev()")
    aborts(["output_max_grid_size=0"], "output_max_grid_size must be positive")
    aborts(["interp_type=2"], "interp_type must be 0 (piecewise constant) or 1 (cell cons linear)")
    aborts(["ngpus=2"], "ngpus > 1 is not supported")
    aborts(["comp_batch=0"], "comp_batch must be 1 .. 16")
    aborts(["slab_boxes=0"], "slab_boxes must be positive")
    # a 2-D file
    lv = Level(np.array([[0, 0, 0, 15, 15, 0]], dtype=np.int32), (0, 0, 0), (15, 15, 0), (0, 0, 0), np.zeros(3), np.ones(3))
    p2 = str(tmp_path / "plt2d")
    write_plotfile(p2, Hierarchy([lv], 2), [MultiFab(lv, 1, 0)], ["a"], dim=2)
    n[0] += 1
    r = _tool(["infile=" + p2, "output_file=" + str(tmp_path / "o2d")], tmp_path)
    assert r.returncode == 134 and not os.path.exists(tmp_path / "o2d")
    # a ratio other than 2 or 4; ratios that differ between levels (the Header's ratio line)
    ratio_line = 2 + len(c.names) + 5
    p3 = _write_case(c, tmp_path, "plt_ratio3")
    _edit_header(p3, lambda ls: ls.__setitem__(ratio_line, "3 3 "))
    aborts(["output_level=1"], "only refinement ratios 2 and 4 are supported", infile=p3)
    p4 = _write_case(c, tmp_path, "plt_ratio24")
    _edit_header(p4, lambda ls: ls.__setitem__(ratio_line, "2 4 "))
    aborts(["output_level=2"], "levels with different refinement ratios are not supported", infile=p4)
    # an output path that is, or contains, the input
    r = _tool(["infile=" + p, "output_file=" + p], tmp_path)
    assert r.returncode == 134 and "is or contains the input plotfile" in r.stderr
    r = _tool(["infile=" + p, "output_file=" + str(tmp_path)], tmp_path)
    assert r.returncode == 134 and "is or contains the input plotfile" in r.stderr
    assert os.path.exists(os.path.join(p, "Header")) and os.path.exists(os.path.join(p, "Level_2", "Cell_H"))
    # cells without source data: the count, and the partial output is removed
    h = FC.case("hole0")
    ph = _write_case(h, tmp_path, "plt_hole")
    for extra in ([], ["stream_write=0"]):
        aborts(["output_max_grid_size=8"] + extra, "256 cells found no source data", infile=ph)
    assert not [q for q in os.listdir(tmp_path) if ".old." in q]
    # an output directory that exists and is not a plotfile is written into as it is: what else it holds survives the abort, only
    # what the run created is removed
    for k, extra in enumerate(([], ["stream_write=0"], ["slab_boxes=1", "comp_batch=1"])):
        d = tmp_path / f"mine{k}"
        os.makedirs(d / "Level_0")
        os.makedirs(d / "sub")
        for f in ("notes.txt", "Level_0/other.dat", "sub/keep.bin"):
            with open(d / f, "w") as fh:
                fh.write("not the tool's\n")
        r = _tool(["infile=" + ph, "output_file=" + str(d), "output_max_grid_size=8"] + extra, tmp_path)
        assert r.returncode == 134 and "256 cells found no source data" in r.stderr
        left = sorted(os.path.relpath(os.path.join(w, f), d) for w, _, fs in os.walk(d) for f in fs)
        assert left == ["Level_0/other.dat", "notes.txt", "sub/keep.bin"], (extra, left)
        for f in left:
            with open(d / f) as fh:
                assert fh.read() == "not the tool's\n"
