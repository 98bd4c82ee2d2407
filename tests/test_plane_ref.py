"""CPU tier of the plane tools: the dense numpy restatement (tests/plane_ref.py) against known answers, the case matrix's power to
tell the defined order of additions from two plausible wrong ones, and the tools' host side (tools/common/pa_image.h: keys, palette,
PPM / PGM) as a stand-alone program -- also under AddressSanitizer / UBSan."""
import os
import subprocess

import numpy as np
import pytest

import plane_cases as PC
import plane_ref as PR
from peleanalysis_amd.hierarchy import Level, MultiFab
from util import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one_level(n, data):
    """one level of n = (nx, ny, nz) cells in one box holding data [K][nz][ny][nx]"""
    lv = Level(np.array([[0, 0, 0, n[0] - 1, n[1] - 1, n[2] - 1]]), (0, 0, 0), tuple(np.array(n) - 1), (0, 0, 0), np.zeros(3), np.ones(3))
    m = MultiFab(lv, data.shape[0], 0)
    m.valid(0)[...] = data
    return lv, m


# ------------------------------------------------------------------------------------------------ known answers
@pytest.mark.parametrize("name", ["three_levels", "ratio4", "subbox_odd"])
@pytest.mark.parametrize("dir", PC.DIRS)
def test_ones_sum_to_the_thickness(name, dir):
    c = PC.case(name)
    ones = [MultiFab(m.level, 1, 0, fill=1.0) for m in c.mfs]
    sb = c.subbox(dir)
    F, nosrc = PR.composite(c.levels, ones, c.ratios, sb[:3], sb[3:], (0,))
    assert nosrc == 0
    S = PR.plane_sum(F, dir, sb[dir], c.max_grid_size)
    assert np.array_equal(S, np.full(S.shape, float(sb[3 + dir] - sb[dir] + 1)))


def test_hand_computed_chunked_sum():
    """2 x 2 x 4 cells, summed along z in chunks of 2: ((0 + (0 + a + b)) + (0 + c + d)), not (((a + b) + c) + d)"""
    col = np.array([1.0, 1e16, -1e16, 1.0])
    data = np.zeros((1, 4, 2, 2))
    data[0, :, 0, 0] = col
    data[0, :, 1, 1] = [0.1, 0.2, 0.3, 0.4]
    lv, m = _one_level((2, 2, 4), data)
    F, _ = PR.composite([lv], [m], [], (0, 0, 0), (1, 1, 3), (0,))
    S = PR.plane_sum(F, 2, 0, 2)[0]
    assert S[0, 0] == ((0.0 + ((0.0 + 1.0) + 1e16)) + ((0.0 + -1e16) + 1.0)) == 0.0
    assert (((0.0 + 1.0) + 1e16) + -1e16) + 1.0 == 1.0  # what one chunk would give
    assert S[1, 1] == ((0.0 + ((0.0 + 0.1) + 0.2)) + ((0.0 + 0.3) + 0.4))
    assert S[0, 1] == 0.0 and S[1, 0] == 0.0
    assert PR.chunks(0, 15, 6) == [(0, 5), (6, 10), (11, 15)] and PR.chunks(3, 3, 32) == [(3, 3)]


def test_coarse_cells_add_once_per_fine_cell():
    """a coarse cell 2 fine cells wide adds its value twice: (0 + v) + v, and the image axes are (d0, d1) = the two other directions"""
    c = PC.case("uneven_chunks")
    r = PC.reference("uneven_chunks", 0)
    # pixel (j' = 0, k' = 1) of dir 0: the column i = 0 .. 15 at fine (j, k) = (0, 1) lies outside the fine box (4..11): all coarse
    v = c.mfs[0].valid(0)[0, 0, 0, :]  # coarse row k = 0, j = 0
    want, cells = 0.0, [x for x in v for _ in range(2)]
    for a, b in PR.chunks(0, 15, 6):
        s = 0.0
        for p in range(a, b + 1):
            s = s + cells[p]
        want = want + s
    assert r["sum"].shape == (3, 16, 16) and r["sum"][0, 1, 0] == want


def test_minus_zero_sums_to_plus_zero_and_slices_as_it_is():
    for dir in PC.DIRS:
        r = PC.reference("thin", dir)
        F0 = r["F"][0]
        assert np.signbit(F0[F0 == 0.0]).any()
        zero = np.take(F0, 0, axis=2 - dir) == 0.0
        assert zero.any() and not np.signbit(r["sum"][0][zero]).any()
        sl = r["slice"][0]
        assert np.signbit(sl[sl == 0.0]).any()


def test_pixel_levels_of_a_hand_made_plane():
    plane = np.array([[-1.0, 0.0, 0.5, 1.0], [2.0, np.nan, np.inf, 1.0 / 255.0], [0.999999, 254.5 / 255.0, -np.inf, -0.0]])
    lv = PR.pixelize(plane, 0.0, 1.0)
    assert lv.dtype == np.uint8
    assert lv.tolist() == [[0, 0, 127, 255], [255, 0, 255, 1], [254, 254, 0, 0]]
    assert PR.pixelize(plane, 1.0, 1.0).tolist() == [[0, 0, 0, 0], [255, 0, 255, 0], [0, 0, 0, 0]]  # min == max: t = +-inf or NaN
    assert PR.minmax(plane) == (-np.inf, np.inf) and PR.minmax(np.array([[np.nan, 3.0], [-2.0, np.nan]])) == (-2.0, 3.0)
    with pytest.raises(PR.PlaneAbort):
        PR.minmax(np.full((2, 2), np.nan))
    r = PC.reference("nan_inf", 2)
    assert np.isnan(r["sum"][0]).sum() == 1 and np.isposinf(r["sum"][0]).sum() == 1 and r["sum_minmax"][1] == np.inf


def test_image_bytes_against_literals():
    lv = np.array([[0, 1], [2, 255], [7, 7]], dtype=np.uint8)
    assert PR.pgm_bytes(lv) == b"P5\n2 3\n255\n" + bytes([0, 1, 2, 255, 7, 7])
    pal = PR.load_palette(PC.palette_bytes())
    want = b"P6\n2 3\n255\n" + bytes([3, 255, 101, 10, 254, 114, 17, 253, 127, (255 * 7 + 3) % 256, 0, (255 * 13 + 101) % 256, 52, 248, 192, 52, 248, 192])
    assert PR.ppm_bytes(lv, pal) == want
    assert PR.sumfile_bytes(np.array([[[1.0, 2.0]]])) == b"1 1 2\n" + np.array([1.0, 2.0], dtype="<f8").tobytes()


def test_palettes_of_768_and_1024_bytes():
    p3, p4 = PR.load_palette(PC.palette_bytes()), PR.load_palette(PC.palette_bytes(alpha=True))
    assert len(PC.palette_bytes()) == 768 and len(PC.palette_bytes(alpha=True)) == 1024
    assert not p3[3].any() and p4[3][5] == 15 and all(np.array_equal(a, b) for a, b in zip(p3[:3], p4[:3]))
    with pytest.raises(PR.PlaneAbort):
        PR.load_palette(PC.palette_bytes()[:767])


# ------------------------------------------------------------------------------------------------ discrimination
@pytest.mark.parametrize("name", ["single", "uneven_chunks", "ratio4"])
@pytest.mark.parametrize("dir", PC.DIRS)
def test_cases_tell_the_order_of_additions(name, dir):
    """the defined sum differs in some pixel's bits from the sum without chunks and from F_coarse * R in place of R additions"""
    c = PC.case(name)
    r = PC.reference(name, dir)
    sb = c.subbox(dir)
    assert not bits_equal(r["sum"], PR.plane_sum(r["F"], dir, sb[dir], c.max_grid_size, chunked=False))
    if c.ratios:
        R = c.ratios[0]
        # the fine level's value where it has the cell; elsewhere the coarse value times R, once per coarse cell
        one = [MultiFab(m.level, 1, 0, fill=1.0) for m in c.mfs]
        zero_fine = [one[0], MultiFab(c.levels[1], 1, 0, fill=0.0)]
        cmask, _ = PR.composite(c.levels, zero_fine, c.ratios, sb[:3], sb[3:], (0,))  # 1 where level 0 owns the cell
        F = np.array(r["F"])
        idx = np.arange(sb[dir], sb[3 + dir] + 1)
        first = (idx % R == 0).reshape([-1 if a == 2 - dir else 1 for a in range(3)])
        owned = cmask[0] == 1.0
        Fm = np.where(owned[None], np.where(first[None], F * R, 0.0), F)
        assert not bits_equal(r["sum"], PR.plane_sum(Fm, dir, sb[dir], c.max_grid_size))


# ------------------------------------------------------------------------------------------------ the tools' host side
@pytest.fixture(scope="module")
def check_programs(tmp_path_factory):
    """tools/common/pa_image.h as a stand-alone program: a plain build and one under AddressSanitizer + UBSan"""
    d = tmp_path_factory.mktemp("planecheck")
    src = os.path.join(ROOT, "tools", "src", "planeImageCheck.cpp")
    out = {}
    for tag, flags in (("plain", ["-O2"]), ("asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(d / ("planeImageCheck_" + tag))
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + [src, "-o", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[tag] = exe
    return out


def _run(exe, args, cwd):
    return subprocess.run([exe] + args, cwd=cwd, capture_output=True, text=True, timeout=60)


def _fields(stdout):
    return {ln.split(" ", 1)[0]: (ln.split(" ", 1) + [""])[1] for ln in stdout.strip().split("\n")}


FILEKEYS = ["names=a b c", "domains=0 0 0 7 7 7  0 0 0 15 15 15  0 0 0 31 31 31"]


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_host_images(check_programs, build, tmp_path):
    exe = check_programs[build]
    rng = np.random.default_rng(5)
    lv = rng.integers(0, 256, size=(7, 5), dtype=np.uint8)
    lv[0, :2] = (0, 255)
    (tmp_path / "lv.bin").write_bytes(lv.tobytes())
    for alpha in (False, True):
        (tmp_path / "pal").write_bytes(PC.palette_bytes(alpha))
        (tmp_path / "o.ppm").write_bytes(b"an older and much longer file" * 100)  # overwritten, as fopen("w") does
        r = _run(exe, ["check=image", "type=image", "width=5", "height=7", "levels=lv.bin", "palette=pal", "out=o.ppm"], tmp_path)
        assert r.returncode == 0 and r.stderr == "", r.stderr
        assert r.stdout == ("alpha 0 %d\n" % ((255 * 3) % 256) if alpha else "alpha 0 0\n")
        assert (tmp_path / "o.ppm").read_bytes() == PR.ppm_bytes(lv, PR.load_palette(PC.palette_bytes(alpha)))
    r = _run(exe, ["check=image", "type=gray", "width=5", "height=7", "levels=lv.bin", "out=o.pgm"], tmp_path)
    assert r.returncode == 0 and r.stderr == "" and (tmp_path / "o.pgm").read_bytes() == PR.pgm_bytes(lv)
    (tmp_path / "short").write_bytes(PC.palette_bytes()[:767])
    r = _run(exe, ["check=image", "type=image", "width=5", "height=7", "levels=lv.bin", "palette=short", "out=o2.ppm"], tmp_path)
    assert r.returncode == 134 and "shorter than 768 bytes" in r.stderr and not (tmp_path / "o2.ppm").exists()


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_host_keys_of_avgtoplane(check_programs, build, tmp_path):
    exe = check_programs[build]
    (tmp_path / "pal").write_bytes(PC.palette_bytes())
    base = ["check=avgtoplane"] + FILEKEYS + ["infile=/some/where/plt00120/", "palette=pal"]
    r = _run(exe, base, tmp_path)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    f = _fields(r.stdout)
    assert f == {"comps": "0 1 2", "finestLevel": "2", "dir": "0", "max_grid_size": "32", "box": "0 0 0 31 31 31", "min": "0 0", "max": "0 0",
                 "outfile": "plt00120.ppm", "sumfile": ""}
    r = _run(exe, base + ["comps=2 0", "finestLevel=1", "box=1 3 5 9 11 15", "dir=2", "max_grid_size=5", "min=-1.5", "max=1e3", "sumfile=s.bin"], tmp_path)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    f = _fields(r.stdout)
    assert f == {"comps": "2 0", "finestLevel": "1", "dir": "2", "max_grid_size": "5", "box": "1 3 5 9 11 15", "min": "1 -1.5", "max": "1 1000",
                 "outfile": "plt00120.ppm", "sumfile": "s.bin"}
    assert _fields(_run(exe, base + ["sComp=1", "nComp=2"], tmp_path).stdout)["comps"] == "1 2"
    for bad, msg in ((["dir=3"], "dir must be 0, 1 or 2"), (["dir=-1"], "dir must be"), (["finestLevel=3"], "finestLevel out of range"),
                     (["comps=0 3"], "component 3 is not in the plotfile"), (["sComp=2", "nComp=2"], "component 3 is not"),
                     (["finestLevel=1", "box=0 0 0 16 15 15"], "not inside the domain of level 1"), (["box=0 0 0 7 7"], "six integers"),
                     (["box=5 0 0 4 7 7"], "box is empty"), (["max_grid_size=0"], "max_grid_size must be"), (["palette=nosuch"], "cannot open palette file")):
        r = _run(exe, base + bad, tmp_path)
        assert r.returncode == 134 and msg in r.stderr, (bad, r.returncode, r.stderr)
    r = _run(exe, [a for a in base if not a.startswith("palette=")], tmp_path)
    assert r.returncode == 134 and "palette not found" in r.stderr


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_host_keys_of_sliceplot(check_programs, build, tmp_path):
    exe = check_programs[build]
    (tmp_path / "pal").write_bytes(PC.palette_bytes(alpha=True))
    base = ["check=sliceplot"] + FILEKEYS + ["file=run/plt7", "slicedir=1", "sliceloc=20", "varname=b"]
    r = _run(exe, base + ["palette=pal"], tmp_path)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert _fields(r.stdout) == {"comp": "1", "finestLevel": "2", "slicedir": "1", "sliceloc": "20", "box": "0 20 0 31 20 31", "outtype": "image", "writes": "1",
                                 "min": "0 0", "max": "0 0", "outfile": "plt7.ppm"}
    r = _run(exe, base + ["outtype=gray", "min=0.25", "outfile=x/y.pgm", "finestLevel=1", "sliceloc=15"], tmp_path)  # gray needs no palette
    assert r.returncode == 0 and r.stderr == "", r.stderr
    f = _fields(r.stdout)
    assert f["outtype"] == "gray" and f["writes"] == "1" and f["min"] == "1 0.25" and f["outfile"] == "x/y.pgm" and f["box"] == "0 15 0 15 15 15"
    assert _fields(_run(exe, base + ["outtype=gray"], tmp_path).stdout)["outfile"] == "plt7.pgm"
    f = _fields(_run(exe, base + ["outtype=fab"], tmp_path).stdout)
    assert f["writes"] == "0"
    for bad, msg in ((["slicedir=3"], "slicedir must be"), (["sliceloc=32"], "sliceloc is outside the domain of level 2"), (["sliceloc=-1"], "sliceloc is outside"),
                     (["finestLevel=0", "sliceloc=8"], "outside the domain of level 0"), (["varname=density"], "is not a variable of the plotfile"),
                     (["finestLevel=-1"], "finestLevel out of range")):
        r = _run(exe, base + ["palette=pal"] + bad, tmp_path)
        assert r.returncode == 134 and msg in r.stderr, (bad, r.returncode, r.stderr)
    r = _run(exe, base, tmp_path)  # image without a palette
    assert r.returncode == 134 and "palette not found" in r.stderr
    r = _run(exe, [a for a in base if not a.startswith("sliceloc=")] + ["palette=pal"], tmp_path)
    assert r.returncode == 134 and "sliceloc not found" in r.stderr
