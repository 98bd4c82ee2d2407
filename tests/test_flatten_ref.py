"""CPU tier of flattenAMRFile3d: the dense reference against the average's, the reason the tool is not a one-file average, the
case matrix's own claims, the host side of the tool as a stand-alone program (plain and under AddressSanitizer + UBSan), and the
new symbols of the ABI."""
import filecmp
import os
import re
import subprocess

import numpy as np
import pytest

import avgplt_cases as AC
import avgplt_ref as AR
import flatten_cases as FC
import flatten_ref as FR
from peleanalysis_amd import capi
from util import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("interp_type", FC.INTERP_TYPES)
@pytest.mark.parametrize("name", [n for n in FC.CASES if n.startswith("avg_")])
def test_reference_equals_the_averages_on_cubes(name, interp_type):
    c = FC.case(name)
    V, _ = FC.reference(name, interp_type)
    want = AR.file_levels_dense(c.mfs, c.comps, c.nlev, AC.N0, c.ratio, c.is_per, interp_type)
    assert len(V) == c.nlev
    for l in range(c.nlev):
        assert V[l].shape == want[l].shape and bits_equal(V[l], want[l]), (name, l)
        got, nosrc = FR.flatten(c.mfs, c.comps, l, c.n0, c.ratio, c.is_per, interp_type)
        assert nosrc == 0 and bits_equal(got, V[l])  # levels finer than the output level are ignored


def test_a_one_file_average_loses_the_sign_of_zero():
    """0.0 + (-0.0) = +0.0: the running sum of avgPlotfiles does not return the file's own bits, flatten does"""
    c = FC.case("rawbits")
    V, _ = FC.reference("rawbits", 1)
    flat = V[1]
    avg = (np.zeros_like(flat) + flat) * (1.0 / 1.0)
    u, a = flat.view(np.uint64), avg.view(np.uint64)
    assert int((u == FC.NEG_ZERO).sum()) == 4 and int((u == FC.NAN_PAYLOAD).sum()) == 4  # two cells, two variables each
    assert int((a == FC.NEG_ZERO).sum()) == 0
    differ = u != a
    assert differ.any() and (u[differ] == FC.NEG_ZERO).all()  # nothing else differs: a NaN's payload survives an addition of 0.0
    # and the cells are the file's own, on the output level
    m = c.mfs[1]
    assert m.valid(0)[0].view(np.uint64)[3, 5, 7] == FC.NEG_ZERO and u[0, 3, 5, 7] == FC.NEG_ZERO


@pytest.mark.parametrize("name", FC.CASES)
def test_case_claims(name):
    c = FC.case(name)
    for l in c.outs:
        lo, hi = c.domain(l)
        assert int(np.prod(np.array(hi) + 1)) <= 420000
        ob = c.out_boxes(l).astype(np.int64)
        assert int(np.prod(ob[:, 3:] - ob[:, :3] + 1, axis=1).sum()) == int(np.prod(np.array(hi) + 1))  # a partition of the domain
        wide, general, skipped, rects = c.expected_launch(l)
        assert wide + general + skipped == len(ob)
        if l == 0 or c.general_only:
            assert (wide, skipped, rects) == (0, 0, 0)
    if c.general_only:
        ob = c.out_boxes(1)
        assert ((ob[:, 3] - ob[:, 0] + 1) % 2 == 1).all() and (ob[:, 0] % 2 != 0).any()  # odd widths, boxes off the parents' edges
    if c.nlev > 1 and name != "hole0":
        # the limiter: the data reach parents with alpha < 1 and parents with a zero slope
        _, keep = FC.reference(name, 1)
        assert keep
        assert any((k["alpha"] < 1.0).any() for k in keep), name
        assert any(((k["sl"][0] == 0.0) | (k["sl"][1] == 0.0) | (k["sl"][2] == 0.0)).any() for k in keep), name
        V0, _ = FC.reference(name, 0)
        V1, _ = FC.reference(name, 1)
        assert not bits_equal(V0[1], V1[1])


def test_matrix_holds_what_it_promises():
    e = FC.case("wide80_r2").expected_launch(1)
    assert FC.case("wide80_r2").out_boxes(1).shape[0] == 1 and e[0] == 1 and e[3] >= 1    # one box, 80 parents in x
    assert FC.case("wide40_r4").out_boxes(1).shape[0] == 1
    wide, general, skipped, rects = FC.case("mixed_routes").expected_launch(1)
    assert wide > 0 and general > 0
    ob = FC.case("mixed_routes").out_boxes(1)
    assert ((ob[:, 1] % 2 != 0) & (ob[:, 0] % 2 == 0) & ((ob[:, 3] - ob[:, 0]) % 2 == 1)).any()  # a wide box that starts inside a parent in y
    wide, general, skipped, rects = FC.case("coverage").expected_launch(1)
    assert skipped == 8 and general == 0 and wide == 56 and rects > skipped + 1
    assert FC.case("coverage_r4").expected_launch(1)[2] >= 2
    assert len(FC.case("vars17").names) == 17
    c = FC.case("hole0")
    V, nosrc = FR.flatten(c.mfs, c.comps, 0, c.n0, c.ratio, c.is_per, 1)
    assert nosrc == 8 * 8 * 4 and int(np.isnan(V[0]).sum()) == nosrc
    pers = {FC.case(n).is_per for n in FC.CASES}
    for d in range(3):  # periodic and wall faces in every direction
        assert {p[d] for p in pers} == {0, 1}


# ------------------------------------------------------------------------------------------------ the host side of the tool
@pytest.fixture(scope="module")
def plan_programs(tmp_path_factory):
    """tools/src/flattenPlanCheck.cpp: a plain build and one under AddressSanitizer + UBSan (stand-alone programs, run directly)"""
    d = tmp_path_factory.mktemp("flattenplan")
    src = os.path.join(ROOT, "tools", "src", "flattenPlanCheck.cpp")
    libdir = os.path.join(ROOT, "peleanalysis_amd")
    out = {}
    for tag, flags in (("plain", ["-O2"]), ("asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(d / ("flattenPlanCheck_" + tag))
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-I" + ROOT] + flags + [src, "-o", exe, "-L" + libdir, "-lpeleanalysis_amd",
                            "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        out[tag] = exe
    return out


def _rows(boxes):
    return "%d\n" % len(boxes) + "".join(" ".join(str(int(x)) for x in row) + "\n" for row in boxes)


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_slabs_and_rectangles(plan_programs, build):
    seen = 0
    for name in ("coverage", "coverage_r4", "mixed_routes", "avg_thin_f0", "wide80_r2", "offalign3"):
        c = FC.case(name)
        l = c.nlev - 1
        fb, ob = c.hier.levels[l].boxes, c.out_boxes(l)
        shape = FR.level_shape(c.n0, c.ratio, l)
        for slab_boxes in (1, 3, len(ob), len(ob) + 5):
            r = subprocess.run([plan_programs[build], "rects"], input="%d\n" % slab_boxes + _rows(fb) + _rows(ob), capture_output=True, text=True, timeout=120)
            assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
            lines = r.stdout.split("\n")
            at, i = 0, 0
            count = np.zeros(shape, dtype=np.int32)
            while i < len(lines) and lines[i]:
                w = lines[i].split()
                assert w[0] == "slab"
                b0, b1, nrect, nfb = (int(x) for x in w[1:])
                assert b0 == at and b0 < b1 <= min(len(ob), b0 + slab_boxes)  # the slabs partition the boxes in order
                at = b1
                used = set()
                for ln in lines[i + 1:i + 1 + nrect]:
                    f, o, lo0, lo1, lo2, hi0, hi1, hi2 = (int(x) for x in ln.split())
                    assert b0 <= o < b1
                    assert (np.array([lo0, lo1, lo2]) >= np.maximum(fb[f, :3], ob[o, :3])).all() and (np.array([hi0, hi1, hi2]) <= np.minimum(fb[f, 3:], ob[o, 3:])).all()
                    count[lo2:hi2 + 1, lo1:hi1 + 1, lo0:hi0 + 1] += 1
                    used.add(f)
                assert nfb == len(used)
                i += 1 + nrect
                seen += nrect
            assert at == len(ob)
            # the rectangles tile (file n slabs) exactly: every cell of the file's boxes once, no other cell
            assert np.array_equal(count, AR.occupancy(fb, shape).astype(np.int32)), (name, slab_boxes)
    assert seen > 100


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_streaming_writer_is_byte_identical(plan_programs, build, tmp_path):
    for k, spec in enumerate(("20 12 9 5 3 7", "16 16 16 8 1 1", "33 7 5 64 17 3")):
        d = tmp_path / f"w{k}"
        r = subprocess.run([plan_programs[build], "write", str(d)], input=spec + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
        assert re.fullmatch(r"ok \d+ \d+\n", r.stdout)
        for o in range(4):  # the program compared them itself; once more from outside
            for f in ("Header", "Level_0/Cell_H", "Level_0/Cell_D_00000"):
                assert filecmp.cmp(d / "ref" / f, d / f"s{o}" / f, shallow=False), (spec, o, f)
        assert int(r.stdout.split()[2]) == os.path.getsize(d / "ref" / "Level_0" / "Cell_D_00000")


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "peleanalysis_amd.h")).read()
    lib = capi.load_library()
    for sym in ("pa_flatten_level", "pa_flatten_last_launch"):
        assert re.search(r"\b" + sym + r"\(", header), sym
        assert sym in capi.declared_symbols() and hasattr(lib, sym)
    assert hasattr(capi, "Flatten") and callable(capi.Flatten.level) and callable(capi.Flatten.last_launch)
    assert "flattenAMRFile" in open(os.path.join(ROOT, "tools", "Makefile")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "src", "flattenAMRFile.cpp"))
