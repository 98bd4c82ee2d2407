"""CPU tier of the plotfile average: the numpy restatement (tests/avgplt_ref.py) is pinned to the oracle the filter's ghost fill
is held to, has the properties the semantics promise, and the tool's host grid builder (tools/common/pa_avggrids.h) gives a
disjoint cover of the union -- also under AddressSanitizer / UBSan, as a stand-alone program."""
import os
import subprocess

import numpy as np
import pytest

import avgplt_cases as AC
import avgplt_ref as AR
from peleanalysis_amd.hierarchy import Level, MultiFab, chop_box, field_flame, field_trig, fill_analytic
from util import SENT_REF, bits_equal, sentinel_mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _level(boxes, n, is_per):
    return Level(boxes, (0, 0, 0), (n - 1,) * 3, is_per, np.zeros(3), np.ones(3))


@pytest.mark.parametrize("is_per", [(0, 0, 0), (1, 1, 0), (0, 1, 1)])
@pytest.mark.parametrize("interp_type", [0, 1])
@pytest.mark.parametrize("ratio", [2, 4])
def test_interpolation_is_the_oracles_fillpatch(oracle, ratio, interp_type, is_per):
    """the coarse-fine ghost cells FillPatchTwoLevels fills around small fine boxes -- on both walls, through a periodic face and
    inside the domain -- hold the bits of the dense interpolant"""
    nc, ng = 16, 3
    nf = nc * ratio
    crse_lv = _level(chop_box((0, 0, 0), (nc - 1,) * 3, 8), nc, is_per)
    s = ratio * 2  # fine boxes of two coarse cells per side and one slab on each wall / face
    fboxes = np.array([[0, 0, 0, s - 1, 2 * s - 1, s - 1], [nf - s, nf - 2 * s, nf - s, nf - 1, nf - 1, nf - 1],
                       [3 * s, 3 * s, 3 * s, 4 * s - 1, 4 * s - 1, 5 * s - 1], [4 * s, 3 * s, 3 * s, 5 * s - 1, 4 * s - 1, 4 * s - 1],
                       [0, 5 * s, 2 * s, s - 1, 6 * s - 1, 3 * s - 1]], dtype=np.int32)
    fine_lv = _level(fboxes, nf, is_per)
    crse = MultiFab(crse_lv, 2, 0)
    fill_analytic(crse, 0, lambda x, y, z: field_flame(x, y, z, 1))
    fill_analytic(crse, 1, lambda x, y, z: field_trig(x, y, z, 2))
    fine = sentinel_mf(fine_lv, 2, ng, SENT_REF)
    assert oracle.fillpatch_two_levels(fine, crse, 0, 2, ng, ratio, interp_type) == 0
    occ = AR.occupancy(fboxes, (nf,) * 3)
    checked = 0
    for c in range(2):
        dense = AR.interp_dense(AR.dense_of(crse, c, (nc,) * 3), ratio, is_per, interp_type)
        for b in range(fine_lv.nboxes):
            lo = fboxes[b, :3] - ng
            f = fine.fab(b)[c]
            idx = [np.arange(lo[d], lo[d] + f.shape[2 - d]) for d in range(3)]
            inside = [(i >= 0) & (i < nf) | bool(is_per[d]) for d, i in enumerate(idx)]
            w = [i % nf for i in idx]
            cf = ~occ[np.ix_(w[2], w[1], w[0])] & inside[2][:, None, None] & inside[1][None, :, None] & inside[0][None, None, :]
            assert bits_equal(f[cf], dense[np.ix_(w[2], w[1], w[0])][cf]), (ratio, interp_type, is_per, c, b)
            assert (f.view(np.uint64)[~cf] == np.uint64(SENT_REF)).all()  # the oracle fills the coarse-fine cells and nothing else
            checked += int(cf.sum())
    assert checked > 2000


@pytest.mark.parametrize("interp_type", AC.INTERP_TYPES)
def test_one_file_returns_its_own_bits(interp_type):
    c = AC.case("one_file")
    avg, masks = AC.reference("one_file", interp_type)
    for l in range(c.nlev):
        n = AC.N0 * c.ratio ** l
        for v, fc in enumerate(c.comps[0]):
            own = AR.dense_of(c.mfs[0][l], fc, (n,) * 3)
            m = masks[l]
            assert m.any() and not np.isnan(own[m]).any()
            assert bits_equal(avg[l][v][m], own[m])


@pytest.mark.parametrize("interp_type", AC.INTERP_TYPES)
def test_constant_field_stays_constant(interp_type):
    c = AC.case("same_level1")  # two files: the factor 1.0 / 2 is exact
    const = 1234.5678
    files = []
    for mfs in c.mfs:
        files.append([MultiFab(m.level, m.ncomp, 0, fill=const) for m in mfs])
    for f in files:
        for V in AR.file_levels_dense(f, [0, 1], c.nlev, AC.N0, c.ratio, c.is_per, interp_type):
            assert (V == const).all()
    avg, _ = AR.average(files, c.comps, c.nlev, AC.N0, c.ratio, c.is_per, interp_type)
    for a in avg:
        assert (a == const).all()


@pytest.mark.parametrize("ratio,is_per", [(2, (1, 1, 0)), (4, (0, 0, 1))])
def test_linear_interpolation_conserves(ratio, is_per):
    """the mean of a parent's children is the parent.  A child is ((u0 + t0) + t1) + t2 with t_d = xoff_d * (s_d * alpha); the child
    offsets are symmetric about the parent's centre, so the products t_d of the r^3 children cancel exactly in their sum, and what is
    left are the roundings of the three additions per child: each at most 2^-53 times its result, and every partial sum is at most
    |u0| + sum |t_d| <= |u0| + dumax * alpha <= |u0| + min(umax - u0, u0 - umin) <= 3 max|u| (the limiter; the roundings of alpha
    and of the products change that by a factor 1 + O(2^-52)).  So |mean - u0| <= 3 * 3 * 2^-53 * max|u| (1 + O(2^-52)); with the
    2^-64 rounding of the extended-precision mean taken here: k = 10."""
    n = 16
    lv = _level(chop_box((0, 0, 0), (n - 1,) * 3, 8), n, is_per)
    m = MultiFab(lv, 2, 0)
    fill_analytic(m, 0, lambda x, y, z: field_flame(x, y, z, 0))
    fill_analytic(m, 1, lambda x, y, z: field_trig(x, y, z, 1))
    for comp in range(2):
        u = AR.dense_of(m, comp, (n,) * 3)
        fine = AR.interp_dense(u, ratio, is_per, 1)
        assert not bits_equal(fine, AR.interp_dense(u, ratio, is_per, 0))  # slopes are at work
        mean = fine.astype(np.longdouble).reshape(n, ratio, n, ratio, n, ratio).sum(axis=(1, 3, 5)) / np.longdouble(ratio ** 3)
        err = float(np.abs(mean - u.astype(np.longdouble)).max())
        bound = 10 * 2.0 ** -53 * float(np.abs(u).max())
        print(f"ratio {ratio} comp {comp}: |mean - parent| max {err:.3e}, bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("name", AC.CASES)
def test_union_masks_and_python_cover(name):
    c = AC.case(name)
    _, masks = AC.reference(name, 1)
    assert len(masks) == c.nlev
    for l in range(c.nlev):
        n = AC.N0 * c.ratio ** l
        count = np.zeros((n,) * 3, dtype=np.int32)
        for boxes in c.level_box_lists(l):
            for lo0, lo1, lo2, hi0, hi1, hi2 in boxes:
                count[lo2:hi2 + 1, lo1:hi1 + 1, lo0:hi0 + 1] += 1
        assert np.array_equal(masks[l], count > 0)
        ob = c.out_boxes(l).astype(np.int64)
        assert int(np.prod(ob[:, 3:] - ob[:, :3] + 1, axis=1).sum()) == int(masks[l].sum())  # disjoint ...
        assert np.array_equal(AR.occupancy(ob, (n,) * 3), masks[l])                            # ... and a cover
    assert masks[0].all()  # level 0 covers the domain
    for l in range(1, c.nlev):  # the output levels are nested
        r, nc = c.ratio, masks[l - 1].shape[0]
        assert masks[l - 1][masks[l].reshape(nc, r, nc, r, nc, r).any(axis=(1, 3, 5))].all()


@pytest.fixture(scope="module")
def grid_programs(tmp_path_factory):
    """the grid builder as a stand-alone program: a plain build and one under AddressSanitizer + UBSan"""
    d = tmp_path_factory.mktemp("avggrids")
    src = os.path.join(ROOT, "tools", "src", "avgGridsCheck.cpp")
    out = {}
    for tag, flags in (("plain", ["-O2"]), ("asan", ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])):
        exe = str(d / ("avgGridsCheck_" + tag))
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + flags + [src, "-o", exe], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[tag] = exe
    return out


def _run_grids(exe, lists, mgs):
    text = "%d %d\n" % (mgs, len(lists))
    for b in lists:
        text += "%d\n" % len(b) + "".join(" ".join(str(int(x)) for x in row) + "\n" for row in b)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stderr[-2000:])
    lines = r.stdout.split("\n")
    same = int(lines[0].split()[1])
    n = int(lines[1])
    boxes = np.array([[int(x) for x in ln.split()] for ln in lines[2:2 + n]], dtype=np.int64).reshape(-1, 6)
    return same, boxes


@pytest.mark.parametrize("build", ["plain", "asan"])
def test_host_grid_builder(grid_programs, build):
    seen_same = seen_union = 0
    for name in AC.CASES:
        c = AC.case(name)
        _, masks = AC.reference(name, 1)
        for l in range(c.nlev):
            lists = c.level_box_lists(l)
            for mgs in (c.max_grid_size, 32, 5):
                same, boxes = _run_grids(grid_programs[build], lists, mgs)
                n = AC.N0 * c.ratio ** l
                if same:  # every file holds this list: unchanged, whatever the grid size
                    assert all(np.array_equal(b, lists[0]) for b in lists) and np.array_equal(boxes, lists[0])
                    seen_same += 1
                else:
                    assert not all(len(b) == len(lists[0]) and np.array_equal(b, lists[0]) for b in lists)
                    assert (boxes[:, 3:] - boxes[:, :3] + 1).max() <= mgs
                    seen_union += 1
                assert (boxes[:, 3:] >= boxes[:, :3]).all()
                assert int(np.prod(boxes[:, 3:] - boxes[:, :3] + 1, axis=1).sum()) == int(masks[l].sum()), (name, l, mgs)  # disjoint
                assert np.array_equal(AR.occupancy(boxes, (n,) * 3), masks[l]), (name, l, mgs)                          # cover = union
    assert seen_same >= 3 and seen_union >= 6
