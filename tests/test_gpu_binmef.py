"""GPU tier: the surface-PDF kernels (peleanalysis_amd/csrc/pa_binmef.hip) through the C ABI, and binMEF3d.ex end to end, against the
restatement of binMEF.cpp (tests/binmef_ref.py).  The kernels must produce the restatement's leaves -- the same (bin, area) pairs, the
area bits identical, in any order -- so EVERY bin is compared with ==: the hit count with the restatement's, the area with math.fsum of
the bin's terms.  Equality rests on the design: a term of at least 2^-104 of the magnitude declared at begin converts to fixed point
exactly, integer sums are exact and the read rounds once to nearest even, as fsum does; the precondition is asserted on the inputs.
The same input must give the same BITS on every run, for shuffled elements, for the uncombined kernel and for a work list so small that
it is worked off in slices."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import binmef_ref as B
import stats_ref as R
from peleanalysis_amd import capi
from peleanalysis_amd.hierarchy import field_flame, nested_hierarchy
from peleanalysis_amd.plotfile import read_mef, write_plotfile
from util import make_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
SMALL_LIST = 2048  # work_items for n4_128: its list peaks above 20 000 items when it may
# a two-component case whose FIRST round does not fit (576 elements enter 250 at a time and fan out at once): items that still have a
# whole component to clip sit on a nearly full list, which is where a slice rule without a reserve gets stuck
SLICED2 = ("n12_32x32", 1000)
NAMED = ["n8_16x16", "n24_32x8", "n4_128", "n6_8x8x8", "onebin", "allout"]


@functools.lru_cache(maxsize=None)
def surface(n):
    nodes, elts = B.latlong_sphere(n)
    nodes.setflags(write=False)
    elts.setflags(write=False)
    return nodes, elts


@functools.lru_cache(maxsize=None)
def reference(name, cond=None):
    """the restatement of a case, computed once and shared; cond = (condComp, condVal, condSgn)"""
    n, bc, mn, mx, nb = B.CASES[name]
    nodes, elts = surface(n)
    kw = dict(cond_apply=True, cond_comp=cond[0], cond_val=cond[1], cond_sgn=cond[2]) if cond else {}
    return B.bin_surface(nodes, elts, bc, mn, mx, nb, **kw)


def gpu_bin(ctx, name, cond=None, elts=None, uncombined=False, work_items=0):
    n, bc, mn, mx, nb = B.CASES[name]
    nodes, e = surface(n)
    e = e if elts is None else elts
    with capi.SurfBin(ctx, nb, mn, mx, work_items=work_items) as sb:
        sb.begin(sb.max_area(nodes, e))
        if cond:
            sb.add_surface(nodes, e, bc, cond_apply=True, cond_comp=cond[0], cond_val=cond[1], cond_sgn=cond[2], uncombined=uncombined)
        else:
            sb.add_surface(nodes, e, bc, uncombined=uncombined)
        return sb.read()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.int64), np.asarray(b, dtype=np.float64).view(np.int64))


def check(got, ref, what):
    """every bin: hits == the restatement's, area == fsum of its terms (and inside the contract's bound); the three totals exact"""
    area, hits, tot, outside, cnt = got
    nt = int(np.prod(ref.nbins, dtype=np.int64))
    want_area, want_hits = ref.table()
    terms = ref.areas + ref.outside + ref.elem_areas
    mag = max(ref.elem_areas)
    # the precondition of ==: every term is at least 2^-104 of the declared magnitude (frexp: mag < 2^k), so none is truncated
    k = math.frexp(mag)[1]
    assert all(t == 0.0 or t >= 2.0 ** (k - 104) for t in terms), what
    assert np.array_equal(hits, want_hits), (what, int(np.sum(hits != want_hits)))
    assert same_bits(area, want_area), (what, int(np.sum(area != want_area)))
    R.assert_sum_bound(area, np.asarray(ref.keys, dtype=np.int64), np.asarray(ref.areas), nt, what)
    assert tot == math.fsum(ref.elem_areas), what
    assert outside == math.fsum(ref.outside), what
    assert cnt["n_my"] == ref.n_my and cnt["nonfinite"] == ref.nonfinite and cnt["elements"] == len(ref.elem_areas) + ref.nonfinite, (what, cnt)


@pytest.mark.parametrize("name", NAMED)
def test_bins_equal_restatement(ctx, name):
    ref = reference(name)
    got = gpu_bin(ctx, name)
    check(got, ref, name)
    if name == "onebin":  # the 2n pole triangles have no area: 240 leaves from 256 elements, all in one bin
        assert got[1].tolist() == [240]
    if name == "allout":
        assert got[4]["n_my"] == 0 and not got[1].any() and not got[0].any()
    if name == "n4_128":
        assert got[4]["sliced"] == 0 and got[4]["peak"] > 4 * SMALL_LIST


@pytest.mark.parametrize("name", NAMED)
def test_same_bits_for_every_order(ctx, name):
    """two runs, shuffled elements, one set of atomics per leaf: identical bits in every bin and total"""
    n = B.CASES[name][0]
    base = gpu_bin(ctx, name)
    again = gpu_bin(ctx, name)
    e = surface(n)[1]
    shuffled = gpu_bin(ctx, name, elts=e[np.random.default_rng(11).permutation(len(e))])
    plain = gpu_bin(ctx, name, uncombined=True)
    for other, what in ((again, "second run"), (shuffled, "shuffled elements"), (plain, "uncombined")):
        assert same_bits(base[0], other[0]) and np.array_equal(base[1], other[1]), (name, what)
        assert same_bits([base[2], base[3]], [other[2], other[3]]) and base[4]["n_my"] == other[4]["n_my"], (name, what)
    check(plain, reference(name), name + " uncombined")


def test_small_work_list_is_sliced(ctx):
    """n4_128 with a list of 2048 items: the rounds can take only the top of the list, many times over -- the host run of the same
    rounds (tools/bench/binmef_host.hip) takes 293 rounds, 290 of them sliced, for the 26 782 work items; at least items / capacity
    rounds are needed in any case -- the list never holds more than its capacity, and every bin has the bits of the run with the
    default list"""
    ref = reference("n4_128")
    big = gpu_bin(ctx, "n4_128")
    small = gpu_bin(ctx, "n4_128", work_items=SMALL_LIST)
    c = small[4]
    assert c["sliced"] >= 100 and c["rounds"] > c["items"] // SMALL_LIST and c["rounds"] > big[4]["rounds"], c
    assert c["peak"] <= SMALL_LIST == c["capacity"] and c["items"] == big[4]["items"]
    check(small, ref, "n4_128 sliced")
    assert same_bits(big[0], small[0]) and np.array_equal(big[1], small[1]) and same_bits(big[2], small[2])
    # a list that cannot hold the children of one work item fails loudly, and says what would suffice
    with pytest.raises(capi.PaError, match="work_items = 8 cannot hold .* suffices"):
        gpu_bin(ctx, "n4_128", work_items=8)


def test_two_components_sliced_from_the_first_round(ctx):
    """n12 at 32 x 32 with a list of 1000 items: the elements enter in chunks and the first round of every chunk already has to be
    sliced, with items on top that have both components still to clip.  The slice rule keeps r^2 entries free above an item with r
    splits left on its paths, so the top item can always be taken: the call succeeds, within the capacity, with the restatement's
    bins and the bits of the default list."""
    name, cap = SLICED2
    ref = reference(name)
    small = gpu_bin(ctx, name, work_items=cap)
    c = small[4]
    assert c["sliced"] >= 100 and c["peak"] <= cap == c["capacity"] and c["rounds"] > c["items"] // cap, c
    check(small, ref, name + " sliced")
    big = gpu_bin(ctx, name)
    assert big[4]["sliced"] == 0 and big[4]["peak"] > 4 * cap and big[4]["items"] == c["items"]
    assert same_bits(big[0], small[0]) and np.array_equal(big[1], small[1]) and same_bits([big[2], big[3]], [small[2], small[3]])
    for tight in (300, 400):  # capacities that are a small multiple of one item's children
        t = gpu_bin(ctx, name, work_items=tight)
        assert same_bits(big[0], t[0]) and np.array_equal(big[1], t[1]) and t[4]["peak"] <= tight


@pytest.mark.parametrize("sgn", [-1, 0, 1])
def test_condition(ctx, sgn):
    cond = (2, 0.1, sgn)  # z against 0.1
    ref = reference("n8_16x16", cond)
    got = gpu_bin(ctx, "n8_16x16", cond=cond)
    check(got, ref, f"condSgn {sgn}")
    assert len(ref.outside) > 0 and (len(ref.areas) > 0) == (sgn != 0)
    assert same_bits(got[0], gpu_bin(ctx, "n8_16x16", cond=cond, uncombined=True)[0])


def test_nonfinite_elements_are_skipped_and_counted(ctx):
    n, bc, mn, mx, nb = B.CASES["n8_16x16"]
    nodes = surface(n)[0].copy()
    nodes[40, 3] = np.nan
    nodes[90, 1] = np.inf
    e = surface(n)[1]
    ref = B.bin_surface(nodes, e, bc, mn, mx, nb)
    with capi.SurfBin(ctx, nb, mn, mx) as sb:
        sb.begin(sb.max_area(nodes, e))
        sb.add_surface(nodes, e, bc)
        got = sb.read()
    assert ref.nonfinite > 0
    check(got, ref, "nonfinite")


def _tool(args, cwd):
    out = subprocess.run([os.path.join(BIN, "binMEF3d.ex")] + args, cwd=cwd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out


def _tool_args(f, bc, mn, mx, nb):
    j = lambda v: " ".join(repr(x) if isinstance(x, float) else str(x) for x in v)
    return ["infile=" + f, "binComps=" + j(bc), "binMin=" + j(mn), "binMax=" + j(mx), "nBins=" + j(nb)]


@pytest.mark.parametrize("name", NAMED)
def test_tool_end_to_end(tmp_path, name):
    """binMEF3d.ex on the case's MEF: stdout is the restatement's, character for character; with dumpFab=1 normalize=1 so are the
    bytes of the .fab, for one component (n4_128) and for two (allout has no bin to normalise by: 1 / 0)"""
    n, bc, mn, mx, nb = B.CASES[name]
    nodes, elts = surface(n)
    ref = reference(name)
    f = str(tmp_path / "s.mef")
    with open(f, "wb") as fh:
        fh.write(B.mef_bytes(nodes, elts))
    area, hits = ref.table()
    total = math.fsum(ref.elem_areas)
    want, err, _, _ = B.tool_output(area, hits, bc, mn, mx, nb, total, dump_bins=True)
    out = _tool(_tool_args(f, bc, mn, mx, nb) + ["dumpBins=1"], tmp_path)
    assert out.stdout == want
    lines = out.stderr.split("\n")
    assert lines[:4] == ["...finished reading data header", "...%d nodes read from data file (nComp=5)" % len(nodes),
                         "...%d elements read from data file" % len(elts), "...finished reading data"]
    assert lines[4:4 + len(err)] == err
    if len(nb) <= 2 and name != "allout":
        _, _, fab, _ = B.tool_output(area, hits, bc, mn, mx, nb, total, dump_fab=True, normalize=True)
        out = _tool(_tool_args(f, bc, mn, mx, nb) + ["dumpFab=1", "normalize=1", "fabFileBase=pdf"], tmp_path)
        assert out.stdout == "" and open(tmp_path / "pdf.fab", "rb").read() == fab
    if name == "n8_16x16":  # condApply: the third stderr line
        refc = reference(name, (2, 0.1, 1))
        ac, hc = refc.table()
        wantc, errc, _, _ = B.tool_output(ac, hc, bc, mn, mx, nb, total, outside_area=math.fsum(refc.outside))
        out = _tool(_tool_args(f, bc, mn, mx, nb) + ["condApply=1", "condComp=2", "condVal=0.1", "condSgn=1"], tmp_path)
        assert out.stdout == wantc and out.stderr.split("\n")[4:7] == errc
        bad = subprocess.run([os.path.join(BIN, "binMEF3d.ex"), "infile=" + f, "binComps=3 9", "binMin=0 0", "binMax=1 1", "nBins=2 2"], cwd=tmp_path,
                             capture_output=True, text=True)
        assert bad.returncode != 0 and "At least one element in binComps out of range" in bad.stderr
        bad = subprocess.run([os.path.join(BIN, "binMEF3d.ex"), "infile=" + f, "binComps=3", "binMin=0", "binMax=1", "nBins=20000000"], cwd=tmp_path,
                             capture_output=True, text=True)
        assert bad.returncode != 0 and "2^24 bins" in bad.stderr


def test_chain_from_isosurface_tool(tmp_path):
    """isosurface3d.ex (an isosurface of temp carrying x_velocity and density) -> binMEF3d.ex on the two carried fields, against the
    restatement run on the MEF as plotfile.read_mef reads it; binned on the iso field itself everything lands in ONE bin"""
    H = nested_hierarchy(16, 1, 8, is_per=(0, 0, 0))
    mfs = make_states(H, 3, 0, field_flame, seed=77)
    p = str(tmp_path / "plt00005")
    write_plotfile(p, H, mfs, ["temp", "x_velocity", "density"], time=0.125, level_steps=[5])
    iso = subprocess.run([os.path.join(BIN, "isosurface3d.ex"), "infile=" + p, "isoCompName=temp", "isoVal=1150", "comps=0 1 2"], cwd=tmp_path,
                         capture_output=True, text=True)
    assert iso.returncode == 0, iso.stderr
    f = p + "_temp_1150.mef"
    label, names, nodes, faces = read_mef(f)
    assert names == ["X", "Y", "Z", "temp", "x_velocity", "density"] and len(faces) > 100
    bc, nb = (4, 5), (8, 6)
    mn = tuple(float(np.floor(nodes[:, c].min() * 8) / 8) for c in bc)
    mx = tuple(float(np.ceil(nodes[:, c].max() * 8) / 8) + 0.125 for c in bc)
    ref = B.bin_surface(nodes, faces, bc, mn, mx, nb)
    area, hits = ref.table()
    want, err, _, _ = B.tool_output(area, hits, bc, mn, mx, nb, math.fsum(ref.elem_areas))
    out = _tool(_tool_args(f, bc, mn, mx, nb), tmp_path)
    assert ref.n_my > 0 and int((hits > 0).sum()) > 4
    assert out.stdout == want and out.stderr.split("\n")[4:6] == err
    # the iso field: one bin holds every leaf
    one = B.bin_surface(nodes, faces, (3,), (1000.0,), (1300.0,), (3,))
    a1, h1 = one.table()
    assert (h1 > 0).tolist() == [False, True, False]
    want1, _, _, _ = B.tool_output(a1, h1, (3,), (1000.0,), (1300.0,), (3,), math.fsum(one.elem_areas))
    for extra in ([], ["uncombined=1"]):
        assert _tool(_tool_args(f, (3,), (1000.0,), (1300.0,), (3,)) + extra, tmp_path).stdout == want1
