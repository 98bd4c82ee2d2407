"""GPU tier: the surface and stream-tube kernels against what the REFERENCE's compiled code returned.  The expected values are read
from tests/golden/<tool>_ref.npz (recorded by tests/golden/make_golden_surf.py from oracle/_ref); the inputs are built again by
tests/surfpin_cases.py and their digests are checked.  Nothing here reads the reference tree or needs oracle/_ref, and no restatement
stands between the kernels and the record: the quantities are the ones test_gpu_binmef.py, test_gpu_surfcut.py, test_gpu_surfjoin.py
and test_gpu_tubestats.py compare with tests/*_ref.py.

  pa_surfbin_*   every bin: hits equal, area == math.fsum of the recorded leaves of the bin (the kernels add in 192-bit fixed point and
                 round once); NmyTriangles equal; the outside area == fsum of the recorded outside leaves; the total == fsum of the
                 recorded element areas.  A case with more than 12 000 leaves keeps the reference's serial table only: there
                 |gpu - serial| <= hits * 2^-52 * serial per bin, which holds for ANY two orders of summing `hits` nonnegative terms
                 (each of the hits - 1 additions of the serial sum errs by at most 2^-53 of a partial sum <= the result; the exactly
                 rounded sum adds 2^-53 more).  Combined and `uncombined` mode.
  pa_surf_slice  vertices as bits, directed pairs and segments.  The contour LINES are assembled on the host (tools/common/pa_contour.h):
                 test_surf_reference_pin.py holds that code to the recorded lines.
  pa_surf_trim   nodes as bits, elements, the unused-node count; the areas before and after: smallest and largest as bits, the total ==
                 the exactly rounded sum of the recorded terms (the rule of test_gpu_fixed_sums.py).
  pa_surfjoin_*  nodes as bits and elements after every step of a chain, with the grid / auto path and with brute force.
  pa_tube_*      the sums over the wedges formed, in the reference's order, from the recorded per-wedge volumes, integrals and areas;
                 peak samples and flags; neighbour lists; one smoothing pass.
Not pinned (tests/test_surf_reference_pin.py says why): max_grad (a documented deviation), merges with a surface
without elements, non-finite elements in binMEF.  Outputs start as the payload NaN of tests/util.py where the binding lets them."""
import ctypes as C
import math

import numpy as np
import pytest

import fixed192_ref as FX
import surfpin_cases as P
from peleanalysis_amd import capi
from util import SENT_GPU, sentinel_count

pytestmark = pytest.mark.gpu

HITS_SENTINEL = -0x0BADC0DE


def ub(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(ub(a), ub(b))


def check_digest(tool, c, digest):
    assert str(P.load(tool)[c["name"] + "_sha"]) == digest(c), c["name"]


def exact_total(terms):
    """the exactly rounded sum, as the 192-bit accumulator returns it (tests/fixed192_ref.py)"""
    terms = [float(t) for t in terms]
    if not terms:
        return 0.0
    s = FX.scale_of(max(terms))
    tot, flag = FX.sum_terms(terms, s)
    assert flag == 0
    return FX.read(tot, s)


# ------------------------------------------------------------------------------------------------ binMEF
def surfbin_read_into_sentinels(sb):
    """SurfBin.read with the two tables starting as sentinels"""
    nt = int(np.prod(sb.nbins, dtype=np.int64))
    area, hits = np.full(nt, SENT_GPU, dtype=np.uint64).view(np.float64), np.full(nt, HITS_SENTINEL, dtype=np.int64)
    tot, outside = C.c_double(math.nan), C.c_double(math.nan)
    cnt = np.full(8, HITS_SENTINEL, dtype=np.int64)
    p64 = C.POINTER(C.c_int64)
    sb.ctx.check(sb.ctx.lib.pa_surfbin_read(sb.ctx.h, sb.h, area.ctypes.data_as(C.POINTER(C.c_double)), hits.ctypes.data_as(p64), C.byref(tot), C.byref(outside),
                                            cnt.ctypes.data_as(p64)))
    assert sentinel_count(area, SENT_GPU) == 0 and not (hits == HITS_SENTINEL).any()
    return area, hits, tot.value, outside.value, dict(zip(sb.COUNTERS, (int(v) for v in cnt)))


def check_surfbin(ctx, c, uncombined):
    g = P.load("binmef")
    k, what = c["name"], (c["name"], "uncombined" if uncombined else "combined")
    with capi.SurfBin(ctx, c["nbins"], c["bin_min"], c["bin_max"]) as sb:
        amax = sb.max_area(c["nodes"], c["elts"])
        sb.begin(amax)
        kw = dict(cond_apply=True, cond_comp=c["cond"][0], cond_val=c["cond"][1], cond_sgn=c["cond"][2]) if c["cond"] else {}
        sb.add_surface(c["nodes"], c["elts"], c["bin_comps"], uncombined=uncombined, **kw)
        area, hits, tot, outside, cnt = surfbin_read_into_sentinels(sb)
    nt = len(area)
    want_hits = np.zeros(nt, dtype=np.int64)
    want_hits[g[k + "_tk"]] = g[k + "_th"]
    assert np.array_equal(hits, want_hits), (what, int((hits != want_hits).sum()))
    assert cnt["n_my"] == int(g[k + "_nmy"]) and cnt["nonfinite"] == 0 and cnt["elements"] == len(c["elts"]), (what, cnt)
    leaves, ea = P.binmef_leaves(g, c), P.binmef_elem_areas(g, c)
    if leaves is not None:
        keys, areas, out_leaves = leaves
        mag = math.frexp(amax)[1]  # the precondition of ==: no term is below 2^-104 of the magnitude declared at begin, so none is truncated
        assert all(t == 0.0 or t >= 2.0 ** (mag - 104) for t in np.concatenate([areas, out_leaves] + ([ea] if ea is not None else []))), what
        per = [[] for _ in range(nt)]
        for q, a in zip(keys.tolist(), areas.tolist()):
            per[q].append(a)
        want = np.array([math.fsum(p) for p in per])
        assert same(area, want), (what, int((ub(area) != ub(want)).sum()))
        assert same(outside, math.fsum(out_leaves)), (what, outside)
    else:
        ser = np.zeros(nt)
        ser[g[k + "_tk"]] = g[k + "_ta"]
        assert np.all(np.abs(area - ser) <= want_hits * 2.0 ** -52 * ser), (what, float(np.abs(area - ser).max()))
        so = float(g[k + "_outside"])
        assert abs(outside - so) <= int(g[k + "_noutside"]) * 2.0 ** -52 * so, (what, outside, so)
    if ea is not None:
        assert same(tot, math.fsum(ea)), (what, tot)
    else:
        st = float(g[k + "_total"])
        assert abs(tot - st) <= len(c["elts"]) * 2.0 ** -52 * st, (what, tot, st)


@pytest.mark.parametrize("name", [c["name"] for c in P.binmef_cases() if not c["name"].startswith("soup")])
def test_surfbin_named_cases_equal_the_reference(ctx, name):
    c = next(c for c in P.binmef_cases() if c["name"] == name)
    check_digest("binmef", c, P.binmef_digest)
    for uncombined in (False, True):
        check_surfbin(ctx, c, uncombined)


@pytest.mark.parametrize("block", range(4))
def test_surfbin_edge_soups_equal_the_reference(ctx, block):
    """16 soups per test: values on bin edges and one ulp off them, collinear triangles, 1 to 4 components, every kind of condition"""
    for i in range(16 * block, 16 * block + 16):
        c = P.edge_soup(i)
        check_digest("binmef", c, P.binmef_digest)
        for uncombined in (False, True):
            check_surfbin(ctx, c, uncombined)


# ------------------------------------------------------------------------------------------------ sliceMEF
def check_slice(s, c, g):
    k = c["name"]
    V, Pr, Sg = g[k + "_V"], g[k + "_P"], g[k + "_S"]
    assert s.slice(c["comp"], c["loc"]) == (len(V), len(Sg)), k
    verts, pairs, segs = s.slice_read(fill=SENT_GPU)[:3]
    assert sentinel_count(verts, SENT_GPU) == 0, k
    assert same(verts, V.reshape(verts.shape)), (k, int((ub(verts) != ub(V.reshape(verts.shape))).sum()))
    assert np.array_equal(pairs, Pr.reshape(pairs.shape)) and np.array_equal(segs, Sg.reshape(segs.shape)), k


@pytest.mark.parametrize("name", list(P.SC.SLICES))
def test_slices_of_named_surfaces_equal_the_reference(ctx, name):
    g = P.load("slicemef")
    cases = [c for c in P.slicemef_cases() if c["name"].rsplit("_", 1)[0] == name and not c["name"].startswith("patch")]
    assert len(cases) == len(P.SC.SLICES[name][1])
    with capi.Surf(ctx, cases[0]["nodes"], cases[0]["elts"]) as s:
        for c in cases:
            check_digest("slicemef", c, P.slicemef_digest)
            check_slice(s, c, g)


@pytest.mark.parametrize("block", range(4))
def test_slices_of_patches_equal_the_reference(ctx, block):
    """16 patches per test: mixed diagonals; shuffled, dropped, duplicated and reversed elements; nodes on the location and within
    epsilon of it"""
    g = P.load("slicemef")
    for i in range(16 * block, 16 * block + 16):
        c = P.patch(i)
        check_digest("slicemef", c, P.slicemef_digest)
        with capi.Surf(ctx, c["nodes"], c["elts"]) as s:
            check_slice(s, c, g)


# ------------------------------------------------------------------------------------------------ trimMEFgen
@pytest.mark.parametrize("name", list(P.SC.TRIMS))
def test_trims_equal_the_reference(ctx, name):
    g = P.load("trimmef")
    c = next(c for c in P.trimmef_cases() if c["name"] == name)
    check_digest("trimmef", c, P.trimmef_digest)
    src, E = g[name + "_src"], g[name + "_E"].astype(np.int32).reshape(-1, 3)
    want_nodes = np.ascontiguousarray(c["nodes"][src]).reshape(len(src), c["nodes"].shape[1])
    with capi.Surf(ctx, c["nodes"], c["elts"]) as s:
        for areas, when in ((g[name + "_A0"], "before"), (g[name + "_A1"], "after")):
            if when == "after":
                assert s.trim(c["conds"], c["rxy"], c["sign_rxy"]) == int(g[name + "_unused"]), name
                nodes, elts = s.read(fill=SENT_GPU)
                assert nodes.shape == want_nodes.shape and sentinel_count(nodes, SENT_GPU) == 0 and same(nodes, want_nodes), name
                assert elts.dtype == np.int32 and np.array_equal(elts, E), name
            tot, lo, hi = s.area()
            if len(areas):
                assert same(tot, exact_total(areas)) and same(lo, areas.min()) and same(hi, areas.max()), (name, when, tot, lo, hi)
            else:
                assert (tot, lo, hi) == (0.0, 0.0, 0.0), (name, when)


# ------------------------------------------------------------------------------------------------ mergeMEF
def check_merge(ctx, c, g, method):
    want = P.merge_expected(c, g)
    with capi.Surf(ctx, c["M"][0], c["M"][1]) as m:
        for q, s in enumerate(c["S"]):
            with capi.Surf(ctx, s[0], s[1]) as t:
                m.merge(t, c["eps"], c["rem"], method)
            nodes, elts = m.read(fill=SENT_GPU)
            wn, we = want[q]
            assert nodes.shape == wn.shape and elts.shape == we.shape, (c["name"], q, method, nodes.shape, wn.shape)
            assert sentinel_count(nodes, SENT_GPU) == 0 and same(nodes, wn), (c["name"], q, method, int((ub(nodes) != ub(wn)).sum()))
            assert np.array_equal(elts, we), (c["name"], q, method)


@pytest.mark.parametrize("name", [n for n in P.JC.MERGES if n not in P.MERGE_NOT_PINNED])
def test_merge_chains_equal_the_reference(ctx, name):
    g = P.load("mergemef")
    c = next(c for c in P.mergemef_cases() if c["name"] == name)
    check_digest("mergemef", c, P.mergemef_digest)
    for method in (0, 2):
        check_merge(ctx, c, g, method)


@pytest.mark.parametrize("block", range(2))
def test_merge_pairs_equal_the_reference(ctx, block):
    """16 pairs per test: nodes at distance exactly eps, just inside and just outside; clusters where the lowest index must win; eps = 0"""
    g = P.load("mergemef")
    for i in range(16 * block, 16 * block + 16):
        c = P.pair(i)
        check_digest("mergemef", c, P.mergemef_digest)
        for method in (0, 2):
            check_merge(ctx, c, g, method)


# ------------------------------------------------------------------------------------------------ streamTubeStats
def tube_setup(ctx, c):
    from test_gpu_tubestats import tables
    box, node, fabs = tables(c["path"])
    tube = capi.Tube(ctx, box, node, c["path"]["face"])
    xyz = capi.Tube.flat([a[:3] for a in fabs])
    data = capi.Tube.flat([a[list(c["comps"])] for a in fabs]) if len(c["comps"]) else np.zeros(1)
    return tube, xyz, data


@pytest.mark.parametrize("name", [t[0] for t in P.TUBES if t[1] == "wedges"])
def test_tube_wedges_equal_the_reference(ctx, name):
    """the element loop of streamTubeStats.cpp:650-699 over the RECORDED per-wedge values, in its order of additions"""
    g = P.load("tubestats")
    c = P.tube_case(name)
    check_digest("tubestats", c, P.tube_digest)
    K, E = len(c["comps"]), len(c["face"]) // 3
    vol_j, area_j, int_j, area0 = g[name + "_vol"], g[name + "_area"], g[name + "_integ"], g[name + "_area0"]
    vol, wa, raw = np.zeros(E), np.zeros(E), np.zeros((K, E))
    with np.errstate(all="ignore"):
        for j in range(c["npts"] - 1):
            vol += vol_j[j]
            for q in range(K):
                raw[q] += int_j[j, q]
                if q == 0:
                    wa += int_j[j, 0] * (0.5 * (area_j[j] + area_j[j + 1]))
        per = raw / area0
    tube, xyz, data = tube_setup(ctx, c)
    got = tube.wedges(xyz, data, K, c["jl"], c["npts"])
    tube.close()
    for gq, w, what in zip(got, (vol, area0, wa, raw, per), ("volume", "area", "area_wtAvg", "raw", "per area")):
        assert gq.shape == w.shape and np.array_equal(np.isnan(gq), np.isnan(w)), (name, what)
        fin = ~np.isnan(w)
        assert np.array_equal(ub(gq)[fin], ub(w)[fin]), (name, what, int((ub(gq)[fin] != ub(w)[fin]).sum()))


@pytest.mark.parametrize("name", [t[0] for t in P.TUBES if t[1] == "lines"])
def test_tube_peaks_equal_the_reference(ctx, name):
    g = P.load("tubestats")
    c = P.tube_case(name)
    check_digest("tubestats", c, P.tube_digest)
    tube, xyz, data = tube_setup(ctx, c)
    for i, (p, sc) in enumerate(P.PEAKS):
        s, ok = tube.peaks(data, len(c["comps"]), p, list(sc))
        w = g["%s_ps%d" % (name, i)]
        assert same(s, w.reshape(s.shape)) and np.array_equal(ok, g["%s_pok%d" % (name, i)].astype(bool)), (name, i)
    tube.close()


@pytest.mark.parametrize("name", [t[0] for t in P.TUBES if t[1] == "neighbours"])
def test_tube_neighbours_and_smoothing_equal_the_reference(ctx, name):
    g = P.load("tubestats")
    c = P.tube_case(name)
    check_digest("tubestats", c, P.tube_digest)
    tube, xyz, data = tube_setup(ctx, c)
    rp, cols = tube.neighbors()
    assert np.array_equal(rp, g[name + "_rp"]) and np.array_equal(cols, g[name + "_cols"]), name
    vals, area = P.smooth_inputs(name, tube.nElts)
    assert same(tube.smooth(vals, area, 1), g[name + "_sm"]), name
    tube.close()
