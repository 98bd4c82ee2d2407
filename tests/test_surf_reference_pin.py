"""CPU tier: the restatements of the surface and stream-tube tools held to the REFERENCE's compiled code.  `make -C oracle ref` cuts
the arithmetic of binMEF.cpp, sliceMEF.cpp, trimMEFgen.cpp, mergeMEF.cpp and streamTubeStats.cpp out of the reference tree and compiles
it (oracle/ref/*_ref_wrap.cpp, oracle/ref/surf_shim.h); tests/golden/make_golden_surf.py recorded what it returns for the cases of
tests/surfpin_cases.py (tests/golden/<tool>_ref.npz).  Here: the records belong to today's case builders (digests); binmef_ref,
surfcut_ref, surfjoin_ref and tubestats_ref reproduce them bit for bit; where oracle/_ref exists a fresh run of the compiled code
reproduces them too and a seeded fuzz compares restatement and compiled code on inputs the records do not hold; the host run of the
binMEF kernels' path code gives the recorded leaves; the matrix holds the situations it was built for; and planted mistakes fail.

Kept OUT of the pinned set, on purpose:
  - max_grad of streamTubeStats.cpp.  Its second pass starts from the coordinates of the line's LAST point (hiX is not reset at :920);
    tubestats_ref and the kernels walk the line's own segments (streamTubeStats3d).  The record holds the reference's
    values, and test_max_grad_deviation_is_the_documented_one checks that they are what INTEGRATION.md says they are.
  - merges with a surface that has no element (surfjoin_cases empty_s, m_without_elements): mergeMEF.cpp divides by zero there.
  - elements with a value that is not finite in binMEF (skipped and counted; undefined in the reference).
  - the third epsilon test of VI_doIt (|v1 - v2| < epsilon) cannot decide on a cut edge -- there the first test holds already -- so
    no slice reaches it; the live check calls VI_doIt directly on such a pair.
The area TOTALS of the restatements are exactly rounded sums (tests/fixed192_ref.py) where the reference adds serially: the terms are
pinned bit for bit, and the reference's serial totals to the serial sum of those terms."""
import collections
import math

import numpy as np
import pytest

import binmef_ref as B
import surfcut_ref as CR
import surfjoin_ref as JR
import surfpin_cases as P
import tubestats_ref as T
from oracle import surfref as S

TOOL_NAMES = list(P.TOOLS)


def ub(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(ub(a), ub(b))


def have(tool):
    return (S.lib_tube() if tool == "tubestats" else S.lib(tool)) is not None


# ------------------------------------------------------------------------------------------------ the comparisons
def binmef_agrees(c, g, R=None):
    """the restatement R of case c against the record: leaves in visiting order (where kept), the serial table, the counts"""
    R = R or P.binmef_restatement(c)
    k = c["name"]
    ser, hits = R.table_serial()
    touched = np.nonzero(hits)[0]
    ok = R.nonfinite == 0 and R.n_my == int(g[k + "_nmy"]) and len(R.areas) == int(g[k + "_nleaves"]) and len(R.outside) == int(g[k + "_noutside"])
    ok = ok and np.array_equal(touched, g[k + "_tk"]) and same(ser[touched], g[k + "_ta"]) and np.array_equal(hits[touched], g[k + "_th"])
    ok = ok and same(P._serial(R.outside), g[k + "_outside"]) and same(P._serial(R.elem_areas), g[k + "_total"])
    ea = P.binmef_elem_areas(g, c)
    if ea is not None:
        ok = ok and same(R.elem_areas, ea)
    leaves = P.binmef_leaves(g, c)
    if leaves is not None:
        ok = ok and np.array_equal(np.asarray(R.keys, dtype=np.int64), leaves[0]) and same(R.areas, leaves[1]) and same(sorted(R.outside), leaves[2])
    return bool(ok)


def slice_agrees(c, g, mistake=None):
    k = c["name"]
    w = CR.slice_surface(c["nodes"], c["elts"], c["comp"], c["loc"], mistake=mistake)
    lines = CR.contour_lines(w["segs"], mistake=mistake)
    flat = np.array([s for ln in lines for s in ln], dtype=np.int64).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(np.int64)
    return bool(same(w["verts"], g[k + "_V"]) and np.array_equal(w["pairs"], g[k + "_P"]) and np.array_equal(w["segs"], g[k + "_S"])
                and np.array_equal(flat, g[k + "_L"]) and np.array_equal(off, g[k + "_LO"]))


def trim_agrees(c, g, mistake=None):
    k = c["name"]
    n2, e2, unused = CR.trim_surface(c["nodes"], c["elts"], c["conds"], c["rxy"], c["sign_rxy"], mistake=mistake)
    src = g[k + "_src"]
    ok = n2.shape == (len(src), c["nodes"].shape[1]) and same(n2, c["nodes"][src].reshape(n2.shape)) and np.array_equal(e2, g[k + "_E"]) and unused == int(g[k + "_unused"])
    if ok and mistake is None:
        a0, a1 = CR.triangle_areas(c["nodes"], c["elts"]), CR.triangle_areas(n2, e2)
        ok = same(a0, g[k + "_A0"]) and same(a1, g[k + "_A1"]) and same(P._serial(a0), g[k + "_T0"]) and same(P._serial(a1), g[k + "_T1"])
    return bool(ok)


def merge_agrees(c, g, mistake=None):
    nodes, elts = c["M"]
    for (wn, we), s in zip(P.merge_expected(c, g), c["S"]):
        nodes, elts, _ = JR.merge_iso(nodes, elts, s[0], s[1], c["eps"], c["rem"], mistake=mistake, rows=mistake is None)
        if not (same(nodes, wn) and np.array_equal(elts, we)):
            return False
    return True


def tube_agrees(c, g):
    k, L, n = c["name"], c["L"], c["n"]
    idX = [0, 1, 2]
    with np.errstate(all="ignore"):
        if c["kind"] == "wedges":
            ok = same(T.wedge_surf_area(L, n, idX, 0), g[k + "_area0"])
            for j in range(c["npts"]):
                ok = ok and same(T.wedge_surf_area(L, n, idX, c["jl"] + j), g[k + "_area"][j])
            for j in range(c["npts"] - 1):
                ok = ok and same(T.wedge_volume_int(L, n, c["jl"] + j, -1, idX), g[k + "_vol"][j])
                for q in range(len(c["comps"])):
                    ok = ok and same(T.wedge_volume_int(L, n, c["jl"] + j, 3 + q, idX), g[k + "_integ"][j, q])
            return bool(ok)
        if c["kind"] == "lines":
            ok = True
            for i, (p, sc) in enumerate(P.PEAKS):
                s, good = T.peak_val(L, 3 + p, [3 + q for q in sc])
                ok = ok and same(s, g["%s_ps%d" % (k, i)]) and np.array_equal(good, g["%s_pok%d" % (k, i)].astype(bool))
            return bool(ok)
    nb = T.build_node_neighbors(c["path"]["face"], len(L.node_box))
    vals, area = P.smooth_inputs(k, len(nb))
    return bool(np.array_equal(np.concatenate([[0], np.cumsum([len(x) for x in nb])]), g[k + "_rp"])
                and np.array_equal(np.concatenate([np.asarray(x, np.int64) for x in nb]), g[k + "_cols"]) and same(T.smooth_vals(vals, area, nb), g[k + "_sm"]))


AGREES = {"binmef": binmef_agrees, "slicemef": slice_agrees, "trimmef": trim_agrees, "mergemef": merge_agrees, "tubestats": tube_agrees}
DIGEST = {"binmef": P.binmef_digest, "slicemef": P.slicemef_digest, "trimmef": P.trimmef_digest, "mergemef": P.mergemef_digest, "tubestats": P.tube_digest}


# ------------------------------------------------------------------------------------------------ records and restatements
@pytest.mark.parametrize("tool", TOOL_NAMES)
def test_fixture_belongs_to_todays_cases(tool):
    g = P.load(tool)
    cases = P.TOOLS[tool][0]()
    assert g.names == [c["name"] for c in cases]
    for c in cases:
        assert str(g[c["name"] + "_sha"]) == DIGEST[tool](c), c["name"]
    if tool == "binmef":
        assert sum(c["name"].startswith("soup") for c in cases) == 64
        assert all(("%s_lk" % c["name"] in g or "%s_lm" % c["name"] in g) == (int(g[c["name"] + "_nleaves"]) + int(g[c["name"] + "_noutside"]) <= P.MAX_LEAVES) for c in cases)
    if tool == "slicemef":
        assert sum(c["name"].startswith("patch") for c in cases) == 64
    if tool == "mergemef":
        assert sum(c["name"].startswith("pair") for c in cases) == 32 and all(len(c["M"][0]) <= 200 and len(c["S"][0][0]) <= 200 for c in cases if c["name"].startswith("pair"))


@pytest.mark.parametrize("tool", TOOL_NAMES)
def test_restatement_equals_the_reference_record(tool):
    g = P.load(tool)
    bad = [c["name"] for c in P.TOOLS[tool][0]() if not AGREES[tool](c, g)]
    assert bad == []


def _max_grad_as_compiled(L, comp):
    """INTEGRATION.md, streamTubeStats3d: the second pass of max_grad (:920-949) keeps hiX of the first pass, so its first segment runs
    from the line's LAST point to point 1, with the values of points 0 and 1; the line's own segments never pass L > maxs"""
    out = np.zeros(len(L.node_box))
    for q in range(len(L.boxes)):
        m, pts = L.lines_of_box(q)
        for node, p in zip(m, pts):
            a = L.fab[q][:, :, p]
            npts = a.shape[1]
            if npts < 2:
                continue
            seg = lambda u, v: math.sqrt(sum([(a[d, v] - a[d, u]) * (a[d, v] - a[d, u]) for d in range(3)]))
            maxs = max(seg(i - 1, i) for i in range(1, npts))
            first = seg(npts - 1, 1)
            if first > maxs:
                with np.errstate(all="ignore"):
                    out[node] = abs((a[comp, 1] - a[comp, 0]) / np.float64(first))
    return out


def test_max_grad_deviation_is_the_documented_one():
    g = P.load("tubestats")
    differs = 0
    for name in ("lines21", "lines22"):
        c = P.tube_case(name)
        for q in range(len(c["comps"])):
            rec = g[name + "_grad"][q]
            assert same(rec, _max_grad_as_compiled(c["L"], 3 + q)), (name, q)
            ours = T.max_grad(c["L"], 3 + q, [0, 1, 2], False)
            assert not ours.any()
            differs += int((rec != ours).sum())
    assert differs > 0  # the deviation shows on these lines: max_grad is not pinned to the reference


# ------------------------------------------------------------------------------------------------ the compiled code, live
@pytest.mark.parametrize("tool", TOOL_NAMES)
def test_compiled_reference_reproduces_the_record(tool):
    if not have(tool):
        pytest.skip("oracle/_ref/lib%s_ref.so is not built and there is no reference tree" % tool)
    g = P.load(tool)
    cases, record = P.TOOLS[tool]
    for c in cases():
        for key, v in record(c).items():
            w = g["%s_%s" % (c["name"], key)]
            v = np.asarray(v)
            assert v.shape == w.shape, (c["name"], key)
            if v.dtype.kind == "f":
                assert same(v, w), (c["name"], key)
            elif v.dtype.kind == "U":
                assert str(v) == str(w), (c["name"], key)
            else:
                assert np.array_equal(v.astype(np.int64), w), (c["name"], key)


def _live_as_golden(records):
    """{<case>_<key>: array} of fresh records, read the way a fixture is read"""
    d = {}
    for name, r in records:
        for k, v in r.items():
            v = np.asarray(v)
            d["%s_%s" % (name, k)] = v.astype(np.int64) if v.dtype.kind in "iu" else v
    return d


FUZZ = {"binmef": lambda: [P.edge_soup(i) for i in range(64, 464)], "slicemef": lambda: [P.patch(i) for i in range(64, 464)],
        "mergemef": lambda: [P.pair(i) for i in range(32, 132)]}


@pytest.mark.parametrize("tool", ["binmef", "slicemef", "mergemef"])
def test_fuzz_restatement_against_compiled_reference(tool):
    """400 more soups, 400 more patches, 100 more pairs: the same builders, seeds the records do not hold"""
    if not have(tool):
        pytest.skip("oracle/_ref/lib%s_ref.so is not built and there is no reference tree" % tool)
    record = P.TOOLS[tool][1]
    bad = []
    for c in FUZZ[tool]():
        try:
            live = _live_as_golden([(c["name"], record(c))])
        except S.RefAssertion:
            with pytest.raises(B.SplitFractionError):  # both stop, or neither
                P.binmef_restatement(c)
            continue
        if not AGREES[tool](c, live):
            bad.append(c["name"])
    assert bad == []


def test_fuzz_trim_and_tube_against_compiled_reference():
    if not (have("trimmef") and have("tubestats")):
        pytest.skip("oracle/_ref is not built and there is no reference tree")
    from test_gpu_tubestats import random_dir  # the builder only: nothing of that module runs here
    import streamsample_ref as SS
    rng = np.random.default_rng(2024)
    for i in range(64, 264):  # the patches as surfaces, with random conditions and radii
        c = P.patch(i)
        nodes = c["nodes"]
        comps = [int(rng.integers(5)) for _ in range(int(rng.integers(3)))]
        conds = tuple((cc, CR.SIGNS[int(rng.integers(5))], float(nodes[int(rng.integers(len(nodes))), cc])) for cc in comps)  # a value some node holds
        rxy = float(np.round(rng.uniform(0.2, 1.2), 2)) if rng.random() < 0.5 else -1.0
        t = dict(name=c["name"], nodes=nodes, elts=c["elts"], conds=conds, rxy=rxy, sign_rxy=CR.SIGNS[int(rng.integers(5))])
        assert trim_agrees(t, _live_as_golden([(t["name"], P.record_trimmef(t))])), t
    for seed in range(100, 106):
        files = random_dir(seed, K=3, uniform_j=bool(seed % 2))[1]
        path = SS.read_stream_dir(files)
        L = T.Lines(path, [0, 1, 2, 3, 4, 5])
        boxes = [(lo[1], np.ascontiguousarray(np.asarray(a)[:6]), np.asarray(path["ins"][l][b], dtype=np.int32)) for l, lev in enumerate(path["levels"])
                 for b, (lo, hi, a) in enumerate(lev)]
        face = np.asarray(path["face"], np.int64)
        n = [face[k::3] - 1 for k in range(3)]
        R = S.Tube(boxes)
        jlo, jhi = int(L.jlo_b[L.jhi_b > L.jlo_b].max()), int(L.jhi_b[L.jhi_b > L.jlo_b].min())  # the range every box with lines holds
        with np.errstate(all="ignore"):
            for pt in range(jlo, jhi):
                for comp in (-1, 3, 5):
                    v, a = R.wedges(face, pt, comp)
                    assert same(v, T.wedge_volume_int(L, n, pt, comp, [0, 1, 2])) and same(a, T.wedge_surf_area(L, n, [0, 1, 2], pt)), (seed, pt, comp)
        s, ok = R.peaks(4, [3, 5])
        ws, wok = T.peak_val(L, 4, [3, 5])
        assert same(s, ws) and np.array_equal(ok, wok), seed


def test_vi_doit_branches_against_compiled_reference():
    """VI_doIt (sliceMEF.cpp:581-605) called directly: each of the three epsilon tests and the interpolation, the third of which no
    slice reaches"""
    if not have("slicemef"):
        pytest.skip("oracle/_ref/libslicemef_ref.so is not built and there is no reference tree")
    rng = np.random.default_rng(3)
    for v1, v2 in ((1.0 - 0.4e-8, 2.0), (0.0, 1.0 + 0.4e-8), (1.0 - 0.3e-8, 1.0 + 0.3e-8), (1.5, 1.5 + 0.5e-8), (1.5 + 0.5e-8, 1.5), (0.25, 1.75), (3.0, -1.0),
                   (1.0 - 1.0e-8, 2.0), (0.0, 1.0 + 1.0e-8)):
        p1, p2 = rng.uniform(-1.0, 1.0, size=5), rng.uniform(-1.0, 1.0, size=5)
        p1[3], p2[3] = v1, v2
        assert same(S.slicemef_vi(1.0, 3, p1, p2), CR.vi_doit(1.0, 3, [p1.tolist(), p2.tolist()], 0, 1)), (v1, v2)


# ------------------------------------------------------------------------------------------------ the kernels' path code, on the host
def test_binmef_host_run_gives_the_recorded_leaves(tmp_path):
    """tools/bench/binmef_host.hip (the code the kernels run for one path of the recursion, and the slice rule of the rounds) on every
    edge soup, with a list of 4096 items and with one of 64: the recorded leaves as a multiset, area bits included; flag 0"""
    from test_binmef_ref import _bits, _host_build, _host_run
    g = P.load("binmef")
    exe = str(tmp_path / "binmef_host")
    _host_build(exe)
    for c in P.binmef_cases():
        if not c["name"].startswith("soup"):
            continue
        keys, areas, outside = P.binmef_leaves(g, c)
        nt = int(np.prod(c["nbins"]))
        want = collections.Counter([(int(k), _bits(a)) for k, a in zip(keys, areas)] + [(nt, _bits(a)) for a in outside]
                                   + [(nt + 1, _bits(a)) for a in P.binmef_elem_areas(g, c)])
        for cap in (1 << 12, 64):
            got, cnt = _host_run(exe, str(tmp_path), c["nodes"], c["elts"], c["bin_comps"], c["bin_min"], c["bin_max"], c["nbins"], cap, c["cond"])
            assert collections.Counter(map(tuple, got.tolist())) == want, (c["name"], cap)
            assert cnt["flag"] == 0 and cnt["peak"] <= cap, (c["name"], cap, cnt)


def test_host_line_assembly_gives_the_recorded_lines(tmp_path):
    """tools/common/pa_contour.h (what sliceMEF3d.ex assembles the contour lines with, through tools/src/contourCheck.cpp) on the
    RECORDED segments of every cut with at most 600 of them: the recorded lines, by its fast path and by its list scan"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "contourCheck")
    r = subprocess.run(["g++", "-std=c++17", "-O2", "-I" + root, os.path.join(root, "tools", "src", "contourCheck.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    g = P.load("slicemef")
    ran = 0
    for c in P.slicemef_cases():
        k = c["name"]
        segs, flat, off = g[k + "_S"], g[k + "_L"].tolist(), g[k + "_LO"]
        if not 0 < len(segs) <= 600:
            continue
        want = [[tuple(s) for s in flat[off[q]:off[q + 1]]] for q in range(len(off) - 1)]
        text = "%d %d\n" % (len(g[k + "_P"]), len(segs)) + "".join("%d %d\n" % (a, b) for a, b in segs.tolist())
        r = subprocess.run([exe, "lines"], input=text, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", (k, r.stderr[-500:])
        rows = r.stdout.split("\n")
        nf = int(rows[0].split()[1])
        parse = lambda block: [[(int(w[i]), int(w[i + 1])) for i in range(0, len(w), 2)] for w in (ln.split() for ln in block)]
        assert parse(rows[1:1 + nf]) == want and parse(rows[2 + nf:2 + 2 * nf]) == want, k
        ran += 1
    assert ran > 90


# ------------------------------------------------------------------------------------------------ what the matrix holds
def test_binmef_matrix_holds_what_it_promises(monkeypatch):
    g = P.load("binmef")
    seen = collections.Counter()
    de, fg = B.find_de, B.find_fg
    monkeypatch.setattr(B, "find_de", lambda *a: (seen.update(["DE"]), de(*a))[1])
    monkeypatch.setattr(B, "find_fg", lambda *a: (seen.update(["FG"]), fg(*a))[1])
    with_leaf = soups = 0
    for c in P.binmef_cases():
        if not c["name"].startswith("soup"):
            continue
        soups += 1
        R = P.binmef_restatement(c)  # a SplitFractionError (the reference's assertion) fails the test: no soup may trip it
        assert binmef_agrees(c, g, R), c["name"]  # evaluated on the PINNED restatement
        with_leaf += len(R.areas) > 0
        seen["nc%d" % len(c["bin_comps"])] += 1
        lo = B.bin_edges(c["bin_min"], c["bin_max"], c["nbins"])
        used = np.unique(c["elts"]) - 1
        for j, comp in enumerate(c["bin_comps"]):
            v = c["nodes"][used, comp]
            seen["above"] += int((v > c["bin_max"][j]).any())
            seen["below"] += int((v < lo[j][0]).any())
            seen["on_edge"] += int(np.isin(v, lo[j]).any())
            seen["at_max"] += int((v == c["bin_max"][j]).any())
        if c["cond"] and len(R.outside):
            seen["fails_sgn%d" % c["cond"][2]] += 1
        if c["cond"] and c["cond"][0] == c["bin_comps"][0]:
            seen["cond_on_binned"] += 1
        seen["dropped_by_areaEps"] += int(any(a < 1.0e-20 for a in R.elem_areas))
    for what in ("DE", "FG", "above", "below", "on_edge", "at_max", "nc1", "nc2", "nc3", "nc4", "fails_sgn-1", "fails_sgn0", "fails_sgn1", "cond_on_binned",
                 "dropped_by_areaEps"):
        assert seen[what] > 0, (what, dict(seen))
    # 30 % of the soups must yield a leaf (a generator that puts everything out of range pins nothing); 59 % do
    assert soups == 64 and with_leaf >= 0.3 * soups, with_leaf


def _eps_branch(c, pair):
    v1, v2 = c["nodes"][pair[0], c["comp"]], c["nodes"][pair[1], c["comp"]]
    return 1 if abs(c["loc"] - v1) < CR.EPS else (2 if abs(c["loc"] - v2) < CR.EPS else (3 if abs(v1 - v2) < CR.EPS else 0))


def test_slice_and_merge_matrix_holds_what_it_promises(monkeypatch):
    g = P.load("slicemef")
    seen = collections.Counter()
    join = CR.join_fragments

    def counting_join(lines):
        before = len([ln for ln in lines if ln])
        out = join(lines)
        seen["joined"] += int(len(out) < before)
        return out

    monkeypatch.setattr(CR, "join_fragments", counting_join)
    for c in P.slicemef_cases():
        assert slice_agrees(c, g), c["name"]  # evaluated on the PINNED restatement (this also runs the counting join)
        k = c["name"]
        seen["multi_line"] += int(len(g[k + "_LO"]) > 2)
        segs = [tuple(sorted(s)) for s in g[k + "_S"].tolist()]
        seen["duplicate_segment"] += int(len(set(segs)) < len(segs))
        for pair in g[k + "_P"].tolist():
            seen["eps%d" % _eps_branch(c, pair)] += 1
    for what in ("multi_line", "joined", "duplicate_segment", "eps0", "eps1", "eps2"):
        assert seen[what] > 0, (what, dict(seen))
    assert seen["eps3"] == 0  # unreachable on a cut edge (module docstring)
    g = P.load("mergemef")
    first_not_nearest = exact = eps0 = 0
    for c in P.mergemef_cases():
        if not c["name"].startswith("pair"):
            continue
        assert merge_agrees(c, g), c["name"]
        xm, xs, e2 = c["M"][0][:, :3], c["S"][0][0][:, :3], c["eps"] * c["eps"]
        eps0 += int(c["eps"] == 0.0)
        for s in xs:
            d = ((0.0 + (s[0] - xm[:, 0]) ** 2) + (s[1] - xm[:, 1]) ** 2) + (s[2] - xm[:, 2]) ** 2
            hit = np.flatnonzero(d <= e2)
            first_not_nearest += int(len(hit) > 1 and d[hit[0]] > d[hit].min())
            exact += int(len(hit) > 0 and d[hit[0]] == e2 and e2 > 0)
    assert first_not_nearest > 0 and exact > 0 and eps0 == 8


# ------------------------------------------------------------------------------------------------ negative controls
@pytest.mark.parametrize("mistake", CR.MISTAKES)
def test_every_planted_mistake_of_surfcut_ref_fails_against_the_record(mistake):
    if mistake in ("elt_any", "keep_unused"):
        g = P.load("trimmef")
        assert any(not trim_agrees(c, g, mistake) for c in P.trimmef_cases())
    else:
        g = P.load("slicemef")
        assert any(not slice_agrees(c, g, mistake) for c in P.slicemef_cases() if len(c["elts"]) <= 2000)


@pytest.mark.parametrize("mistake", JR.MISTAKES)
def test_every_planted_mistake_of_surfjoin_ref_fails_against_the_record(mistake):
    g = P.load("mergemef")
    assert any(not merge_agrees(c, g, mistake) for c in P.mergemef_cases() if len(c["M"][0]) + len(c["S"][0][0]) <= 400)


def test_one_ulp_on_one_leaf_fails_the_binmef_comparison():
    g = P.load("binmef")
    c = next(c for c in P.binmef_cases() if c["name"] == "n6_8x8x8")
    R = P.binmef_restatement(c)
    rec = g.case(c["name"])
    assert binmef_agrees(c, g, R) and binmef_agrees(c, rec, R)
    q = len(R.areas) // 2
    rec[c["name"] + "_la"][q] = np.nextafter(rec[c["name"] + "_la"][q], math.inf)  # one recorded leaf, one ulp
    assert not binmef_agrees(c, rec, R)
    rec = g.case(c["name"])
    lk = rec[c["name"] + "_lk"]
    q = next(i for i in range(len(lk) - 1) if lk[i] != lk[i + 1])
    lk[q], lk[q + 1] = lk[q + 1], lk[q]  # the visiting order is pinned as well
    assert not binmef_agrees(c, rec, R)
    rec = g.case(c["name"])
    rec[c["name"] + "_ta"][0] = np.nextafter(rec[c["name"] + "_ta"][0], 0.0)  # and the serial table
    assert not binmef_agrees(c, rec, R)
