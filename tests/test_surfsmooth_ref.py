"""CPU tier: the restatement tests/surfsmooth_ref.py against answers worked out by hand, its properties, planted mistakes that the
comparison must notice, and surfDATtoMEF3d.ex (a host-only tool) end to end against the restatement of its parser."""
import os
import subprocess

import numpy as np
import pytest

import surfsmooth_cases as SC
import surfsmooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tools", "bin")
BIN_ASAN = os.path.join(ROOT, "tools", "bin_asan")
U = 2.0 ** -53  # the unit roundoff


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ answers by hand
def test_hand_answers_are_exact_and_the_restatement_gives_them():
    exact = SC.verify_hand()  # raises where an operation would round
    nodes, e = SC.hand_surface()
    for (area_comp, nsmooth), want in SC.HAND.items():
        assert [float(v) for v in exact[(area_comp, nsmooth)]] == [float(v) for v in want], (area_comp, nsmooth)
        got = R.smooth(nodes, e, SC.COMP, area_comp, nsmooth)
        w = nodes.copy()
        w[:, SC.COMP] = want
        assert u64(got).tolist() == u64(w).tolist(), (area_comp, nsmooth, got[:, SC.COMP].tolist())


def test_structure_of_the_neighbour_lists():
    nodes, e = SC.structure("same_triple")
    _, info = R.smooth(nodes, e, 3, detail=True)
    assert info["nbr_off"].tolist() == [0, 3, 6, 9, 12] and info["nbr_adj"].tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]  # equal triples are neighbours
    nodes, e = SC.structure("node_twice")
    _, info = R.smooth(nodes, e, 3, detail=True)
    assert info["nbr_adj"].tolist() == [1, 2, 0, 2, 0, 1] and info["w"][1] == 0.0  # the needle: once in each list, no area
    nodes, e = SC.structure("edge_pair")
    assert R.smooth(nodes, e, 3, detail=True)[1]["nbr_adj"].tolist() == [1, 0]  # two shared nodes, one entry
    nodes, e = SC.structure("vertex_pair")
    assert R.smooth(nodes, e, 3, detail=True)[1]["nbr_adj"].tolist() == [1, 0]
    nodes, e = SC.structure("two_patches")
    assert R.smooth(nodes, e, 3, detail=True)[1]["nbr_adj"].tolist() == [1, 0, 3, 2]
    nodes, e = SC.structure("unused_node")
    out, info = R.smooth(nodes, e, 3, nsmooth=2, detail=True)
    assert info["written"] == 4 and u64(out[1]).tolist() == u64(nodes[1]).tolist()
    for k in (63, 64, 65, 300):
        _, info = R.smooth(*SC.structure("fan%d" % k), 3, nsmooth=0, detail=True)
        assert info["max_neighbours"] == k - 1 and info["nbr_off"][-1] == k * (k - 1)
    out = R.smooth(nodes, e, 3, nsmooth=0)
    assert np.array_equal(u64(np.delete(out, 3, axis=1)), u64(np.delete(nodes, 3, axis=1)))  # no other component is touched


# ------------------------------------------------------------------------------------------------ properties
def stage_bound(info, nsmooth, scale):
    """Every stage (to the elements, each iteration, to the nodes) forms fl(sum of w*q) / fl(sum of w) over m <= max|N(e)| + 1 terms.  With
    positive weights the serial sums carry a relative error below (m - 1) u each, the products u each and the quotient u, so a stage's
    result is within (2 m + 1) u |q|max (to first order; doubled here for the higher orders) of a true convex combination of its inputs."""
    m = max(info["max_neighbours"] + 1, 3)
    return (nsmooth + 2) * 2 * (2 * m + 1) * U * scale


@pytest.mark.parametrize("name", list(SC.STRUCTURES))
def test_constant_field_and_range(name):
    nodes, e = SC.structure(name)
    for area_comp in SC.WEIGHTS:
        if name == "node_twice" and area_comp < 0:
            continue  # its needle has area 0: the weights are not all positive
        for nsmooth in SC.NSMOOTH:
            c = nodes.copy()
            c[:, 3] = 0.1
            out, info = R.smooth(c, e, 3, area_comp, nsmooth, detail=True)
            err = np.abs(out[:, 3] - 0.1) / np.spacing(0.1)
            print("%s areaComp %d nSmooth %d: a constant moves by at most %.1f ulp" % (name, area_comp, nsmooth, err.max()))
            # 2 ulp per averaging (to the elements, each iteration, to the nodes) while a sum has at most 16 terms, which covers
            # surfaces of ordinary valence (m = 13).  One thread adds the m = max|N(e)| + 1 terms of a sum one by one, and the
            # worst-case error of such a sum is linear in m, so the allowance is: 2 ulp * ceil(m / 16) per averaging.
            m = info["max_neighbours"] + 1
            assert err.max() <= 2 * -(-m // 16) * (nsmooth + 2), (name, area_comp, nsmooth, m, err.max())
            assert err.max() * np.spacing(0.1) <= stage_bound(info, nsmooth, 0.1), (name, area_comp, nsmooth, err.max())
            out, info = R.smooth(nodes, e, 3, area_comp, nsmooth, detail=True)
            used = np.unique(e - 1)
            lo, hi = nodes[used, 3].min(), nodes[used, 3].max()
            tol = stage_bound(info, nsmooth, max(abs(lo), abs(hi)))
            assert lo - tol <= out[used, 3].min() and out[used, 3].max() <= hi + tol, (name, area_comp, nsmooth)
            # smoothing contracts: the spread over the elements never grows
            q0 = R.smooth(nodes, e, 3, area_comp, 0, detail=True)[1]["q"]
            assert info["q"].max() - info["q"].min() <= (q0.max() - q0.min()) + tol


@pytest.mark.parametrize("name", ["octahedron", "fan65", "strip257", "grid12_permuted"])
def test_permuting_the_elements_changes_only_the_order_of_additions(name):
    nodes, e = SC.structure(name)
    perm = np.random.default_rng(5).permutation(len(e))
    inv = np.argsort(perm)  # old id -> new id
    for area_comp in SC.WEIGHTS:
        a, ia = R.smooth(nodes, e, 3, area_comp, 2, detail=True)
        b, ib = R.smooth(nodes, e[perm], 3, area_comp, 2, detail=True)
        assert u64(ib["w"]).tolist() == u64(ia["w"][perm]).tolist()  # per element: no order in it
        for k, old in enumerate(perm):
            mine = ib["nbr_adj"][ib["nbr_off"][k]:ib["nbr_off"][k + 1]]
            theirs = ia["nbr_adj"][ia["nbr_off"][old]:ia["nbr_off"][old + 1]]
            assert mine.tolist() == sorted(inv[theirs].tolist())  # the same set, ascending in the new ids
        tol = stage_bound(ia, 2, np.abs(nodes[:, 3]).max())
        assert np.abs(a[:, 3] - b[:, 3]).max() <= 2 * tol and np.abs(ia["q"][perm] - ib["q"]).max() <= 2 * tol
        same = R.smooth(nodes, e[np.arange(len(e))], 3, area_comp, 2)
        assert u64(same).tolist() == u64(a).tolist()


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_show(mistake):
    """each mistake changes the bytes of at least the cases named here"""
    where = {"running_area": ["edge_pair", "grid12_permuted"], "gauss_seidel": ["edge_pair", "grid12_permuted"], "no_self": ["edge_pair", "grid12_permuted"],
             "edge_twice": ["edge_pair", "grid12_permuted"], "descending": ["fan65", "grid12_permuted"], "by_element": ["vertex_pair", "grid12_permuted"]}[mistake]
    for name in where:
        nodes, e = SC.structure(name)
        for area_comp in SC.WEIGHTS:
            good = R.smooth(nodes, e, 3, area_comp, 2)
            bad = R.smooth(nodes, e, 3, area_comp, 2, mistake=mistake)
            assert u64(good).tolist() != u64(bad).tolist(), (mistake, name, area_comp)
    if mistake in ("running_area", "by_element"):  # these show without an iteration
        nodes, e = SC.hand_surface()
        assert R.smooth(nodes, e, 3, 4, 0, mistake=mistake)[:, 3].tolist() != SC.HAND[(4, 0)]
    if mistake in ("gauss_seidel", "no_self", "edge_twice"):  # these need one; a descending order shows only in the rounding
        nodes, e = SC.hand_surface()
        nodes = nodes.copy()
        nodes[8, 4] = 19.0  # w of the last element: 7, so that the pair on one edge has W = 8
        assert R.smooth(nodes, e, 3, 4, 1)[5:, 3].tolist() == [6.5] * 4 and R.smooth(nodes, e, 3, 4, 1, mistake=mistake)[5:, 3].tolist() != [6.5] * 4


def test_nan_reaches_exactly_k_plus_one_rings():
    for name in ("nan_n0", "nan_n1", "nan_n2", "nan_n4"):
        nodes, e, comp, area_comp, k = SC.value_case(name)
        out = R.smooth(nodes, e, comp, area_comp, k)
        dist = SC.node_rings(e, len(nodes), SC.NAN_NODE)
        assert np.isnan(out[:, comp]).tolist() == [0 <= d <= k + 1 for d in dist], name
        assert 0 < np.isnan(out[:, comp]).sum() < len(nodes)


def test_guards_keep_the_value():
    nodes, e, comp, area_comp, k = SC.value_case("zero_area_n2")
    out, info = R.smooth(nodes, e, comp, area_comp, k, detail=True)
    assert info["written"] == 0 and u64(out).tolist() == u64(nodes).tolist() and not info["w"].any()
    nodes, e, comp, area_comp, k = SC.value_case("signed_weights_n2")
    out, info = R.smooth(nodes, e, comp, area_comp, k, detail=True)
    assert 0 < info["written"] < len(nodes) and (info["w"] < 0).any() and (info["w"] == 0).any()
    nodes, e, comp, area_comp, k = SC.value_case("neg_zero_inf_n1")
    out = R.smooth(nodes, e, comp, area_comp, k)
    assert u64(out[:16, 3]).tolist() == [0x8000000000000000] * 16 and np.isposinf(out[16:, 3]).any() and np.isfinite(out[16:, 3]).any()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_entries_are_declared_and_bound():
    from peleanalysis_amd import capi
    names = ("pa_surfsmooth_run", "pa_surfsmooth_read")
    declared = capi.declared_symbols()
    assert set(names) <= set(declared) and sorted(n for n in declared if n.startswith("pa_surfsmooth")) == sorted(names)
    lib = capi.load_library()
    for n in names:
        assert n in lib._pa_signatures and n not in lib._pa_missing and hasattr(lib, n), n
    assert callable(capi.Surf.smooth) and callable(capi.Surf.smooth_read)
    assert capi.Surf.LAUNCH[8] == ("smooth", "elements", "incidence", "neighbours", "iterations", "nodes_written", "max_neighbours", "kernels")
    for f in ("smoothMEF3d.ex", "surfDATtoMEF3d.ex"):
        assert os.access(os.path.join(BIN, f), os.X_OK), f


# ------------------------------------------------------------------------------------------------ surfDATtoMEF3d.ex
def _run(exe, args, cwd, bindir=BIN):
    return subprocess.run([os.path.join(bindir, exe)] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.fixture(scope="module")
def asan_tool():
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "-s", "bin_asan/surfDATtoMEF3d.ex"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return "surfDATtoMEF3d.ex"


def _both(args, cwd, asan_tool):
    """the tool, then its sanitizer build on the same input as a program of its own, in the inherited environment (no sanitizer runtime
    is preloaded for it): -> the plain run"""
    out = _run("surfDATtoMEF3d.ex", args, cwd)
    keep = {f: open(os.path.join(cwd, f), "rb").read() for f in os.listdir(cwd) if f.endswith(".mef")}
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    san = subprocess.run([os.path.join(BIN_ASAN, asan_tool)] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True, timeout=120, env=env)
    assert "Sanitizer" not in san.stderr and "runtime error" not in san.stderr, san.stderr[-3000:]
    assert san.returncode == out.returncode and san.stdout == out.stdout, (san.returncode, out.returncode, san.stderr[-2000:])
    for f, b in keep.items():
        assert open(os.path.join(cwd, f), "rb").read() == b, f
    return out


@pytest.mark.parametrize("name", ["tetrahedron", "fan65", "grid12_permuted"])
def test_dat_round_trip(tmp_path, asan_tool, name):
    nodes, e = SC.structure(name)
    names = ["X", "Y", "Z", "curv", "area"]
    with open(tmp_path / "a.mef", "wb") as fh:
        fh.write(R.mef_bytes(nodes, e, "flame 0.125", names))
    assert _run("surfMEFtoDAT3d.ex", ["infile=a.mef"], tmp_path).returncode == 0
    text = open(tmp_path / "a.dat").read()
    assert text == R.dat_text(nodes, e, "flame 0.125", names)
    os.rename(tmp_path / "a.mef", tmp_path / "first.mef")
    out = _both(["infile=a.dat"], tmp_path, asan_tool)  # the default outfile: a.mef
    assert out.returncode == 0, out.stderr
    files, lines = R.parse_dat(text, "a.mef")
    assert out.stdout.split("\n") == lines + [""] and len(files) == 1
    got = open(tmp_path / "a.mef", "rb").read()
    assert got == files[0][1]
    # the nodes are the float() of the printed text, the elements exact, the title without its quotes
    printed = np.array([[float(t) for t in ln.split()] for ln in text.split("\n")[2:2 + len(nodes)]])
    assert got == R.mef_bytes(printed, e, "flame 0.125", names)
    # ... so a second round trip changes nothing
    assert _run("surfMEFtoDAT3d.ex", ["infile=a.mef", "outfile=b.dat"], tmp_path).returncode == 0
    assert open(tmp_path / "b.dat").read() == text
    out = _both(["infile=b.dat", "outfile=c.mef"], tmp_path, asan_tool)
    assert out.returncode == 0 and open(tmp_path / "c.mef", "rb").read() == got


TWO_ZONES = """TITLE = "two patches"
VARIABLES = X, Y
  Z  "curv"
ZONE T="first one", N=4, E=2,
  F=FEPOINT, ET=TRIANGLE
0, 0, 0, 1.5
1 0 0 -2.5e-3
0,1,0,1e300
1 1 0.5 nan
1 2 3
4, 3, 2

ZONE T=second N=3 E=1 F=FEPOINT ET=TRIANGLE
 0 0 0 7
 0 3 0 8 extra
 4 0 0 9
 3 2 1
ZONE N=3, E=0, ET=TRIANGLE
0 0 0 0
1 0 0 0
0 1 0 0
"""


def test_dat_zones_commas_and_a_variables_list_over_two_lines(tmp_path, asan_tool):
    with open(tmp_path / "in.v2.dat", "w") as fh:
        fh.write(TWO_ZONES)
    files, lines = R.parse_dat(TWO_ZONES, "in.v2.mef")
    assert [f for f, _ in files] == ["in.v2.mef", "in.v2_1.mef", "in.v2_2.mef"] and lines[1] == "zoneID, area = 1, 6" and lines[2] == "zoneID, area = 2, 0"
    assert files[0][1].startswith(b'first one\nX Y Z "curv"\n2 3\n') and files[1][1].startswith(b"second\n") and files[2][1].startswith(b"LabelHere\n")
    out = _both(["infile=in.v2.dat"], tmp_path, asan_tool)
    assert out.returncode == 0 and out.stdout.split("\n") == lines + [""], out.stderr
    for f, b in files:
        assert open(tmp_path / f, "rb").read() == b, f
    files, lines = R.parse_dat(TWO_ZONES, "out")  # an outfile without .mef
    out = _both(["infile=in.v2.dat", "outfile=out"], tmp_path, asan_tool)
    assert out.returncode == 0 and [f for f, _ in files] == ["out", "out_1.mef", "out_2.mef"]
    for f, b in files:
        assert open(tmp_path / f, "rb").read() == b, f


ABORTS = {
    "quads": (lambda t: t.replace("ET=TRIANGLE\n0, 0", "ET=QUADRILATERAL\n0, 0"), "element type QUADRILATERAL is not TRIANGLE"),
    "no_et": (lambda t: t.replace("  F=FEPOINT, ET=TRIANGLE\n", "  F=FEPOINT\n"), "element type undefined is not TRIANGLE"),
    "short_node_line": (lambda t: t.replace("1 0 0 -2.5e-3\n", "1 0 0\n"), "node line 2 has 3 values, not 4"),
    "short_element_line": (lambda t: t.replace("4, 3, 2\n", "4, 3\n"), "element line 2 has 2 node ids, not 3"),
    "node_id_0": (lambda t: t.replace("1 2 3\n", "1 0 3\n"), "element 1 names a node that does not exist"),
    "node_id_past_n": (lambda t: t.replace("4, 3, 2\n", "5, 3, 2\n"), "element 2 names a node that does not exist"),
    "no_n": (lambda t: t.replace("N=4, ", ""), "no node count N in the ZONE header"),
    "no_e": (lambda t: t.replace("E=2,", ""), "no element count E in the ZONE header"),
    "truncated": (lambda t: t[:t.index(" 4 0 0 9")], "the file ends after 2 of 4 data lines"),
    "truncated_in_zone_0": (lambda t: t[:t.index("1 2 3\n")] + "1 2 3\n", "the file ends after 5 of 6 data lines"),
    "not_a_number": (lambda t: t.replace("1 1 0.5 nan", "1 1 0.5 abc"), "is not a number"),
    "underscore_in_a_number": (lambda t: t.replace("1 1 0.5 nan", "1 1 0.5 1_0"), "is not a number"),  # float() would take it
    "hexadecimal_float": (lambda t: t.replace("1 1 0.5 nan", "1 1 0.5 0x1p3"), "is not a number"),     # strtod would take it
    "nan_with_a_payload": (lambda t: t.replace("1 1 0.5 nan", "1 1 0.5 nan(7)"), "is not a number"),
    "underscore_in_a_node_id": (lambda t: t.replace("4, 3, 2\n", "4, 3, 0_2\n"), "element 2 names a node that does not exist"),
    "no_zone": (lambda t: t[:t.index("ZONE")], "has no ZONE line"),
    "no_variables": (lambda t: t.replace("VARIABLES = ", ""), "has no VARIABLES list"),
    "two_variables": (lambda t: t.replace('  Z  "curv"\n', ""), "needs x, y, z as the first three variables"),
    "text_behind_a_zone": (lambda t: t.replace("\nZONE T=second", "\nsomething\nZONE T=second"), "expected a ZONE line"),
}


@pytest.mark.parametrize("name", list(ABORTS))
def test_dat_aborts_by_message(tmp_path, asan_tool, name):
    change, message = ABORTS[name]
    text = change(TWO_ZONES)
    assert text != TWO_ZONES
    with open(tmp_path / "in.dat", "w") as fh:
        fh.write(text)
    with pytest.raises(R.DatError, match=message.replace("(", r"\(")) as err:
        R.parse_dat(text, "in.mef")
    assert message in str(err.value)
    out = _both(["infile=in.dat"], tmp_path, asan_tool)
    assert out.returncode == 134 and message in out.stderr, out.stderr
    out = _run("surfDATtoMEF3d.ex", ["infile=missing.dat"], tmp_path)
    assert out.returncode == 134 and "Unable to open file" in out.stderr
