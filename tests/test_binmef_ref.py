"""CPU tier: the restatement of binMEF.cpp (tests/binmef_ref.py) against known answers -- the comparison with the reference's compiled
arithmetic and its golden file is tests/test_surf_reference_pin.py -- and the C ABI of the surface PDFs (pa_surfbin_*): declared in the
header, exported by the library.
The pure-host entry pa_surfbin_max_area is compared with the restatement's triangle areas."""
import collections
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import binmef_ref as B
from peleanalysis_amd import capi

EPS = 2.0 ** -52


def test_reference_self_test_square():
    """binMEF.cpp:349-362 (disabled there): the square [-0.1, 1.1]^2 binned on x and y over [0, 1], one bin each:
    'Total area of this surface: 1.44 (sum of bins: 1)'"""
    nodes = np.array([[-.1, -.1, 0], [1.1, -.1, 0], [1.1, 1.1, 0], [-.1, 1.1, 0]])
    elts = np.array([[1, 2, 3], [1, 3, 4]])
    R = B.bin_surface(nodes, elts, (0, 1), (0, 0), (1, 1), (1, 1))
    total = 0.0
    for a in R.elem_areas:
        total += a
    area, hits = R.table_serial()
    assert total == 1.4400000000000004 and area.tolist() == [1.0]
    assert R.n_my == hits[0] == len(R.areas) and R.outside == [] and R.nonfinite == 0
    out, err, fab, s = B.tool_output(area, hits, (0, 1), (0, 0), (1, 1), (1, 1), total)
    assert out == "0.5 0.5 1\n" and s == 1.0 and fab is None
    assert err == ["number of nonempty bins: 1", "Total area of this surface: 1.44 (sum of bins: 1)"]


def test_planar_triangle_linear_field_trapezoids():
    """the triangle (0,0) (1,0) (0,1) with f = 10 + 4x binned in 5 bins over [10, 14]: the piece with a <= x < b is a trapezoid of area
    (b - a) - (b^2 - a^2) / 2.  Tolerance: a leaf's vertices come from at most `depth` interpolations one after the other, each
    D = A - f (A - C) with f a rounded quotient: 6 roundings of relative size 2^-53 on coordinates of magnitude <= 1 (the field: <= 14,
    scaled back by the bin width 0.8 when it becomes a position: x 17.5); the area of a leaf adds about 10 more, and a bin sums its
    leaves, whose areas add up to at most the triangle's 1/2.  Together: 17.5 * (6 * depth + 10) * 2^-52 * (1/2) per bin."""
    nodes = np.array([[0.0, 0.0, 0.0, 10.0], [1.0, 0.0, 0.0, 14.0], [0.0, 1.0, 0.0, 10.0]])
    for elts in ([[1, 2, 3]], [[2, 3, 1]], [[3, 2, 1]]):
        R = B.bin_surface(nodes, np.array(elts), (3,), (10.0,), (14.0,), (5,))
        area, hits = R.table()
        tol = 17.5 * (6 * R.depth + 10) * EPS * 0.5
        assert R.depth <= 2 * 5 + 2
        for i in range(5):
            a, b = 0.2 * i, 0.2 * (i + 1)
            want = (b - a) - (b * b - a * a) / 2
            assert abs(area[i] - want) <= tol, (i, area[i], want, tol)
        assert np.all(hits > 0) and abs(area.sum() - 0.5) <= 5 * tol
        # a range that cuts the triangle off on both sides: x in [0.25, 0.75] only
        R = B.bin_surface(nodes, np.array(elts), (3,), (11.0,), (13.0,), (2,))
        area, hits = R.table()
        for i, (a, b) in enumerate(((0.25, 0.5), (0.5, 0.75))):
            assert abs(area[i] - ((b - a) - (b * b - a * a) / 2)) <= tol


@pytest.fixture(scope="module")
def sphere8():
    return B.latlong_sphere(8)


def _max_edge(nodes, elts):
    P = nodes[:, :3][np.asarray(elts) - 1]
    return max(float(np.linalg.norm(P[:, a] - P[:, b], axis=1).max()) for a, b in ((0, 1), (1, 2), (2, 0)))


def test_sphere_16x16_against_8x8_in_groups(sphere8):
    """the 16 x 16 bins summed 2 x 2 are the 8 x 8 bins of the same ranges: every second edge of the fine bins IS an edge of the coarse
    ones (dBin halves exactly), and clipping a piecewise linear field at more edges changes the pieces, not the surface they cover.
    The prototype differs by zero; the margin: a vertex of a leaf carries at most 6 * depth roundings of 2^-53 relative to coordinates
    <= 1 (see the planar test), which moves the area of a leaf by at most that times its perimeter <= 3 h, h = the longest element edge;
    a group compares n16 + n8 leaves."""
    nodes, elts = sphere8
    n, bc, mn, mx, nb = B.CASES["n8_16x16"]
    R16 = B.bin_surface(nodes, elts, bc, mn, mx, nb)
    R8 = B.bin_surface(nodes, elts, bc, mn, mx, (8, 8))
    a16, h16 = R16.table()
    a8, h8 = R8.table()
    g16 = a16.reshape(8, 2, 8, 2).sum(axis=(1, 3))
    n16 = h16.reshape(8, 2, 8, 2).sum(axis=(1, 3))
    h = _max_edge(nodes, elts)
    margin = (n16 + h8.reshape(8, 8)) * (6 * max(R16.depth, R8.depth) * 2.0 ** -53) * 3 * h
    assert np.all(np.abs(g16 - a8.reshape(8, 8)) <= margin), float(np.abs(g16 - a8.reshape(8, 8)).max())
    assert np.array_equal(n16 > 0, h8.reshape(8, 8) > 0)
    # the case's ranges cut part of the surface off (T reaches 300 and 2000, s exceeds 0.9): strictly less than the whole.  Ranges
    # that hold every value of both fields: the bins add up to the surface, the 2n pole triangles (zero area) excepted
    tot = math.fsum(R16.elem_areas)
    assert 0.25 * tot < math.fsum(R16.areas) < 0.75 * tot
    Rall = B.bin_surface(nodes, elts, bc, (0.0, -2.0), (3000.0, 2.0), nb)
    assert abs(math.fsum(Rall.areas) - tot) <= Rall.n_my * (6 * Rall.depth * 2.0 ** -53) * 3 * h
    assert abs(tot - 4 * math.pi) < 0.15 * 4 * math.pi and len(R16.elem_areas) == 256
    assert min(R16.areas) >= 1e-20 and R16.n_my == len(R16.areas) > 256


def test_condition_signs(sphere8):
    """condSgn +1 / -1 / 0 (:206-226) on z against 0: the leaves are those of the unconditioned run, each either in its bin or in
    areaOutsideCondition; no vertex has z == 0 (the equator row holds cos(pi/2) = 6e-17), so sgn 0 accepts nothing"""
    nodes, elts = sphere8
    n, bc, mn, mx, nb = B.CASES["n8_16x16"]
    R = B.bin_surface(nodes, elts, bc, mn, mx, nb)
    got = {}
    for sgn in (-1, 0, 1):
        C_ = B.bin_surface(nodes, elts, bc, mn, mx, nb, cond_apply=True, cond_comp=2, cond_val=0.0, cond_sgn=sgn)
        assert sorted(C_.areas + C_.outside) == sorted(R.areas) and C_.n_my == R.n_my
        got[sgn] = C_
    assert got[0].areas == [] and len(got[1].areas) > 0 and len(got[-1].areas) > 0
    # strict comparisons: a leaf that touches z = 0 is in neither half
    assert len(got[1].areas) + len(got[-1].areas) < R.n_my
    assert abs(math.fsum(got[1].areas) - math.fsum(got[-1].areas)) < 0.2 * math.fsum(R.areas)
    # sgn 0 accepts where all three vertices hold the value exactly
    flat = np.array([[0.0, 0.0, 0.0, 1.0, 7.0], [1.0, 0.0, 0.0, 2.0, 7.0], [0.0, 1.0, 0.0, 3.0, 7.0]])
    Z = B.bin_surface(flat, np.array([[1, 2, 3]]), (3,), (0.0,), (4.0,), (4,), cond_apply=True, cond_comp=4, cond_val=7.0, cond_sgn=0)
    assert Z.outside == [] and len(Z.areas) == Z.n_my >= 2
    out, err, fab, s = B.tool_output(*Z.table(), (3,), (0.0,), (4.0,), (4,), 0.5, outside_area=0.0)
    assert err[2] == "   area outside condition: 0 (total: %s)" % B.cxx(s)


def test_values_on_edges_and_at_bin_max():
    """getBin (:168-200): an upper-bound search on the edge array -- a value ON an edge belongs to the bin above it, == binMax to the
    last bin, above binMax to nBins, below the first edge to -1"""
    lo = B.bin_edges((0.0,), (1.0,), (4,))
    assert lo == [[0.0, 0.25, 0.5, 0.75]]
    f = lambda v: B.get_bin((v,), (0,), lo, (1.0,))[0]
    assert [f(v) for v in (0.0, 0.25, 0.5, 0.75, 1.0)] == [0, 1, 2, 3, 3]
    assert f(-5e-324) == -1 and f(1.0 + 2 ** -52) == 4 and f(0.25 - 2 ** -54) == 0 and f(0.75 - 2 ** -53) == 2
    # edges that are not representable: binMin + i * dBin, never a division
    lo = B.bin_edges((350.0,), (1950.0,), (128,))[0]
    assert lo[77] == 350.0 + 77 * ((1950.0 - 350.0) / 128) and B.get_bin((lo[77],), (0,), [lo], (1950.0,)) == (77,)
    # a triangle with vertices exactly on an edge and exactly at binMax: all of it is counted, nothing below the edge
    nodes = np.array([[0.0, 0.0, 0.0, 0.25], [1.0, 0.0, 0.0, 1.0], [0.0, 1.0, 0.0, 1.0]])
    R = B.bin_surface(nodes, np.array([[1, 2, 3]]), (3,), (0.0,), (1.0,), (4,))
    area, hits = R.table()
    assert hits[0] == 0 and np.all(hits[1:] > 0) and abs(area.sum() - 0.5) < 64 * EPS
    # a flat triangle AT binMax is one leaf in the last bin
    nodes[:, 3] = 1.0
    R = B.bin_surface(nodes, np.array([[1, 2, 3]]), (3,), (0.0,), (1.0,), (4,))
    assert R.keys == [3] and R.areas == [0.5]


def test_zero_area_elements_and_one_bin(sphere8):
    """the 2n = 16 pole triangles of the lat-long sphere have two coincident vertices: area 0 < areaEps, no leaf.  With one bin over
    everything the other 240 elements are one leaf each, with the element's own area."""
    nodes, elts = sphere8
    n, bc, mn, mx, nb = B.CASES["onebin"]
    R = B.bin_surface(nodes, elts, bc, mn, mx, nb)
    assert len(elts) == 256 and sorted(R.elem_areas)[:16] == [0.0] * 16 and sorted(R.elem_areas)[16] > 1e-3
    assert R.keys == [0] * 240 and R.n_my == 240 and R.areas == [a for a in R.elem_areas if a > 0]
    # areaEps <= 0 lets them through: a touched bin that may hold 0 is still printed (nonempty means touched)
    flat = np.array([[0.0, 0.0, 0.0, 0.5], [0.0, 0.0, 0.0, 0.5], [1.0, 0.0, 0.0, 0.5]])
    Z = B.bin_surface(flat, np.array([[1, 2, 3]]), (3,), (0.0,), (1.0,), (2,), area_eps=0.0)
    area, hits = Z.table()
    assert hits.tolist() == [0, 1] and area.tolist() == [0.0, 0.0]
    out, err, fab, s = B.tool_output(area, hits, (3,), (0.0,), (1.0,), (2,), 0.0)
    assert out == "0.75 0\n" and err[0] == "number of nonempty bins: 1"


def test_surface_out_of_range(sphere8):
    nodes, elts = sphere8
    n, bc, mn, mx, nb = B.CASES["allout"]
    R = B.bin_surface(nodes, elts, bc, mn, mx, nb)
    assert R.keys == [] and R.n_my == 0 and len(R.elem_areas) == 256
    area, hits = R.table()
    out, err, fab, s = B.tool_output(area, hits, bc, mn, mx, nb, math.fsum(R.elem_areas))
    assert out == "" and s == 0.0 and err[0] == "number of nonempty bins: 0" and err[1].endswith("(sum of bins: 0)")
    # partly out: the piece above binMax is cut at binMax (the abin >= nBins branch of findDE / findFG) and dropped
    nodes = np.array([[0.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 4.0], [0.0, 1.0, 0.0, 0.0]])
    R = B.bin_surface(nodes, np.array([[1, 2, 3]]), (3,), (1.0,), (3.0,), (2,))
    area, hits = R.table()
    for i, (a, b) in enumerate(((0.25, 0.5), (0.5, 0.75))):
        assert abs(area[i] - ((b - a) - (b * b - a * a) / 2)) <= 256 * EPS


def test_nonfinite_elements_are_skipped(sphere8):
    nodes, elts = sphere8
    n, bc, mn, mx, nb = B.CASES["n8_16x16"]
    bad = nodes.copy()
    bad[40, 3] = np.nan
    bad[90, 1] = np.inf
    R = B.bin_surface(bad, elts, bc, mn, mx, nb)
    touched = int(np.sum(np.any(np.isin(elts, (41, 91)), axis=1)))
    assert R.nonfinite == touched > 0 and len(R.elem_areas) == 256 - touched
    bad = nodes.copy()
    bad[40, 2] = np.nan  # z is not binned here, but it is a coordinate
    assert B.bin_surface(bad, elts, bc, mn, mx, nb).nonfinite > 0


def test_tool_output_fab_and_bins():
    """dumpFab with two components: component 0 is the FAB's x; normalize multiplies by 1 / binSum (:637); dumpBins (:491-501)"""
    area = np.array([0.0, 0.25, 0.0, 0.5, 0.0, 0.125])  # nbins (2, 3): key = b0 * 3 + b1
    hits = np.array([0, 2, 0, 1, 0, 4])
    out, err, fab, s = B.tool_output(area, hits, (3, 4), (0.0, -1.0), (1.0, 2.0), (2, 3), 1.0, dump_fab=True, normalize=True, dump_bins=True)
    head, data = fab.split(b"\n", 1)
    assert head == (B.FAB_DESC + "((0,0,0) (1,2,0) (0,0,0)) 1").encode() and s == 0.875
    d = np.frombuffer(data, "<f8").reshape(3, 2)
    r = 1. / 0.875
    assert d.tolist() == [[0.0, 0.5 * r], [0.25 * r, 0.0], [0.0, 0.125 * r]]
    assert out == ("bin: 3 bounds: \n         bin: [0,0.5]\n         bin: [0.5,1]\n\n"
                   "bin: 4 bounds: \n         bin: [-1,0]\n         bin: [0,1]\n         bin: [1,2]\n\n")
    out, err, fab, s = B.tool_output(area, hits, (3, 4), (0.0, -1.0), (1.0, 2.0), (2, 3), 1.0)
    assert out == "0.25 0.5 0.25\n0.75 -0.5 0.5\n0.75 1.5 0.125\n" and fab is None
    # three components are never a .fab
    out3, _, fab3, _ = B.tool_output(np.ones(8), np.ones(8, dtype=int), (0, 1, 2), (0, 0, 0), (1, 1, 1), (2, 2, 2), 8.0, dump_fab=True)
    assert fab3 is None and out3.count("\n") == 8 and out3.startswith("0.25 0.25 0.25 1\n")


def test_surfbin_abi_declared_and_exported(sphere8):
    """the header declares the pa_surfbin_* entry points with their binMEF.cpp citations, the library exports them and the binding
    knows their signatures; the host entry pa_surfbin_max_area is triangleArea (:46-60) over the elements"""
    names = ["pa_surfbin_create", "pa_surfbin_begin", "pa_surfbin_add_surface", "pa_surfbin_read", "pa_surfbin_destroy", "pa_surfbin_max_area"]
    declared = capi.declared_symbols()
    lib = capi.load_library()
    for n in names:
        assert n in declared and hasattr(lib, n) and n in lib._pa_signatures
    import os
    txt = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "peleanalysis_amd.h")).read()
    for cite in ("binMEF.cpp:231-331", "binMEF.cpp:522-540", "binMEF.cpp:594-670", "binMEF.cpp:46-60"):
        assert cite in txt
    assert hasattr(capi, "SurfBin")
    nodes, elts = sphere8
    cols = [np.ascontiguousarray(nodes[:, c]) for c in range(3)]
    pd = C.POINTER(C.c_double)
    e = np.ascontiguousarray(elts, dtype=np.int32)
    got = lib.pa_surfbin_max_area(len(nodes), cols[0].ctypes.data_as(pd), cols[1].ctypes.data_as(pd), cols[2].ctypes.data_as(pd), len(e),
                                  e.ctypes.data_as(C.POINTER(C.c_int32)))
    P = [tuple(r) for r in nodes]
    assert got == max(B.triangle_area(P[a - 1], P[b - 1], P[c - 1]) for a, b, c in elts)
    e2 = e.copy()
    e2[3, 1] = len(nodes) + 1
    assert lib.pa_surfbin_max_area(len(nodes), cols[0].ctypes.data_as(pd), cols[1].ctypes.data_as(pd), cols[2].ctypes.data_as(pd), len(e2),
                                   e2.ctypes.data_as(C.POINTER(C.c_int32))) == -1.0


# ----------------------------------------------------------------------------- the rounds of the kernels, on the host
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _host_build(out, extra=()):
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", *extra,
                           os.path.join(ROOT, "tools", "bench", "binmef_host.hip"), "-o", out])


def _host_run(exe, tmp, nodes, elts, bc, mn, mx, nb, cap, cond=None, expect=0):
    """tools/bench/binmef_host.hip on a surface -> ((key, area bits) sorted, the counters it prints)"""
    nc = len(bc)
    cols = [nodes[:, 0], nodes[:, 1], nodes[:, 2]] + [nodes[:, c] for c in bc] + ([nodes[:, cond[0]]] if cond else [])
    pad = [0.0] * (4 - nc)
    dpar = list(mn) + pad + list(mx) + pad + [float(n) for n in nb] + pad + [cond[1] if cond else 0.0, 1.0e-20, 0.0, 0.0]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("8q", len(nodes), len(elts), nc, 1 if cond else 0, cond[2] if cond else 0, cap, 0, 0))
        f.write(struct.pack("16d", *dpar))
        f.write(np.concatenate(cols).astype("<f8").tobytes())
        f.write(np.ascontiguousarray(elts, dtype="<i4").tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert r.returncode == expect, (r.returncode, r.stdout, r.stderr)
    if expect:
        return None, r.stdout
    w = r.stdout.split()
    d = np.fromfile(fout, dtype="<i8").reshape(-1, 2)
    return d[np.lexsort((d[:, 1], d[:, 0]))], {w[i]: int(w[i + 1]) for i in range(0, len(w), 2)}


def _bits(v):
    return np.float64(v).view(np.int64).item()


def test_host_run_of_the_kernels_rounds(tmp_path):
    """The code the kernels run for one path of the recursion (sb_chain) and the slice rule of the rounds (pa_binmef_slice) are host
    code too: tools/bench/binmef_host.hip drives them through count -> slice -> emit without a device.  Its leaves are the
    restatement's as a multiset, area bits included, for every list capacity; a two-component surface at 128 x 128 bins is worked off
    on lists of 600, 1000 and 1500 items -- 12 to 30 times the children of one item, capacities at which a rule that fills the list
    to the brim cannot take the top item any more -- with the leaves of the default list; only a list below one item's children
    fails.  The sanitizer build runs the sliced cases clean."""
    exe, san = str(tmp_path / "binmef_host"), str(tmp_path / "binmef_host_san")
    _host_build(exe)
    _host_build(san, ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"))
    tmp = str(tmp_path)
    for name, caps, cond in (("n8_16x16", (1 << 19, 2000), None), ("n8_16x16", (1 << 19,), (2, 0.1, 1)), ("n4_128", (1 << 19, 2048, 300), None),
                             ("n6_8x8x8", (1 << 19, 200), None), ("onebin", (1 << 19,), None), ("allout", (64,), None), ("n12_32x32", (1000, 300), None)):
        n, bc, mn, mx, nb = B.CASES[name]
        nodes, elts = B.latlong_sphere(n)
        kw = dict(cond_apply=True, cond_comp=cond[0], cond_val=cond[1], cond_sgn=cond[2]) if cond else {}
        R = B.bin_surface(nodes, elts, bc, mn, mx, nb, **kw)
        nt = int(np.prod(nb))
        want = collections.Counter([(k, _bits(a)) for k, a in zip(R.keys, R.areas)] + [(nt, _bits(a)) for a in R.outside] + [(nt + 1, _bits(a)) for a in R.elem_areas])
        for cap in caps:
            got, cnt = _host_run(san if cap < 1 << 19 else exe, tmp, nodes, elts, bc, mn, mx, nb, cap, cond)
            assert collections.Counter(map(tuple, got.tolist())) == want, (name, cap)
            assert cnt["peak"] <= cap and cnt["flag"] == 0 and (cnt["sliced"] > 0) == (cap < 1 << 19 and name != "allout"), (name, cap, cnt)
    nodes, elts = B.latlong_sphere(24)
    args = ((3, 4), (350.0, -0.9), (1950.0, 0.9), (128, 128))
    full, cfull = _host_run(exe, tmp, nodes, elts, *args, 1 << 19)
    assert cfull["peak"] <= 1 << 19 and cfull["sliced"] > 0  # 3.2 million work items: the default list is sliced too
    for cap in (600, 1000, 1500):
        got, cnt = _host_run(exe, tmp, nodes, elts, *args, cap)
        assert np.array_equal(got, full) and cnt["peak"] <= cap and cnt["items"] == cfull["items"], (cap, cnt)
    _, msg = _host_run(exe, tmp, nodes, elts, *args, 8, expect=2)
    assert msg.startswith("STUCK")
