"""CPU tier of the decimator: the restatement tests/decimate_ref.py is pinned by known answers that do NOT come from it -- topology
(Euler characteristic per component, closedness), the face count, the order of the survivors, the flat grid (z, corners, area), the
locked edge, closed forms of two hand-computed quantities -- and five planted mistakes must each make one of those checks fail."""
import functools
import math

import numpy as np
import pytest

import decimate_cases as DC
import decimate_ref as R

NAMES = list(DC.CASES)


@functools.lru_cache(maxsize=None)
def run(name, mistakes=()):
    x, e = DC.mesh(name)
    d = R.Decimator(x, e, mistakes=mistakes, **DC.options(name))
    d.run(DC.CASES[name][1])
    return d, d.output()


# ---------------------------------------------------------------- the checks (each raises AssertionError)
def components_chi(elts):
    """V - E + F of every connected component, ordered by the component's smallest vertex"""
    parent = {}

    def find(v):
        while parent.setdefault(v, v) != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b, c in elts.tolist():
        parent[find(b)] = find(a)
        parent[find(c)] = find(a)
    comp = {}
    for a, b, c in elts.tolist():
        V, E, F = comp.setdefault(find(a), (set(), set(), [0]))
        V.update((a, b, c))
        E.update((min(u, v), max(u, v)) for u, v in ((a, b), (b, c), (c, a)))
        F[0] += 1
    return [len(V) - len(E) + F[0] for _, (V, E, F) in sorted(comp.items(), key=lambda kv: min(kv[1][0]))]


def check_euler(name, out):
    assert components_chi(out[1]) == components_chi(DC.mesh(name)[1]), name


def check_closed(name, out):
    """checkIso.cpp's rule (:127-149), made strict: every edge is traversed exactly once in each direction"""
    seen = {}
    for a, b, c in out[1].tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            seen[(u, v)] = seen.get((u, v), 0) + 1
    for (u, v), n in seen.items():
        assert n == 1 and seen.get((v, u), 0) == 1, (name, u, v)


def check_count(name, d, out):
    target = DC.CASES[name][1]
    nf = len(DC.mesh(name)[1])
    if target >= nf:
        assert len(out[1]) == nf and d.rounds == 0 and d.message is None, name
    elif d.message is None:
        assert len(out[1]) in (target, target - 1), (name, len(out[1]), target)
    else:
        assert d.message == "no valid contraction left at %d faces" % len(out[1]) and len(out[1]) > target, (name, d.message)


def check_order(name, d, out):
    """the survivors keep their relative input order: the output is the valid faces in slot order over the used vertices in id order"""
    P, F, valid, _ = d.state()
    live = F[valid.astype(bool)]
    used = np.unique(live)
    assert np.array_equal(out[1], np.searchsorted(used, live).astype(np.int32) + 1), name
    assert np.array_equal(out[0].view(np.uint64), P[used].view(np.uint64)), name
    assert np.all(np.diff(used) > 0)


def normals(out):
    p = out[0][out[1] - 1]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])


def check_flat_up(name, out):
    """a planar, counter-clockwise triangulation stays one: every z is exactly 0 and every face normal points up"""
    assert np.all(out[0][:, 2] == 0.0), name
    assert np.all(normals(out)[:, 2] > 0.0), name


def check_grid(name, out):
    """the unit square: z == 0 exactly, the four corners survive, and the triangle areas add up to the square's area 1.  The bound:
    every coordinate is a dyadic rational with few bits (grid points k / 8 and midpoints of such), so each cross product and each
    area 0.5 * |n_z| is exact; what is left is the rounding of the sum of n terms, at most (n - 1) * 2^-53 * A <= n * 2^-52 * A"""
    check_flat_up(name, out)
    pts = {tuple(r) for r in out[0].tolist()}
    for c in ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0)):
        assert c in pts, (name, c)
    n = normals(out)
    area = 0.0
    for a in (0.5 * np.abs(n[:, 2])).tolist():
        area += a
    assert abs(area - 1.0) <= len(n) * 2.0 ** -52 * 1.0, (name, area)


def check_tetrahedron(name, d, out):
    x, e = DC.mesh(name)
    assert d.rounds == 0 and d.message == "no valid contraction left at 4 faces", (name, d.message)
    assert np.array_equal(out[1], e) and np.array_equal(out[0].view(np.uint64), x.view(np.uint64)), name


# ---------------------------------------------------------------- the restatement passes them
@pytest.mark.parametrize("name", NAMES)
def test_topology_count_and_order(name):
    d, out = run(name)
    check_euler(name, out)
    check_count(name, d, out)
    check_order(name, d, out)
    if name in DC.CLOSED:
        check_closed(name, out)
    assert np.isfinite(out[0]).all()


def test_tetrahedron_comes_back_untouched():
    check_tetrahedron("tetrahedron", *run("tetrahedron"))


def test_octahedron_to_6():
    d, out = run("octahedron_to_6")
    assert len(out[1]) == 6 and len(out[0]) == 5 and d.rounds == 1 and d.record() == [12, 0, 12, 1, 1, 1, 2, 6]


def test_flat_grid_keeps_plane_corners_and_area():
    check_grid("grid8_O1", run("grid8_O1")[1])
    out = run("zero_area_face")[1]  # the face without area may survive: no normal points down
    assert np.all(out[0][:, 2] == 0.0) and np.all(normals(out)[:, 2] >= 0.0)


def test_reflex_fan_is_not_turned_over():
    check_flat_up("reflex_fan", run("reflex_fan")[1])


def test_unused_node_and_target_above_the_face_count():
    x, e = DC.mesh("target_ge_nfaces")
    d, out = run("target_ge_nfaces")
    keep = np.delete(np.arange(len(x)), 5)  # node 5 is the one no element names
    assert d.rounds == 0 and np.array_equal(out[0].view(np.uint64), x[keep].view(np.uint64))
    assert np.array_equal(out[1], np.searchsorted(keep, e - 1).astype(np.int32) + 1)


def test_locked_edge_and_its_three_faces_survive():
    x, e = DC.mesh("fin_locked_edge")
    d, out = run("fin_locked_edge")
    a, b = int(e[0, 0]), int(e[0, 1])
    mine = [f for f in e.tolist() if a in f and b in f]
    assert len(mine) == 3 and d.record()[1] == 1
    # both ends are locked: they are in the output with the input's bits (the third vertices of the faces are free to move) ...
    bits = [tuple(r) for r in out[0].view(np.uint64).tolist()]
    na, nb = bits.index(tuple(x[a - 1].view(np.uint64).tolist())) + 1, bits.index(tuple(x[b - 1].view(np.uint64).tolist())) + 1

    def directed(faces, u, v):
        return sorted(sum(1 for q in range(3) if f[q] == u and f[(q + 1) % 3] == v) for f in faces if u in f and v in f)
    # ... and the edge still has its three faces, each traversing it in the direction the input's face did
    theirs = [f for f in out[1].tolist() if na in f and nb in f]
    assert len(theirs) == 3 and directed(theirs, na, nb) == directed(mine, a, b) == [0, 1, 1]
    tip = tuple(x[-1].view(np.uint64).tolist())  # the fin's third vertex has no other face: nothing can move it
    assert tip in bits and any(bits.index(tip) + 1 in f for f in theirs)


def test_hand_computed_quadric_and_cost():
    """closed forms.  Regular tetrahedron (+-1, +-1, +-1), -W 0: the face opposite vertex u lies in the plane u . x + 1 = 0, unit normal
    u / sqrt(3), d = 1 / sqrt(3); the three faces at v are those opposite the other vertices, and sum_u u u^T = 4 I, sum_u u = 0 over
    all four, so Q(v) = ((4 I - v v^T) / 3, -v / 3, 1): for v = (1, 1, 1) the ten entries are 1 -1/3 -1/3 -1/3 1 -1/3 -1/3 1 -1/3 1.
    Octahedron +-e_i, -W 0: the faces are the planes (+-x +- y +- z - 1) / sqrt(3) = 0; contracting the edge from a = e_x to b = e_y
    onto a costs nothing for the four faces at a and (s_x - 1)^2 / 3 for the face at b with sign s_x: 0 + 0 + 4/3 + 4/3 = 8/3; the
    same onto b, and the tie goes to a."""
    x, e = DC.mesh("tetrahedron")
    d = R.Decimator(x, e, weighting=0)
    want = [1.0, -1 / 3, -1 / 3, -1 / 3, 1.0, -1 / 3, -1 / 3, 1.0, -1 / 3, 1.0]
    assert tuple(x[0]) == (1.0, 1.0, 1.0)
    for g, w in zip(d.Q[0], want):
        assert abs(g - w) <= 8 * 2.0 ** -52, (d.Q[0], want)  # three terms of magnitude <= 1/3 each, a few roundings apiece
    x, e = DC.mesh("octahedron_to_6")
    d = R.Decimator(x, e, weighting=0, placement=0)
    eid = d.eid[(0 << 32) | 2]  # vertices 0 = +x and 2 = +y
    q = [d.Q[0][i] + d.Q[2][i] for i in range(10)]
    assert abs(R.qcost(q, d.P[0]) - 8 / 3) <= 16 * 2.0 ** -52 * (8 / 3)
    key, vbar = d._candidate(eid)
    assert vbar == (1.0, 0.0, 0.0) and key & 0xFFFFFFFF == eid
    assert abs((key >> 32) - R.float_bits(8 / 3)) <= 1  # the float nearest the cost, or its neighbour


def test_every_option_changes_the_result():
    """-O 0 / 1 / 3, -W 0 / 1 and -B 0 each reach the kernels: the outputs differ"""
    outs = {n: run(n)[1][0].tobytes() for n in ("ico320_O0", "ico320_O1", "ico320_O3_W0", "cylinder", "cylinder_W0", "cylinder_B0")}
    assert len(set(outs.values())) == len(outs)
    x, e = DC.mesh("ico320_O0")
    pts = {tuple(r) for r in x.tolist()}
    assert all(tuple(r) in pts for r in run("ico320_O0")[1][0].tolist())  # -O 0 only ever keeps input positions


# ---------------------------------------------------------------- planted mistakes: each fails a named check
def test_mistake_link_condition():
    with pytest.raises(AssertionError):
        check_tetrahedron("tetrahedron", *run("tetrahedron", ("no_link",)))
    with pytest.raises(AssertionError):
        check_euler("target_0", run("target_0", ("no_link",))[1])


def test_mistake_flip_test():
    with pytest.raises(AssertionError):
        check_flat_up("reflex_fan", run("reflex_fan", ("no_flip",))[1])


def test_mistake_independence_rule():
    """key == vk[a] == vk[b] (the 1-ring of the edge only) lets both short equator edges go in one round"""
    out = run("octa_4cycle", ("one_ring",))[1]
    with pytest.raises(AssertionError):
        check_closed("octa_4cycle", out)
    with pytest.raises(AssertionError):
        check_euler("octa_4cycle", out)


def test_mistake_boundary_quadric():
    with pytest.raises(AssertionError):
        check_grid("grid8_O1", run("grid8_O1", ("no_boundary",))[1])


def test_mistake_cut_at_R():
    """without the limit at R = valid faces - target.  The prefix rule of step 5 is implied by the budget of step 3, so
    the planted mistake drops both: every independent candidate of a round is applied"""
    d, out = run("ico1280_half", ("no_cut",))
    with pytest.raises(AssertionError):
        check_count("ico1280_half", d, out)


def test_mef_bytes_layout():
    x, e = DC.mesh("octahedron_to_6")
    b = R.mef_bytes(x, e)
    head = b"decimated surface\nX Y Z\n8 3\n" + R.FAB_DESC.encode() + b"((0,0,0) (5,0,0) (0,0,0)) 3\n"
    assert b.startswith(head) and len(b) == len(head) + 6 * 24 + 8 * 12
    assert math.isclose(np.frombuffer(b, "<f8", 18, len(head))[0], 1.0)
