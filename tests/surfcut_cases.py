"""The case matrix of the surface cutting and trimming tests (tests/test_surfcut_ref.py on the CPU, tests/test_gpu_surfcut.py on the
GPU): the smallest surfaces at which each rule of sliceMEF.cpp / trimMEFgen.cpp can still go wrong, one named case per rule.  A
surface is (nodes [N][ncomp >= 3] float64, elts [M][3] int32, 1-based); node fields beyond x, y, z are random doubles (seeded) unless a
case states them.  SLICES: name -> (builder, [(comp, location), ...]).  TRIMS: name -> (builder, dict(conds, rxy, sign_rxy)).
The largest inputs are the 5120-face sphere and the 64 x 64 grid."""
import functools

import numpy as np

import decimate_cases as DC


def _surf(nodes, elts1):
    nodes = np.ascontiguousarray(nodes, dtype=np.float64)
    elts1 = np.ascontiguousarray(np.asarray(elts1, dtype=np.int32).reshape(-1, 3))
    nodes.setflags(write=False)
    elts1.setflags(write=False)
    return nodes, elts1


def with_fields(mesh, ncomp, seed):
    """x, y, z + (ncomp - 3) random fields in (-1, 1)"""
    xyz, e = mesh
    rng = np.random.default_rng(seed)
    return _surf(np.hstack([xyz, rng.uniform(-1.0, 1.0, size=(len(xyz), ncomp - 3))]), e)


def triangle(case):
    """one triangle whose field (component 3) puts it in the given case at location 0: bit q set <-> node q below"""
    rng = np.random.default_rng(100 + case)
    nodes = rng.uniform(-1.0, 1.0, size=(3, 5))
    mag = rng.uniform(0.1, 1.0, size=3)
    nodes[:, 3] = [(-mag[q] if (case >> q) & 1 else mag[q]) for q in range(3)]
    return _surf(nodes, [(1, 2, 3)])


def shared_edge(order):
    """A = (0,1,2) asks for edge {0,1} as (0,1) (node 0 is its apex), B = (1,0,3) as (1,0) (node 1 is its apex); location 0.1"""
    rng = np.random.default_rng(7)
    nodes = rng.uniform(-1.0, 1.0, size=(4, 5))
    nodes[:, 3] = [-0.3, 0.7, 0.9, -0.6]
    A, B = (1, 2, 3), (2, 1, 4)
    return _surf(nodes, [A, B] if order == "ab" else [B, A])


def eps_triangle(v0, v1, v2=3.0):
    """one triangle with the given values of component 3; location 1.0"""
    rng = np.random.default_rng(11)
    nodes = rng.uniform(-1.0, 1.0, size=(3, 5))
    nodes[:, 3] = [v0, v1, v2]
    return _surf(nodes, [(1, 2, 3)])


def octahedron():
    return _surf(*DC.octahedron())


@functools.lru_cache(maxsize=None)
def grid(n, ncomp=5):
    """the open n x n patch; component 3 = y - (x - 0.5)^2 (its contour 0.1 is an open line whose lowest point, where the element order
    first meets it, is its middle); the rest random"""
    xyz, e = DC.grid(n)
    rng = np.random.default_rng(20 + n)
    f = rng.uniform(-1.0, 1.0, size=(len(xyz), ncomp - 3))
    f[:, 0] = xyz[:, 1] - (xyz[:, 0] - 0.5) * (xyz[:, 0] - 0.5)
    return _surf(np.hstack([xyz, f]), e)


@functools.lru_cache(maxsize=None)
def ico(level, ncomp):
    return with_fields(DC.icosphere(level), ncomp, 30 + level)


def ico_plus3():
    """1283 faces: no multiple of a wavefront or a workgroup"""
    nodes, e = ico(3, 4)
    return _surf(nodes, np.vstack([e, e[[5, 700, 1279]][:, [1, 2, 0]]]))


def fin():
    """three triangles on one edge: the contour between the edge's ends has a vertex of degree 3 there"""
    xyz, e = DC.sphere_with_fin()
    return with_fields((xyz, e), 4, 41)


def fin_cut():
    nodes, e = fin()
    a, b = e[0, 0] - 1, e[0, 1] - 1
    d = int(np.argmax(np.abs(nodes[a, :3] - nodes[b, :3])))
    return d, 0.5 * (nodes[a, d] + nodes[b, d])


def duplicated():
    """the 4 x 4 patch with element 5 twice: duplicate segments"""
    nodes, e = grid(4)
    return _surf(nodes, np.vstack([e, e[5:6]]))


def two_spheres():
    return with_fields(DC.two_spheres(), 4, 43)


_T = {("tri_case%d" % c): ((lambda c=c: triangle(c)), [(3, 0.0)]) for c in range(8)}
_V = 1.0
SLICES = dict(_T)
SLICES.update({
    "shared_edge_ab": (lambda: shared_edge("ab"), [(3, 0.1)]),
    "shared_edge_ba": (lambda: shared_edge("ba"), [(3, 0.1)]),
    "node_on_location": (lambda: eps_triangle(_V, 2.0, -1.0), [(3, _V)]),           # node 0 is not below; cut edges (2,0) and (2,1)
    "eps1_inside": (lambda: eps_triangle(_V - 0.5e-8, 2.0), [(3, _V)]),            # |val - v1| < 1e-8: node p1
    "eps1_outside": (lambda: eps_triangle(_V - 2.0e-8, 2.0), [(3, _V)]),
    "eps2_inside": (lambda: eps_triangle(0.0, _V + 0.5e-8), [(3, _V)]),            # |val - v2| < 1e-8: node p2
    "eps2_outside": (lambda: eps_triangle(0.0, _V + 2.0e-8), [(3, _V)]),
    "eps_both": (lambda: eps_triangle(_V - 0.3e-8, _V + 0.3e-8), [(3, _V)]),      # both ends within 1e-8: the first test wins
    # |v1 - v2| < 1e-8 with the location between them puts |val - v1| below 1e-8 as well, so the third test cannot be the one that
    # decides on a cut edge; these two sit on either side of it (test_surfcut_ref.py calls the branch directly)
    "eps3_inside": (lambda: eps_triangle(_V - 0.45e-8, _V + 0.45e-8), [(3, _V)]),
    "eps3_outside": (lambda: eps_triangle(_V - 1.01e-8, _V + 1.01e-8), [(3, _V)]),
    "octahedron_z": (octahedron, [(2, 0.5)]),
    "grid8": (lambda: grid(8), [(0, 0.3), (3, 0.1), (4, 0.0)]),
    "grid64": (lambda: grid(64), [(0, 0.3), (3, 0.1), (4, 0.25)]),
    "ico320_c3": (lambda: ico(2, 3), [(0, -0.25), (2, 0.0), (1, 1.0e-3)]),
    "ico1280_c4": (lambda: ico(3, 4), [(0, 0.0), (2, -0.5), (3, 0.2)]),
    "ico5120_c11": (lambda: ico(4, 11), [(2, 0.1), (10, 0.0), (0, -0.7)]),
    "ico1283": (ico_plus3, [(2, 0.05), (3, -0.1)]),
    "fin_degree3": (fin, [fin_cut()]),
    "duplicate_element": (duplicated, [(0, 0.6), (4, 0.0)]),
    "two_spheres": (two_spheres, [(2, 0.1), (0, 3.0), (3, 0.0)]),
    "miss": (lambda: ico(2, 3), [(2, 5.0), (0, -5.0)]),
})

_G8X = 0.125  # the x of the second column of grid(8)
TRIMS = {
    "grid_lt": (lambda: grid(8), dict(conds=[(0, "lt", 0.5)])),
    "grid_le": (lambda: grid(8), dict(conds=[(0, "le", 0.5)])),
    "grid_gt": (lambda: grid(8), dict(conds=[(0, "gt", 0.5)])),
    "grid_ge": (lambda: grid(8), dict(conds=[(0, "ge", 0.5)])),
    "grid_eq_unused": (lambda: grid(8), dict(conds=[(0, "eq", _G8X)])),  # column 1 goes: the 9 nodes of column 0 lose every element
    "grid_two": (lambda: grid(8), dict(conds=[(0, "lt", 0.25), (4, "gt", 0.5)])),
    "grid_rxy": (lambda: grid(8), dict(rxy=0.6, sign_rxy="gt")),
    "grid_rxy_cond": (lambda: grid(8), dict(conds=[(3, "lt", 0.0)], rxy=0.3, sign_rxy="le")),
    "grid_nothing": (lambda: grid(8), dict(conds=[(1, "gt", 5.0)])),
    "grid_everything": (lambda: grid(8), dict(conds=[(1, "ge", 0.0)])),
    "grid64_two": (lambda: grid(64), dict(conds=[(4, "lt", -0.5), (3, "ge", 0.6)])),
    "ico_lt": (lambda: ico(2, 5), dict(conds=[(2, "lt", -0.3)])),
    "ico_le": (lambda: ico(2, 5), dict(conds=[(3, "le", 0.0)])),
    "ico_gt": (lambda: ico(2, 5), dict(conds=[(4, "gt", 0.8)])),
    "ico_ge": (lambda: ico(2, 5), dict(conds=[(0, "ge", 0.5)])),
    "ico_eq": (lambda: ico(2, 5), dict(conds=[(3, "eq", float(ico(2, 5)[0][17, 3]))])),
    "ico_two": (lambda: ico(2, 5), dict(conds=[(2, "gt", 0.7), (3, "lt", -0.8)])),
    "ico_rxy": (lambda: ico(2, 5), dict(rxy=0.5, sign_rxy="lt")),
    "ico_rxy_cond": (lambda: ico(2, 5), dict(conds=[(2, "lt", 0.0)], rxy=0.9, sign_rxy="ge")),
    "ico_nothing": (lambda: ico(2, 5), dict(conds=[(2, "gt", 2.0)])),
    "ico_everything": (lambda: ico(2, 5), dict(rxy=0.0, sign_rxy="ge")),
    "ico1283_unused": (ico_plus3, dict(conds=[(3, "gt", 0.0)])),
}
# trim, then slice the trimmed surface without leaving the device: (trim case, comp, location)
TRIM_THEN_SLICE = [("grid_gt", 1, 0.3), ("ico_lt", 0, 0.1), ("grid64_two", 3, 0.1), ("ico1283_unused", 2, 0.2)]


@functools.lru_cache(maxsize=None)
def slice_surface(name):
    return SLICES[name][0]()


@functools.lru_cache(maxsize=None)
def trim_surface(name):
    return TRIMS[name][0]()


def trim_args(name):
    a = dict(conds=[], rxy=-1.0, sign_rxy="lt")
    a.update(TRIMS[name][1])
    return a


def random_soup(seed, nverts, nsegs, max_degree=4):
    """a seeded random segment list for the line assembly: vertex degrees up to max_degree, duplicates and both orientations included"""
    rng = np.random.default_rng(seed)
    deg = np.zeros(nverts, dtype=np.int64)
    segs = []
    for _ in range(20 * nsegs):  # a saturated soup ends short of nsegs
        if len(segs) == nsegs:
            break
        if segs and rng.random() < 0.1:
            l, r = segs[int(rng.integers(len(segs)))]
            if rng.random() < 0.5:
                l, r = r, l
        else:
            l, r = (int(v) for v in rng.integers(nverts, size=2))
        if l == r or deg[l] >= max_degree or deg[r] >= max_degree:
            continue
        deg[l] += 1
        deg[r] += 1
        segs.append((l, r))
    return np.array(segs, dtype=np.int32).reshape(-1, 2)
