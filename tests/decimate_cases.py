"""Mesh builders and the case matrix of the decimator tests (tests/test_decimate_ref.py on the CPU, tests/test_gpu_decimate.py on the
GPU): the smallest meshes at which each rule of the algorithm can still go wrong, one named case per rule.  A mesh is
(xyz [N][3] float64, elts [M][3] int32, 1-based, outward orientation where the surface is closed)."""
import functools

import numpy as np


def _mesh(xyz, faces0):
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
    elts = np.ascontiguousarray(np.asarray(faces0, dtype=np.int32).reshape(-1, 3) + 1)
    xyz.setflags(write=False)
    elts.setflags(write=False)
    return xyz, elts


def tetrahedron():
    v = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
    return _mesh(v, [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])  # normals point away from the centre


def octahedron():
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return _mesh(v, f)


@functools.lru_cache(maxsize=None)
def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """20 * 4^level faces: 320 at level 2, 1280 at level 3 (642 vertices, 1920 edges: more than a block of 256 and a wave of 64)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid = {}

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        g = []
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return _mesh(np.array(v) * radius + np.array(centre), f)


def grid(n=8):
    """the unit square as n x n quads of side 1 / n (exact in binary for n = 8), each split along the same diagonal, z = 0"""
    xyz = [(i / n, j / n, 0.0) for j in range(n + 1) for i in range(n + 1)]
    f = []
    for j in range(n):
        for i in range(n):
            p = j * (n + 1) + i
            f += [(p, p + 1, p + n + 2), (p, p + n + 2, p + n + 1)]
    return _mesh(xyz, f)


def cylinder(nseg=16, nring=5):
    """an open cylinder of radius 1: nring rings of nseg vertices, two boundary loops"""
    xyz = [(np.cos(2 * np.pi * s / nseg), np.sin(2 * np.pi * s / nseg), 0.5 * r) for r in range(nring) for s in range(nseg)]
    f = []
    for r in range(nring - 1):
        for s in range(nseg):
            a, b = r * nseg + s, r * nseg + (s + 1) % nseg
            f += [(a, b, b + nseg), (a, b + nseg, a + nseg)]
    return _mesh(xyz, f)


def hub_disk(valence=100):
    """two rings around one hub of the given valence, slightly domed"""
    xyz = [(0.0, 0.0, 0.2)]
    for rad, z in ((1.0, 0.1), (2.0, 0.0)):
        xyz += [(rad * np.cos(2 * np.pi * s / valence), rad * np.sin(2 * np.pi * s / valence), z) for s in range(valence)]
    f = []
    for s in range(valence):
        a, b = 1 + s, 1 + (s + 1) % valence
        f += [(0, a, b), (a, a + valence, b + valence), (a, b + valence, b)]
    return _mesh(xyz, f)


def two_spheres():
    x1, e1 = icosphere(1)
    x2, e2 = icosphere(2, 0.5, (3.0, 0.0, 0.0))
    return _mesh(np.vstack([x1, x2]), np.vstack([e1 - 1, e2 - 1 + len(x1)]))


def sphere_with_fin():
    """an icosphere with a third triangle glued onto the edge of its first face: that edge has three faces (locked, with both ends)"""
    x, e = icosphere(2)
    a, b = e[0, 0] - 1, e[0, 1] - 1
    tip = 1.5 * (x[a] + x[b]) / 2
    return _mesh(np.vstack([x, tip]), np.vstack([e - 1, [(a, b, len(x))]]))


def with_zero_area_face():
    """the flat grid plus a face whose three corners lie on one line (the collinear boundary nodes 0, 1, 2)"""
    x, e = grid(4)
    return _mesh(x, np.vstack([e - 1, [(0, 2, 1)]]))


def with_unused_node():
    x, e = icosphere(1)
    x = np.vstack([x[:5], [(9.0, 9.0, 9.0)], x[5:]])
    f = e - 1
    return _mesh(x, np.where(f >= 5, f + 1, f))


def octahedron_4cycle():
    """an octahedron whose equator 0-1-2-3 has two short opposite edges (0, 1) and (2, 3) of equal cost (point symmetry): the two
    cheapest edges of the first round.  Vertex 1 is a neighbour of vertex 2, so only one of them may be contracted in a round;
    contracting both pinches the surface along the equator (an edge with four faces)"""
    v = [(1, 0, 0), (0.9, 0.3, 0), (-1, 0, 0), (-0.9, -0.3, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4), (1, 0, 5), (2, 1, 5), (3, 2, 5), (0, 3, 5)]
    return _mesh(v, f)


def reflex_fan():
    """a flat fan around vertex 1 whose ring 0-2-3-4-5 has a reflex corner at vertex 2: moving the centre onto vertex 0 turns face
    (1, 2, 3) over.  With -O 0 -B 0 every cost is exactly 0, the endpoint chosen is the lower id, and edge (0, 1) holds the smallest
    key: the flip test alone keeps it from being contracted"""
    v = [(3, 0, 0), (0, 0, 0), (1, 1, 0), (0, 3, 0), (-3, 0, 0), (0, -3, 0)]
    return _mesh(v, [(1, 0, 2), (1, 2, 3), (1, 3, 4), (1, 4, 5), (1, 5, 0)])


# name: (builder, face target, options)
CASES = {
    "tetrahedron": (tetrahedron, 2, {}),
    "octahedron_to_6": (octahedron, 6, {}),
    "ico320_half": (lambda: icosphere(2), 160, {}),
    "ico320_tenth": (lambda: icosphere(2), 32, {}),
    "ico320_to_20": (lambda: icosphere(2), 20, {}),
    "ico1280_half": (lambda: icosphere(3), 640, {}),
    "ico1280_tenth": (lambda: icosphere(3), 128, {}),
    "ico1280_to_20": (lambda: icosphere(3), 20, {}),
    "grid8_O1": (grid, 8, dict(placement=1)),
    "cylinder": (cylinder, 40, {}),
    "hub100": (hub_disk, 60, {}),
    "two_spheres": (two_spheres, 100, {}),
    "fin_locked_edge": (sphere_with_fin, 60, {}),
    "zero_area_face": (with_zero_area_face, 10, {}),
    "unused_node": (with_unused_node, 40, {}),
    "target_ge_nfaces": (with_unused_node, 80, {}),
    "target_0": (lambda: icosphere(1), 0, {}),
    "ico320_O0": (lambda: icosphere(2), 100, dict(placement=0)),
    "ico320_O1": (lambda: icosphere(2), 100, dict(placement=1)),
    "ico320_O3_W0": (lambda: icosphere(2), 100, dict(placement=3, weighting=0)),
    "cylinder_W0": (cylinder, 60, dict(weighting=0)),
    "cylinder_B0": (cylinder, 60, dict(boundary_weight=0.0)),
    "octa_4cycle": (octahedron_4cycle, 4, {}),
    "reflex_fan": (reflex_fan, 3, dict(placement=0, boundary_weight=0.0)),
}
CLOSED = ("tetrahedron", "octahedron_to_6", "ico320_half", "ico320_tenth", "ico320_to_20", "ico1280_half", "ico1280_tenth", "ico1280_to_20", "two_spheres",
          "unused_node", "target_ge_nfaces", "target_0", "ico320_O0", "ico320_O1", "ico320_O3_W0", "octa_4cycle")


@functools.lru_cache(maxsize=None)
def mesh(name):
    return CASES[name][0]()


def options(name):
    o = dict(boundary_weight=1000.0, weighting=1, placement=3)
    o.update(CASES[name][2])
    return o
