"""The case matrix of the surface smoothing step (tests/test_surfsmooth_ref.py on the CPU, tests/test_gpu_surfsmooth.py on the GPU), all
tiny.  A surface is (nodes [N][5] float64: x, y, z, the field f3, a positive area column f4; elts [M][3] int32, 1-based).

STRUCTURES are crossed with NSMOOTH (both ping-pong parities) and WEIGHTS (the triangles' own areas, and the area column).
VALUES are cases of their own: (builder, comp, area_comp, nsmooth).  HAND has answers worked out by hand; verify_hand() checks with
fractions.Fraction that every operation of them is exact in doubles, so that the hand answers are the bytes."""
import functools
import math
from fractions import Fraction

import numpy as np

NSMOOTH = (0, 1, 2, 5)
WEIGHTS = (-1, 4)
COMP = 3


def _surface(xyz, elts1, seed):
    """the field and the area column: seeded, the areas in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    nodes = np.concatenate([xyz, rng.standard_normal((len(xyz), 1)), 0.5 + rng.random((len(xyz), 1))], axis=1)
    return np.ascontiguousarray(nodes), np.asarray(elts1, dtype=np.int32).reshape(-1, 3)


def _jitter(n, seed):
    return 0.05 * np.random.default_rng(seed).standard_normal((n, 3))


def one_triangle():
    return _surface([[0, 0, 0], [1, 0, 0.2], [0, 1, 0.1]], [[1, 2, 3]], 1)


def edge_pair():
    return _surface([[0, 0, 0], [1, 0, 0.2], [0, 1, 0.1], [1, 1, 0.4]], [[1, 2, 3], [4, 3, 2]], 2)


def vertex_pair():
    return _surface([[0, 0, 0], [1, 0, 0.2], [0, 1, 0.1], [-1, 0, 0.3], [0, -1, 0.2]], [[1, 2, 3], [1, 4, 5]], 3)


def two_patches():
    a, ea = edge_pair()
    return _surface(np.concatenate([a[:, :3], a[:, :3] + 5.0]), np.concatenate([ea, ea[::-1] + 4]), 4)


def unused_node():
    return _surface([[0, 0, 0], [9, 9, 9], [1, 0, 0.2], [0, 1, 0.1], [1, 1, 0.4]], [[1, 3, 4], [5, 4, 3]], 5)


def node_twice():
    """element 2 names node 2 twice (a needle of no area); it still sits in that node's list once"""
    return _surface([[0, 0, 0], [1, 0, 0.2], [0, 1, 0.1], [1, 1, 0.4]], [[1, 2, 3], [2, 2, 4], [4, 3, 2]], 6)


def same_triple():
    return _surface([[0, 0, 0], [1, 0, 0.2], [0, 1, 0.1], [1, 1, 0.4]], [[1, 2, 3], [4, 3, 2], [1, 2, 3], [2, 3, 1]], 7)


def tetrahedron():
    return _surface([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 3, 2], [1, 2, 4], [2, 3, 4], [3, 1, 4]], 8)


def octahedron():
    xyz = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    e = [[1, 3, 5], [3, 2, 5], [2, 4, 5], [4, 1, 5], [3, 1, 6], [2, 3, 6], [4, 2, 6], [1, 4, 6]]
    return _surface(xyz, e, 9)


def fan(k):
    """k triangles round one hub: every element neighbours the k - 1 others"""
    ang = 2.0 * math.pi * np.arange(k) / k
    xyz = np.concatenate([[[0.0, 0.0, 0.5]], np.stack([np.cos(ang), np.sin(ang), 0.1 * np.cos(3 * ang)], axis=1)])
    e = [[1, 2 + i, 2 + (i + 1) % k] for i in range(k)]
    return _surface(xyz, e, 100 + k)


def strip(k):
    """k triangles in a row: element i = (i, i + 1, i + 2)"""
    i = np.arange(k + 2)
    xyz = np.stack([0.5 * i, (i % 2) * 1.0, 0.05 * np.sin(0.3 * i)], axis=1)
    e = [[j + 1, j + 2, j + 3] if j % 2 == 0 else [j + 2, j + 1, j + 3] for j in range(k)]
    return _surface(xyz, e, 200 + k)


def grid(nx, ny, seed, permute=True, scale=1.0, shift=0.0):
    """nx x ny cells of two triangles each on a gently curved sheet; the elements in a seeded random order"""
    ii, jj = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1), indexing="ij")
    x, y = ii.ravel() / nx, jj.ravel() / ny
    xyz = np.stack([x, y, 0.1 * np.sin(3.0 * x) * np.cos(2.0 * y)], axis=1) * scale + shift
    nid = lambda i, j: i * (ny + 1) + j + 1
    e = []
    for i in range(nx):
        for j in range(ny):
            e.append([nid(i, j), nid(i + 1, j), nid(i + 1, j + 1)])
            e.append([nid(i, j), nid(i + 1, j + 1), nid(i, j + 1)])
    e = np.array(e, dtype=np.int32)
    if permute:
        e = e[np.random.default_rng(seed).permutation(len(e))]
    return _surface(xyz, e, seed)


STRUCTURES = {
    "one_triangle": one_triangle, "edge_pair": edge_pair, "vertex_pair": vertex_pair, "two_patches": two_patches, "unused_node": unused_node,
    "node_twice": node_twice, "same_triple": same_triple, "tetrahedron": tetrahedron, "octahedron": octahedron,
    "fan63": lambda: fan(63), "fan64": lambda: fan(64), "fan65": lambda: fan(65), "fan300": lambda: fan(300),
    "strip255": lambda: strip(255), "strip256": lambda: strip(256), "strip257": lambda: strip(257),
    "grid12_permuted": lambda: grid(12, 12, 12),
}


@functools.lru_cache(maxsize=None)
def structure(name):
    nodes, e = STRUCTURES[name]()
    nodes.setflags(write=False)
    e.setflags(write=False)
    return nodes, e


# ------------------------------------------------------------------------------------------------ value cases
def zero_area():
    """every node on one line: all triangles have area 0, so W_e and Wn are 0 and every guard keeps the value"""
    nodes, e = grid(4, 4, 31)
    nodes[:, 1] = 2.0 * nodes[:, 0]
    nodes[:, 2] = -nodes[:, 0]
    return nodes, e


def signed_weights():
    """zeros and negative values in the area column: some W_e and Wn are zero, some negative"""
    nodes, e = grid(6, 6, 32)
    rng = np.random.default_rng(33)
    nodes[:, 4] = rng.integers(-2, 3, len(nodes)).astype(np.float64)
    return nodes, e


def neg_zero_and_inf():
    """patch 1: the field is -0.0 everywhere and must stay -0.0 (the sums begin with their first term); patch 2: one node is +inf"""
    a, ea = grid(3, 3, 34)
    b, eb = grid(5, 5, 35)
    a[:, 3] = -0.0
    b[17, 3] = np.inf
    b[:, :3] += 4.0
    return np.concatenate([a, b]), np.concatenate([ea, eb + len(a)])


NAN_NODE = 6 * 13 + 6  # the middle of the 12 x 12 grid


def one_nan():
    nodes, e = grid(12, 12, 36)
    nodes[NAN_NODE, 3] = np.nan
    return nodes, e


def node_rings(e1, nnodes, start):
    """the graph distance of every node from `start` along triangle edges (-1: not connected)"""
    adj = [set() for _ in range(nnodes)]
    for a, b, c in (np.asarray(e1) - 1).tolist():
        adj[a] |= {b, c}
        adj[b] |= {a, c}
        adj[c] |= {a, b}
    dist = [-1] * nnodes
    dist[start] = 0
    front = [start]
    while front:
        nxt = []
        for n in front:
            for m in adj[n]:
                if dist[m] < 0:
                    dist[m] = dist[n] + 1
                    nxt.append(m)
        front = nxt
    return dist


VALUES = {
    "zero_area_n0": (zero_area, 3, -1, 0), "zero_area_n2": (zero_area, 3, -1, 2),
    "signed_weights_n0": (signed_weights, 3, 4, 0), "signed_weights_n1": (signed_weights, 3, 4, 1), "signed_weights_n2": (signed_weights, 3, 4, 2),
    "comp0_n1": (lambda: grid(6, 6, 37), 0, -1, 1), "comp0_n2_area": (lambda: grid(6, 6, 37), 0, 4, 2), "comp2_n5": (lambda: grid(6, 6, 37), 2, -1, 5),
    "comp_is_area_comp": (lambda: grid(6, 6, 38), 4, 4, 2),
    "neg_zero_inf_n0": (neg_zero_and_inf, 3, -1, 0), "neg_zero_inf_n1": (neg_zero_and_inf, 3, -1, 1), "neg_zero_inf_n2_area": (neg_zero_and_inf, 3, 4, 2),
    "nan_n0": (one_nan, 3, -1, 0), "nan_n1": (one_nan, 3, -1, 1), "nan_n2": (one_nan, 3, 4, 2), "nan_n4": (one_nan, 3, -1, 4),
    "coords_1e6_n2": (lambda: grid(8, 8, 39, shift=1.0e6), 3, -1, 2), "coords_1e-6_n2": (lambda: grid(8, 8, 40, scale=1.0e-6), 3, -1, 2),
    "coords_1e-6_n1_comp1": (lambda: grid(8, 8, 40, scale=1.0e-6), 1, -1, 1),
}


@functools.lru_cache(maxsize=None)
def value_case(name):
    build, comp, area_comp, nsmooth = VALUES[name]
    nodes, e = build()
    nodes.setflags(write=False)
    e.setflags(write=False)
    return nodes, e, comp, area_comp, nsmooth


# ------------------------------------------------------------------------------------------------ answers by hand
# Right triangles of legs 1 and 2: every area is 1.  Patch A is a fan of four round node 0, so every element has the three others as
# neighbours (W = 4); patch B is two triangles on one edge (W = 2).  The node values are integers whose triple sums are multiples of 3.
#   A: q = 3, 5, 7, 5 -> one iteration gives (3 + 5 + 7 + 5) / 4 = 5 everywhere.  B: q = 3, 7 -> 5, 5.
# With the area column in place of the areas, B has w = 1, 3 (W = 4): one iteration gives (1*3 + 3*7) / 4 = 6; A has w = 2 throughout.
HAND_XYZ = [[0, 0, 0], [2, 0, 0], [0, 1, 0], [-2, 0, 0], [0, -1, 0], [10, 0, 0], [12, 0, 0], [10, 1, 0], [12, 1, 0]]
HAND_ELTS = [[1, 2, 3], [1, 3, 4], [1, 4, 5], [1, 5, 2], [6, 7, 8], [9, 8, 7]]
HAND_F = [0, 3, 6, 9, 12, 3, 0, 6, 15]
HAND_A = [2, 2, 2, 2, 2, 1, 1, 1, 7]
HAND = {  # (area_comp, nsmooth) -> the field afterwards
    (-1, 0): [5, 4, 4, 6, 6, 3, 5, 5, 7],
    (-1, 1): [5, 5, 5, 5, 5, 5, 5, 5, 5],
    (-1, 2): [5, 5, 5, 5, 5, 5, 5, 5, 5],
    (4, 0): [5, 4, 4, 6, 6, 3, 6, 6, 7],
    (4, 1): [5, 5, 5, 5, 5, 6, 6, 6, 6],
}


def hand_surface():
    nodes = np.concatenate([np.array(HAND_XYZ, dtype=np.float64), np.array(HAND_F, dtype=np.float64)[:, None], np.array(HAND_A, dtype=np.float64)[:, None]], axis=1)
    return np.ascontiguousarray(nodes), np.array(HAND_ELTS, dtype=np.int32)


def _exact(x):
    """x (a Fraction) as it is, after checking that a double holds it"""
    assert Fraction(float(x)) == x, "not exact in a double: %s" % x
    return x


def _third(s):
    """s * (1./3) as the code forms it; the rounded product must be s / 3 exactly"""
    got = float(s) * (1. / 3)
    assert Fraction(got) * 3 == s, "%s * (1./3) does not round to the third" % s
    return Fraction(got)


def verify_hand():
    """the definition in exact rational arithmetic, every intermediate checked to be a double: -> the same table as HAND"""
    X = [[Fraction(v) for v in p] for p in HAND_XYZ]
    E = [[a - 1 for a in tri] for tri in HAND_ELTS]
    out = {}
    for (area_comp, nsmooth) in HAND:
        w, q = [], []
        for n0, n1, n2 in E:
            if area_comp == 4:
                w.append(_third(_exact(_exact(Fraction(HAND_A[n0]) + HAND_A[n1]) + HAND_A[n2])))
            else:
                r1 = [_exact(X[n1][j] - X[n0][j]) for j in range(3)]
                r2 = [_exact(X[n2][j] - X[n0][j]) for j in range(3)]
                r3 = [_exact(_exact(r1[1] * r2[2]) - _exact(r2[1] * r1[2])), _exact(_exact(r1[2] * r2[0]) - _exact(r2[2] * r1[0])),
                      _exact(_exact(r1[0] * r2[1]) - _exact(r2[0] * r1[1]))]
                res = Fraction(0)
                for j in range(3):
                    res = _exact(res + _exact(r3[j] * r3[j]))
                root = Fraction(math.isqrt(int(res)))
                assert res.denominator == 1 and root * root == res, "the area is not a rational number"
                w.append(_exact(Fraction(1, 2) * root))
            q.append(_third(_exact(_exact(Fraction(HAND_F[n0]) + HAND_F[n1]) + HAND_F[n2])))
        nbrs = [sorted({o for o, t in enumerate(E) if o != e and set(t) & set(E[e])}) for e in range(len(E))]
        W = []
        for e in range(len(E)):
            s = w[e]
            for nb in nbrs[e]:
                s = _exact(s + w[nb])
            W.append(s)
        for _ in range(nsmooth):
            new = []
            for e in range(len(E)):
                s = _exact(w[e] * q[e])
                for nb in nbrs[e]:
                    s = _exact(s + _exact(w[nb] * q[nb]))
                new.append(_exact(s / W[e]))
            q = new
        d = []
        for n in range(len(HAND_F)):
            at = [e for e, t in enumerate(E) if n in t]
            wn, sn = w[at[0]], _exact(w[at[0]] * q[at[0]])
            for e in at[1:]:
                wn, sn = _exact(wn + w[e]), _exact(sn + _exact(w[e] * q[e]))
            d.append(_exact(sn / wn))
        out[(area_comp, nsmooth)] = d
    return out


# the size case: about 20 000 elements
SIZE = dict(nx=100, ny=100, seed=77, comp=3, area_comp=-1, nsmooth=3)


@functools.lru_cache(maxsize=None)
def size_surface():
    nodes, e = grid(SIZE["nx"], SIZE["ny"], SIZE["seed"])
    nodes.setflags(write=False)
    e.setflags(write=False)
    return nodes, e
