"""The case matrix of the stream subsetting (streamSub.cpp; pa_streamsub.hip, streamSub3d), shared by test_streamsub_ref.py (CPU: the
restatement against hand-written answers) and test_gpu_streamsub.py (GPU: kernels and the executable against the restatement).  The
smallest shapes at which each piece can go wrong.  Not a test module."""
import functools
import math

import numpy as np

import streamsample_ref as S
import streamsel_cases as SK
import streamsub_ref as R

NAN_PAYLOAD = 0x7FF8000012345678   # a quiet NaN with a payload
NAN_SIGNAL = 0x7FF0000000000001    # a signalling NaN: a copy through a floating-point register could quiet it
PLUS_INF, MINUS_INF, MINUS_ZERO = 0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000


# ------------------------------------------------------------------------------------------------ the hand-worked directory
def hand_dir():
    """Two levels, three boxes, six lines with permuted ids, three elements; components X Y Z T with value 1000 c + 100 g + 10 line + (j - jlo),
    g the flat box index, so a value names where it came from.
      level 0: box 0 (g 0): 2 lines, j = -1 .. 1, ids 5 2        box 1 (g 1): 1 line, j = 0 .. 1, id 6
      level 1: box 0 (g 2): 3 lines, j = -1 .. 0, ids 1 4 3
      elements (file ids): e0 = 5 2 5 (box g0 alone)   e1 = 6 1 3 (g1 and g2)   e2 = 4 4 4 (g2 alone)"""
    names = ["X", "Y", "Z", "T"]
    shapes = [[(2, -1, 1), (1, 0, 1)], [(3, -1, 0)]]
    ins = [[[5, 2], [6]], [[1, 4, 3]]]
    levels, g = [], 0
    for lev in shapes:
        fabs = []
        for n, jl, jh in lev:
            a = np.zeros((4, jh - jl + 1, n))
            for c in range(4):
                for j in range(jh - jl + 1):
                    for i in range(n):
                        a[c, j, i] = 1000 * c + 100 * g + 10 * i + j
            fabs.append(((0, jl, 0), (n - 1, jh, 0), a))
            g += 1
        levels.append(fabs)
    face = [5, 2, 5, 6, 1, 3, 4, 4, 4]
    return names, R.dir_files(names, levels, ins, face, 3)


# ------------------------------------------------------------------------------------------------ the edge directory
def node_at(ins, lev, box, k):
    return int(ins[lev][box][k])


@functools.lru_cache(maxsize=None)
def edge_dir(npe=3, nrandom=40, seed=5):
    """streamsel_cases.scatter_dir (two levels; boxes of 65 lines, none, 1, 63, 64; four j ranges; ids permuted over everything; the name T
    twice; NaN, +inf and -0.0 in components 4 and 5) with an element table of `npe` nodes over it:
      e0: all nodes in level 0 box 0         e1: nodes in level 0 boxes 0 and 2 and level 1 box 0 (npe = 1: level 0 box 2)
      e2 .. e5: all nodes in level 1 box 1   the rest: random nodes
    Two values of component 3 carry NaN payloads (level 1 box 0) and one is -inf (level 1 box 1, which the all-elements run and the one-box
    run both keep), so the matrix carries NaN with payload, +inf, -inf and -0.0 through the copy.  -> (files, path)"""
    names, files, levels, ins = SK.scatter_dir()
    rng = np.random.default_rng(seed)
    a = levels[1][0][2]
    a[3, 1, 2] = np.array([NAN_PAYLOAD], np.uint64).view(np.float64)[0]
    a[3, 2, 5] = np.array([NAN_SIGNAL], np.uint64).view(np.float64)[0]
    levels[1][1][2][3, 4, 17] = -np.inf
    N = sum(len(i) for per in ins for i in per)
    face = [node_at(ins, 0, 0, (7 * i) % 65) for i in range(npe)]
    spread = [(0, 2, 0), (0, 0, 11), (1, 0, 62), (0, 0, 64)]
    face += [node_at(ins, *spread[i % 4]) for i in range(npe)]
    for e in range(4):
        face += [node_at(ins, 1, 1, (13 * e + 29 * i) % 64) for i in range(npe)]
    face += [int(v) for v in rng.integers(1, N + 1, size=nrandom * npe)]
    files = R.dir_files(names, levels, ins, face, len(face) // npe)
    return files, S.read_stream_dir(files)


EDGE_RUNS = [dict(),                                     # the reference's defined case: element 0 alone
             dict(eltIDs=[1]),                           # three boxes on two levels
             dict(eltIDs=[2, 3, 4, 5]),                  # one box of level 1: level 0 becomes empty
             dict(sElt=0, nElt=46),                      # all elements
             dict(eltIDs=[7, 5, 5, 2]),                  # descending, with a duplicate
             dict(sElt=3, nElt=4),
             dict(eltIDs=[1], comps=["H2"]),             # one component
             dict(eltIDs=[1, 0], comps=["cond", "X"]),   # a subset, given out of the file's order
             dict(eltIDs=[9], comps=["T"], verbose=1),   # the name the file holds twice: both
             dict(sElt=0, nElt=46, comps=["X", "Y", "T", "H2", "cond"], verbose=1)]
EDGE_ONE_BOX = 2
EDGE_ALL = 3


# ------------------------------------------------------------------------------------------------ seed boxes
SEED_LO, SEED_HI = (0.25, 0.25, 0.25), (0.75, 0.75, 0.75)


@functools.lru_cache(maxsize=None)
def seed_dir():
    """the edge directory with hand-set seed points (components 0, 1, 2 at j = 0): every node strictly inside SEED_LO .. SEED_HI or strictly
    outside by chance (uniform in 0 .. 1), then the first elements' nodes by hand:
      e0: seeds exactly on lo, exactly on hi, inside: kept        e1: one coordinate one ulp above hi: dropped
      e2: one coordinate one ulp below lo: dropped                e3: a NaN coordinate: dropped
      e4: all inside: kept      e5: one node outside: dropped     e6: x = +0.0, -0.0, +0.0 (kept only by a box with a zero bound)
    -> (files, path)"""
    names, files, levels, ins = SK.scatter_dir()
    rng = np.random.default_rng(23)
    for l, lev in enumerate(levels):
        for b, (lo, hi, a) in enumerate(lev):
            if len(ins[l][b]):
                a[0:3, 0 - lo[1], :] = rng.uniform(0.0, 1.0, size=(3, a.shape[2]))

    def put(l, b, k, xyz):
        lo, hi, a = levels[l][b]
        a[0:3, 0 - lo[1], k] = xyz
        return node_at(ins, l, b, k)
    mid = (0.5, 0.5, 0.5)
    up, down = math.nextafter(0.75, math.inf), math.nextafter(0.25, -math.inf)
    face = [put(0, 0, 0, SEED_LO), put(1, 0, 0, SEED_HI), put(1, 1, 0, (0.25, 0.75, 0.5))]
    face += [put(0, 0, 1, mid), put(1, 0, 1, (0.5, up, 0.5)), put(1, 1, 1, mid)]
    face += [put(0, 0, 2, mid), put(1, 0, 2, (0.5, 0.5, down)), put(1, 1, 2, mid)]
    face += [put(0, 0, 3, (float("nan"), 0.5, 0.5)), put(1, 0, 3, mid), put(1, 1, 3, mid)]
    face += [put(0, 0, 4, mid), put(0, 2, 0, (0.3, 0.7, 0.26)), put(1, 1, 4, mid)]
    face += [put(0, 0, 5, mid), put(1, 0, 5, (0.9, 0.5, 0.5)), put(1, 1, 5, mid)]
    face += [put(0, 0, 6, (0.0, 0.5, 0.5)), put(1, 0, 6, (-0.0, 0.5, 0.5)), put(1, 1, 6, (0.0, 0.5, 0.5))]
    N = sum(len(i) for per in ins for i in per)
    face += [int(v) for v in rng.integers(1, N + 1, size=60 * 3)]
    files = R.dir_files(names, levels, ins, face, len(face) // 3)
    return files, S.read_stream_dir(files)


INF = float("inf")
SEED_RUNS = [dict(seedLo=SEED_LO, seedHi=SEED_HI),                               # e0 and e4 among the kept, e1 e2 e3 e5 e6 not
             dict(seedLo=(-0.0, 0.0, 0.0), seedHi=(0.0, 1.0, 1.0)),              # bound -0.0 against seed +0.0: e6 alone
             dict(seedLo=(-INF, -INF, -INF), seedHi=(INF, INF, INF), comps=["X", "Y", "T"])]  # everything but the NaN seed
SEED_ALL = dict(seedLo=(-INF, -INF, -INF), seedHi=(INF, INF, INF))               # over edge_dir, which holds no NaN seed: every element, in order
SEED_NONE = dict(seedLo=(2.0, 2.0, 2.0), seedHi=(3.0, 3.0, 3.0))                 # keeps nothing: abort


def no_seed_dir():
    """a box with lines whose j range lacks the seed point"""
    names, files, levels, ins = SK.scatter_dir()
    lo, hi, a = levels[0][2]
    levels[0][2] = ((0, 1, 0), (0, 1 + a.shape[1] - 1, 0), a)
    return R.dir_files(names, levels, ins, [1, 2, 3], 3)  # three elements of one node


# ------------------------------------------------------------------------------------------------ more than one workgroup
@functools.lru_cache(maxsize=None)
def big_dir(nelts, npe=3, seed=3):
    """1030 lines in boxes of 701 and 329 lines of 3 points: runs of 2103 doubles (two copy chunks, odd) and 987 (odd), so consecutive runs
    start 8-byte- but not 16-byte-aligned; `nelts` random elements; seeds uniform in 0 .. 1 -> (files, path)"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(1030) + 1
    fabs, per, at = [], [], 0
    for n in (701, 329):
        a = rng.normal(size=(5, 3, n))
        a[0:3, 1, :] = rng.uniform(0.0, 1.0, size=(3, n))
        fabs.append(((0, -1, 0), (n - 1, 1, 0), a))
        per.append(perm[at:at + n])
        at += n
    face = [int(v) for v in rng.integers(1, 1031, size=nelts * npe)]
    files = R.dir_files(SK.PLT_NAMES, [fabs], [per], face, nelts)
    return files, S.read_stream_dir(files)


BIG_ELTS = [255, 256, 257, 2100]   # the compaction's count blocks: 1, 1, 2, 9
BIG_SEED = dict(seedLo=(0.0, 0.0, 0.0), seedHi=(0.8, 0.8, 1.0))  # about 0.64 ^ 3 of the elements


@functools.lru_cache(maxsize=None)
def many_boxes_dir(nboxes, seed=9):
    """`nboxes` boxes of one line and three points on two levels (runs of 3 doubles: every run shifts the alignment of the next), ids permuted,
    40 random triangles -> (files, path)"""
    rng = np.random.default_rng(seed + nboxes)
    perm = rng.permutation(nboxes) + 1
    n0 = nboxes // 3
    levels, ins = [], []
    for lo_b, hi_b in ((0, n0), (n0, nboxes)):
        levels.append([((0, -1, 0), (0, 1, 0), rng.normal(size=(4, 3, 1))) for _ in range(lo_b, hi_b)])
        ins.append([[int(perm[b])] for b in range(lo_b, hi_b)])
    face = [int(v) for v in rng.integers(1, nboxes + 1, size=40 * 3)]
    files = R.dir_files(["X", "Y", "Z", "T"], levels, ins, face, 40)
    return files, S.read_stream_dir(files)


MANY_BOXES = [255, 256, 257, 1100]   # the box scan: one workgroup, one, block sums of 2, of 5
