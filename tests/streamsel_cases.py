"""The case matrix of the stream selection tools, shared by test_streamsel_ref.py (CPU: the restatement against hand-written answers)
and test_gpu_streamsel.py (GPU: kernels and executables against the restatement).  Not a test module."""
import numpy as np

import streamsel_ref as R

NULL_BOX = ((0, 0, 0), (0, 0, 0))


# ------------------------------------------------------------------------------------------------ the hand-worked directory
def small_dir(ids=(3, 1, 2)):
    """3 lines of 5 points (j = -2 .. 2) in one box, node ids 3, 1, 2 (or `ids`); components X Y Z T c.  Worked out by hand in test_streamsel_ref.py:
      segment lengths   line 0: 1 1 1 1    line 1: 5 0 0 4    line 2: 2 2 2 2
      T                 line 0: ascending  line 1: descending line 2: constant
      c                 line 0: 0 10 20 30 40   line 1: 7 7 9 7 7   line 2: 9 1 1 1 9"""
    X = [[0, 1, 2, 3, 4], [0, 3, 3, 3, 3], [0, 0, 0, 0, 0]]
    Y = [[0, 0, 0, 0, 0], [0, 4, 4, 4, 8], [0, 0, 0, 0, 0]]
    Z = [[0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 2, 4, 6, 8]]
    T = [[1, 2, 3, 4, 5], [5, 4, 3, 2, 1], [1, 1, 1, 1, 1]]
    c = [[0, 10, 20, 30, 40], [7, 7, 9, 7, 7], [9, 1, 1, 1, 9]]
    a = np.array([X, Y, Z, T, c], float).transpose(0, 2, 1)  # [comp][j][line]
    names = ["X", "Y", "Z", "T", "c"]
    return names, R.write_files(names, [[((0, -2, 0), (2, 2, 0), a)]], [[list(ids)]])


# ------------------------------------------------------------------------------------------------ streamScatter
SCATTER_NAMES = ["X", "Y", "T", "H2", "cond", "T"]  # vars=T is the first T (:90-94), condVar=T the last (:106-110)
SCATTER_BOXES = [[(65, -3, 3), None, (1, -4, 3)], [(63, -5, 2), (64, 0, 5)]]  # (lines, jlo, jhi); mid points 0, 0 (from -0.5), -1 (from -1.5), 2 (from 2.5)
MORE, LESS = 3.0, 8.0


def scatter_dir(seed=7):
    """Two levels; a zero box; boxes of 65, 1, 63 and 64 lines with four j ranges; node ids permuted over all boxes and levels.  The
    conditioning values (components 4 and 5) are small integers, so ties abound; the first lines of every box are set by hand:
      0 constant (the mid point stays: truncation against floor)   1 the mid value again at an earlier point (the mid stays)
      2 two equal maxima above the mid value (the first wins)      3 peak at the first point       4 peak at the last point
      5 +inf in mid-line    6 all -0.0 but one +0.0 (no strict >: hiVal = -0.0)    7 NaN at the mid point (hiVal = NaN, dropped)
      8 NaN elsewhere (skipped)    9 hiVal == MORE exactly (kept)    10 hiVal == LESS exactly (dropped)
    The other components are distinct doubles, so a row identifies the (line, j) it was read at."""
    rng = np.random.default_rng(seed)
    N = sum(b[0] for lev in SCATTER_BOXES for b in lev if b)
    perm = rng.permutation(N) + 1
    levels, ins, at = [], [], 0
    for lev in SCATTER_BOXES:
        fabs, per = [], []
        for b in lev:
            if b is None:
                fabs.append(NULL_BOX + (np.zeros((len(SCATTER_NAMES), 1, 1)),))
                per.append([])
                continue
            n, jl, jh = b
            nj, mid = jh - jl + 1, R.trunc_mid(jl, jh) - jl
            a = rng.normal(size=(len(SCATTER_NAMES), nj, n))
            cond = rng.integers(0, 10, size=(nj, n)).astype(float)
            special = [np.full(nj, 5.0)]
            v = np.ones(nj); v[mid] = 5.0; v[0] = 5.0; special.append(v)
            v = np.ones(nj); v[mid] = 2.0; v[1] = 7.0; v[nj - 2] = 7.0; special.append(v)
            v = np.arange(nj, 0, -1.0); special.append(v)
            v = np.arange(nj) * 1.0; special.append(v)
            v = np.ones(nj); v[mid + 1] = np.inf; special.append(v)
            v = np.full(nj, -0.0); v[1] = 0.0; special.append(v)
            v = np.arange(nj) * 1.0; v[mid] = np.nan; special.append(v)
            v = np.full(nj, 4.0); v[0] = np.nan; v[nj - 1] = np.nan; v[mid + 1] = 6.0; special.append(v)
            v = np.full(nj, 1.0); v[nj - 1] = MORE; special.append(v)
            v = np.full(nj, 1.0); v[1] = LESS; special.append(v)
            for k, v in enumerate(special[:n]):
                cond[:, k] = v
            a[4] = cond
            a[5] = cond[::-1] + 0.5  # another conditioning field under the duplicate name
            fabs.append(((0, jl, 0), (n - 1, jh, 0), a))
            per.append(perm[at:at + n])
            at += n
        levels.append(fabs)
        ins.append(per)
    return SCATTER_NAMES, R.write_files(SCATTER_NAMES, levels, ins), levels, ins


SCATTER_RUNS = [dict(vars=["cond", "X", "T", "H2"], condComp=4, condValMoreThan=MORE, condValLessThan=LESS),
                dict(vars=["T", "Y"], condVar="T", condValMoreThan=-1.0, condValLessThan=float("inf")),  # +inf itself is dropped (inf < inf), -0.0 kept
                dict(vars=["cond"], condVar="cond", condValMoreThan=0.0, condValLessThan=0.5),  # -0.0 >= 0: printed as -0
                dict(vars=["X"], condComp=4, condValMoreThan=100.0, condValLessThan=200.0)]  # keeps nothing: empty stdout, exit 0


# ------------------------------------------------------------------------------------------------ stream2plt
PLT_NAMES = ["X", "Y", "Z", "a", "b"]
PLT_BOXES = [[65, None, 1], [63, 64]]
PLT_J = (-4, 3)  # the RXY point: (int)(-0.5) = 0, not floor = -1


def plt_dir(seed=11):
    """Two levels, a zero box, boxes of 65, 1, 63, 64 lines, all j = -4 .. 3.  X Y Z: random walks (the running sqrt sum is inexact).
    a: per line one of  j (on a point at 0: no crossing of 0),  j + 0.5 (ascending crossing),  -(j + 0.5) (descending),  constant 3,
    j with a NaN in mid-line.  b: random, with a large first point on line 0 (the seed of every line's max / min)."""
    rng = np.random.default_rng(seed)
    jl, jh = PLT_J
    nj = jh - jl + 1
    js = np.arange(jl, jh + 1, dtype=float)
    levels, ins, at = [], [], 0
    N = sum(n for lev in PLT_BOXES for n in lev if n)
    perm = rng.permutation(N) + 1
    for l, lev in enumerate(PLT_BOXES):
        fabs, per = [], []
        for n in lev:
            if n is None:
                fabs.append(NULL_BOX + (np.zeros((5, 1, 1)),))
                per.append([])
                continue
            xyz = np.cumsum(rng.normal(size=(3, nj, n)) * 0.37, axis=1) + rng.normal(size=(3, 1, n))
            kind = rng.integers(0, 5, size=n)
            a = np.empty((nj, n))
            for i in range(n):
                a[:, i] = [js, js + 0.5, -(js + 0.5), np.full(nj, 3.0), js][kind[i]]
                if kind[i] == 4:
                    a[2, i] = np.nan
            b = rng.normal(size=(nj, n))
            if l == 0 and at == 0:
                b[0, 0] = 1.25
            fabs.append(((0, jl, 0), (n - 1, jh, 0), np.concatenate([xyz, a[None], b[None]])))
            per.append(perm[at:at + n])
            at += n
        levels.append(fabs)
        ins.append(per)
    return PLT_NAMES, R.write_files(PLT_NAMES, levels, ins), levels, ins


ALL = 1000  # nLines >= NLines: every line is taken whatever the generator
PLT_RUNS = [dict(nLines=ALL),
            dict(nLines=ALL, no_filter=1, comps=[4, 0]),
            dict(nLines=ALL, maxComps=[4], maxVals=[1.5], maxSgns=["lt"]),
            dict(nLines=ALL, maxComps=[4, 3], maxVals=[1.25, 3.0], maxSgns=["gt", "le"]),
            dict(nLines=ALL, minComps=[4, 4], minVals=[-1.0, -2.5], minSgns=["ge", "ne"]),
            dict(nLines=ALL, minComps=[3], minVals=[-4.0], minSgns=["eq"]),
            dict(nLines=ALL, maxComps=[4], maxVals=[0.0], maxSgns=["bigger"]),  # an unknown sign tests false: nothing is written
            dict(nLines=ALL, RXY=1.0, RXYsgn="gt"),
            dict(nLines=ALL, RXY=1.0, RXYsgn="le", comps=[1, 2, 0, 3]),
            dict(nLines=ALL, atComps=[3], compAt=[4.9], valAt=[0.0], atVal=[0.0], atSgns=["gt"]),  # compAt 4.9 -> 4
            dict(nLines=ALL, atComps=[3, 3], compAt=[4, 0], valAt=[0.1, 0.0], atVal=[1.0, -2.0], atSgns=["lt", "ge"]),
            dict(nLines=ALL, maxComps=[4], maxVals=[1.0], maxSgns=["lt"], atComps=[3], compAt=[4], valAt=[0.0], atVal=[0.0], atSgns=["gt"]),  # switched back on
            dict(nLines=ALL, distComp=3, distVal=0.0),
            dict(nLines=ALL, distComp=3, distVal=100.0),  # no crossing anywhere: 2 x length
            dict(nLines=ALL, distComp=4, distVal=0.25, comps=[2, 0, 1, 4, 3], sComp=1, nComp=2),  # comps wins; the coordinates are Z X Y
            dict(nLines=ALL, sComp=1, nComp=3),
            dict(nLines=ALL, maxComps=[4], maxVals=[1.5], maxSgns=["lt"], minComps=[4], minVals=[-2.0], minSgns=["gt"], RXY=0.5, RXYsgn="ge", atComps=[3], compAt=[4],
                 valAt=[-0.5], atVal=[0.0], atSgns=["gt"], distComp=3, distVal=0.0, verbose=1),
            dict(nLines=60, distComp=3, distVal=0.0, verbose=1),  # rval < 1: the recalled draw
            dict(nLines=40000, finestLevel=1),  # capped at 32700
            # the driver's own decoding in one run: reordered comps (3 is b, 4 is a), ne and eq, a fractional compAt (3.9 -> 3), and an
            # unknown sign in an at-test, which ASSIGNS false to the lines that cross and leaves the others as the min-tests left them
            dict(nLines=ALL, comps=[2, 0, 1, 4, 3], minComps=[3, 4], minVals=[-2.5, -4.0], minSgns=["ne", "eq"], atComps=[4], compAt=[3.9], valAt=[0.0],
                 atVal=[0.0], atSgns=["bigger"])]
