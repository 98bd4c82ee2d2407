"""The case matrix of the alternate-surface kernel (pa_streamalt.hip), used by the CPU tier (test_streamalt_ref.py) and the GPU tier
(test_gpu_streamalt.py): hand-built line buffers in the layout the trace writes.

Line components: 0..2 X Y Z, 3 the progress variable, 4..6 the velocities, 7 the thickness component, 8 the T component, 9 the
strain.  The queries: progress = ALT_VAL, thickness component = THICK_LO and THICK_HI, T = T_VAL (0.0, so that -0.0 in the data
meets the >= / < tests).  Every case holds two levels with boxes of 1, 63, 64, 65 and 257 lines and empty boxes between them
(one block, a block boundary inside a box, lines of one block in several boxes), node ids permuted.

Each line takes one value pattern per query component and one coordinate pattern; the cycles (12 and 5 long, the components 0, 5
and 7 patterns apart) meet every combination within a box of 64:
  inc         strictly increasing, the crossing anywhere
  cross_m1    the crossing in segment [-1, 0]            cross_0    in segment [0, 1]
  at_point    val equal to a point value (the >= edge: that point is lIdx)
  at_hi       val == v(hi): no segment has val < rVal, the scan is exhausted (rVal == lVal, frac 0, the last segment weighs 0)
  above       val above all values                       at_lo / below_lo   val at / below v(lo): nothing changes
  plateau     pairs of equal values, one pair at val (the < edge skips the first of them)
  two_up      non-monotone, two up-crossings: the first wins
  nan_mid     a NaN at lo + 1 under an increasing line crossing later (every comparison with it is false: the scan walks on)
  neg_zero    -0.0 at a point of an increasing line (equal to T_VAL = 0.0 in every comparison)
Coordinates: straight (power-of-two spacing), curved (random steps), coincident (some segments of length 0: dd = 0), negzero
(z = -0.0 all along), vertical (rising in z).

Kept out on purpose, because the bits of a NaN RESULT are not the serial code's to define (IEEE 754 leaves payload and sign of a
propagated or generated NaN open: x86 gives 0 / 0 the sign bit, the GPU does not): a NaN at v(lo), v(hi) or in a located
segment's carried values, and a line whose points j = -1 and j = 1 coincide (the angle's 0 / 0).  The NaN that is in the matrix
exercises what the reference's comparisons do with one; no output is a NaN, so every output is compared bit for bit."""
from __future__ import annotations

import functools

import numpy as np

import streamalt_ref as A

NCS = 10
ISO, VEL, THICK, TCOMP, STRAIN = 3, 4, 7, 8, 9
ALT_VAL, THICK_LO, THICK_HI, T_VAL = 1.0, 0.5, 2.0, 0.0
NRK = (3, 4, 5, 51)
BOXES = ((1, 0, 63, 0, 64), (0, 65, 0, 257))  # lines per box, per level
KINDS = ("inc", "cross_m1", "cross_0", "at_point", "at_hi", "above", "at_lo", "below_lo", "plateau", "two_up", "nan_mid", "neg_zero")
COORDS = ("straight", "curved", "coincident", "negzero", "vertical")

# the option sets of the kernel: name -> keyword arguments of streamalt_ref.alt_surface / capi.streamalt_run
SUBSETS = {
    "alt": dict(carry=(ISO,)),
    "thick": dict(carry=(ISO,), thickComp=THICK, thickLo=THICK_LO, thickHi=THICK_HI),
    "strain": dict(carry=(VEL, VEL + 1, VEL + 2, ISO), TComp=TCOMP, TVal=T_VAL, strainComp=STRAIN),
    "angle": dict(carry=(ISO,), addAngle=True),
    "all": dict(carry=(VEL, VEL + 1, VEL + 2, ISO), thickComp=THICK, thickLo=THICK_LO, thickHi=THICK_HI, TComp=TCOMP, TVal=T_VAL, strainComp=STRAIN,
                addAngle=True),
    # every query on the progress variable: one distinct query component, read once
    "same_comp": dict(carry=(ISO,), thickComp=ISO, thickLo=THICK_LO, thickHi=THICK_HI, TComp=ISO, TVal=T_VAL, strainComp=STRAIN, addAngle=True),
}


def values(kind: str, val: float, lo: int, hi: int, rng) -> np.ndarray:
    """one component along a line, j = lo .. hi, built around the query value val"""
    j = np.arange(lo, hi + 1, dtype=np.float64)
    nj = len(j)
    s = float(rng.uniform(0.05, 0.4))
    if kind == "inc":
        return val + s * (j - float(rng.uniform(lo + 0.05, hi - 0.05)))
    if kind == "cross_m1":
        return val + s * (j + 0.5)
    if kind == "cross_0":
        return val + s * (j - 0.25)
    if kind == "at_point":
        return val + 0.25 * (j - int(rng.integers(lo + 1, hi)))
    if kind == "at_hi":
        return val + 0.25 * (j - hi)
    if kind == "above":
        return val - 1.0 - 0.125 * (hi - j)
    if kind == "at_lo":
        return val + 0.25 * (j - lo)
    if kind == "below_lo":
        return val + 0.5 + s * (j - lo)
    if kind == "plateau":
        j0 = int(rng.integers(lo, hi))
        return val + 0.25 * np.floor((j - j0) / 2.0)
    if kind == "two_up":
        return val + 0.3 * (((j - lo) % 4.0) - 1.5)
    if kind == "nan_mid":
        if nj < 5:  # no room for a NaN away from v(lo), v(hi) and the located segment
            return val + s * (j - (hi - 0.5))
        v = val + s * (j - float(rng.uniform(lo + 3.05, hi - 0.05)))
        v[1] = np.nan
        return v
    if kind == "neg_zero":
        v = 0.25 * (j - int(rng.integers(lo + 1, hi)))
        v[v == 0.0] = -0.0
        return v
    raise KeyError(kind)


def coords(kind: str, lo: int, hi: int, rng) -> np.ndarray:
    """X Y Z along a line -> [3][nj]; the points j = -1 and j = 1 never coincide"""
    nj = hi - lo + 1
    x0 = rng.uniform(0.1, 0.9, 3)
    if kind == "straight":
        step = np.array([0.0625, -0.03125, 0.015625]) * (1 if rng.random() < 0.5 else -1)
        x0 = np.round(x0 * 64) / 64
        return x0[:, None] + step[:, None] * np.arange(lo, hi + 1)[None, :]
    inc = rng.normal(0.0, 0.02, (3, nj - 1))
    if kind == "coincident":
        dead = rng.random(nj - 1) < 0.4
        dead[-lo - 1] = False  # segment [-1, 0] stays, so x(-1) != x(1) whatever happens to [0, 1]
        dead[-lo] = True       # segment [0, 1] has length 0
        inc[:, dead] = 0.0
    if kind == "vertical":
        inc[0:2] = 0.0
        inc[2] = np.abs(inc[2]) + 0.001
    x = np.concatenate([x0[:, None], x0[:, None] + np.cumsum(inc, axis=1)], axis=1)
    if kind == "negzero":
        x[2] = -0.0
    return x


@functools.lru_cache(maxsize=None)
def build(nRKsteps: int):
    """-> (lines[l][b] = [NCS][nRKsteps][n] or None, ins[l][b] = 1-based node ids, nNodes)"""
    lo, hi = A.jrange(nRKsteps)
    rng = np.random.default_rng(1000 + nRKsteps)
    nNodes = sum(sum(b) for b in BOXES)
    perm = rng.permutation(nNodes).astype(np.int32) + 1
    lines, ins, k = [], [], 0
    for per in BOXES:
        L, I = [], []
        for n in per:
            if n == 0:
                L.append(None)
                I.append(np.zeros(0, np.int32))
                continue
            st = np.empty((NCS, nRKsteps, n))
            for i in range(n):
                st[0:3, :, i] = coords(COORDS[k % len(COORDS)], lo, hi, rng)
                st[ISO, :, i] = values(KINDS[k % len(KINDS)], ALT_VAL, lo, hi, rng)
                st[THICK, :, i] = values(KINDS[(k + 5) % len(KINDS)], THICK_LO if (k // len(KINDS)) % 2 == 0 else THICK_HI, lo, hi, rng)
                st[TCOMP, :, i] = values(KINDS[(k + 7) % len(KINDS)], T_VAL, lo, hi, rng)
                st[VEL:VEL + 3, :, i] = rng.normal(0.0, 1.0, (3, nRKsteps))
                st[STRAIN, :, i] = rng.normal(0.0, 100.0, nRKsteps)
                k += 1
            L.append(st)
            I.append(perm[k - n:k].copy())
        lines.append(L)
        ins.append(I)
    return lines, ins, nNodes


@functools.lru_cache(maxsize=None)
def reference(nRKsteps: int, subset: str, mistake=None):
    """the restatement on the case (computed once per process; callers must not write into it)"""
    lines, ins, nNodes = build(nRKsteps)
    out, branch, lidx = A.alt_surface(lines, ins, nRKsteps, nNodes, ISO, ALT_VAL, mistake=mistake, **SUBSETS[subset])
    for a in (out, branch, lidx):
        a.setflags(write=False)
    return out, branch, lidx
