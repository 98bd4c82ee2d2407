"""An independent numpy reference of the ghost fills (pa_fill_boundary, pa_fillpatch_two_levels, pa_foextrap, pa_fill_ghosts_hierarchy
and the wall / classification half of pa_apply_bc) on DENSE arrays: no box is ever intersected with another one here.

Per level l and component, two arrays over the level's domain, [nz, ny, nx]:
  D_l  the valid cells of every box painted in, NaN elsewhere;
  I_l  avgplt_ref.interp_dense(D_{l-1}, ratio, is_per, interp_type) for l > 0 (that interpolant is held to the oracle's by
       test_avgplt_ref.py).
A ghost cell q of a box is of class 2 if it lies outside the domain in a non-periodic direction; else it is wrapped by modulo and is
of class 0 where D_l is finite there (FillBoundary's cell) and of class 1 elsewhere (FillPatchTwoLevels').  Its value is D_l / I_l at
the wrapped cell; for class 2 (foextrap) that of q clamped into the domain in the non-periodic directions, itself of class 0 or 1.
A level whose domain is wider than WHOLE_MAX cells is held on a window only (deep levels of a nested hierarchy: 256^3 cells for 8^3
valid ones): the coarse cells under its grown boxes and one more around them, refined.  The window must lie strictly inside the
domain, so that neither the wrap nor the clamp applies to it; that is asserted.

Imports neither the oracle nor the library."""
import dataclasses

import numpy as np

from avgplt_ref import interp_dense

WHOLE_MAX = 48


@dataclasses.dataclass
class LevelRef:
    level: object
    lo: np.ndarray      # (3,) x y z: the cell that index 0 of the dense arrays stands for
    shape: tuple        # (nz, ny, nx)
    whole: bool         # the dense arrays cover the whole domain
    D: dict             # comp -> array
    I: dict             # comp -> array (empty on level 0)
    keep: dict          # comp -> intermediates of interp_dense (interp_type 1)
    clo: np.ndarray = None  # (3,) the coarse cell under index 0 (levels > 0)


@dataclasses.dataclass
class BoxRef:
    G: int              # ghost width of the arrays below (the allocated one)
    cls: np.ndarray     # [nz + 2G, ny + 2G, nx + 2G] int8: -1 valid, 0 / 1 / 2
    layer: np.ndarray   # Chebyshev distance to the valid box (0 = valid cell)
    exp: dict           # comp -> expected value of every ghost cell after FillBoundary, FillPatchTwoLevels and foextrap
    clamp: tuple        # (kz, jy, ix) index vectors: the FAB cell foextrap copies from (the cell itself inside the domain)
    widx: tuple         # (kz, jy, ix) index vectors into the level's dense arrays (wrapped; clipped where outside a wall)
    out: np.ndarray     # bool: outside a wall


def _floor_div(a, r):
    return np.floor_divide(a, r)


def _window(level, G, r, prev):
    """(lo, hi, whole, clo) of the dense arrays of a level"""
    n = level.domhi.astype(np.int64) - level.domlo + 1
    if n.max() <= WHOLE_MAX and (prev is None or prev.whole):
        return level.domlo.astype(np.int64), level.domhi.astype(np.int64), True, (None if prev is None else _floor_div(level.domlo.astype(np.int64), r))
    assert prev is not None, "level 0 is held whole"
    need_lo = level.boxes[:, :3].min(axis=0).astype(np.int64) - G
    need_hi = level.boxes[:, 3:].max(axis=0).astype(np.int64) + G
    clo, chi = _floor_div(need_lo, r) - 1, _floor_div(need_hi, r) + 1
    lo, hi = clo * r, chi * r + r - 1
    assert (lo > level.domlo).all() and (hi < level.domhi).all(), "a windowed level must stay clear of the domain's faces"
    phi = prev.lo + np.array(prev.shape[::-1]) - 1
    assert (clo >= prev.lo).all() and (chi <= phi).all(), "the window's parents must lie in the coarser level's arrays"
    return lo, hi, False, clo


def dense_levels(levels, mfs, comps, ratio, interp_type, alloc):
    """LevelRef per level.  mfs: host multifabs with the valid data (their ghost cells are not read); comps: components to hold;
    alloc[l]: the ghost width of level l's multifab"""
    out = []
    for l, (lv, mf) in enumerate(zip(levels, mfs)):
        prev = out[-1] if l else None
        lo, hi, whole, clo = _window(lv, alloc[l], ratio, prev)
        shape = tuple(int(v) for v in (hi - lo + 1)[::-1])
        R = LevelRef(lv, lo, shape, whole, {}, {}, {}, clo)
        for c in comps:
            a = np.full(shape, np.nan)
            for b in range(lv.nboxes):
                b0 = lv.boxes[b, :3] - lo
                b1 = lv.boxes[b, 3:] - lo + 1
                a[b0[2]:b1[2], b0[1]:b1[1], b0[0]:b1[0]] = mf.valid(b)[c]
            R.D[c] = a
            if l:
                keep = {}
                if whole:
                    R.I[c] = interp_dense(prev.D[c], ratio, lv.is_per, interp_type, keep)
                else:
                    s0 = clo - prev.lo
                    s1 = s0 + np.array(shape[::-1]) // ratio
                    R.I[c] = interp_dense(prev.D[c][s0[2]:s1[2], s0[1]:s1[1], s0[0]:s1[0]], ratio, (0, 0, 0), interp_type, keep)
                assert R.I[c].shape == shape
                R.keep[c] = keep
        out.append(R)
    return out


def box_ref(R: LevelRef, b: int, G: int, comps) -> BoxRef:
    lv = R.level
    blo, bhi = lv.boxes[b, :3].astype(np.int64), lv.boxes[b, 3:].astype(np.int64)
    idx = [np.arange(blo[d] - G, bhi[d] + G + 1) for d in range(3)]
    outs, widx, cidx, clamp, dist = [], [], [], [], []
    for d in range(3):
        i = idx[d]
        lo, hi = int(lv.domlo[d]), int(lv.domhi[d])
        n = hi - lo + 1
        beyond = (i < lo) | (i > hi)
        if not R.whole:
            assert not beyond.any()
            w = c = i - R.lo[d]
            o = np.zeros_like(beyond)
        elif lv.is_per[d]:
            w = c = (i - lo) % n
            o = np.zeros_like(beyond)
        else:
            w = c = np.clip(i, lo, hi) - lo
            o = beyond
        outs.append(o)
        widx.append(w)
        cidx.append(c)
        clamp.append((np.clip(i, lo, hi) if (R.whole and not lv.is_per[d]) else i) - (blo[d] - G))
        dist.append(np.maximum(np.maximum(blo[d] - i, i - bhi[d]), 0))
    out = outs[2][:, None, None] | outs[1][None, :, None] | outs[0][None, None, :]
    layer = np.maximum(np.maximum(dist[2][:, None, None], dist[1][None, :, None]), dist[0][None, None, :])
    ix = np.ix_(widx[2], widx[1], widx[0])
    c0 = comps[0]
    covered = np.isfinite(R.D[c0][ix])
    cls = np.where(out, 2, np.where(covered, 0, 1)).astype(np.int8)
    cls[layer == 0] = -1
    exp = {}
    for c in comps:
        d = R.D[c][ix]
        assert (np.isfinite(d) == covered).all(), "every component is painted on the same cells"
        exp[c] = np.where(covered, d, R.I[c][ix] if R.I else np.nan)  # class 2: widx is the clamped cell already
    return BoxRef(G, cls, layer, exp, (clamp[2], clamp[1], clamp[0]), (widx[2], widx[1], widx[0]), out)


CALL_CLASS = {"fb": 0, "fp": 1, "fo": 2}


def write_mask(B: BoxRef, call: str, ng: int) -> np.ndarray:
    """the cells that call alone may write: ghost cells of its class within ng layers"""
    return (B.cls == CALL_CLASS[call]) & (B.layer <= ng) & (B.layer > 0)


def apply_call(fab: np.ndarray, B: BoxRef, comps, call: str, ng: int) -> int:
    """what the call does to one FAB [ncomp, nz, ny, nx] (in place), given what the FAB holds: FillBoundary and FillPatchTwoLevels
    store the dense value, foextrap copies the FAB's own cell at the clamped index -- after the other two that is the dense value as
    well, alone it is whatever the FAB held there.  Returns the number of doubles stored"""
    m = write_mask(B, call, ng)
    for c in comps:
        if call == "fo":
            src = fab[c][np.ix_(*B.clamp)]
            fab[c][m] = src[m]
        else:
            fab[c][m] = B.exp[c][m]
    return int(m.sum()) * len(comps)


# ----------------------------------------------------------------------------- applyBC
def bc_faces(B: BoxRef, only_dir: int = -1):
    """the first-layer face ghost cells of a box: list of (dir, side, ghost slab index, interior slab index) with slab indices as
    tuples of slices into the grown arrays [z, y, x]"""
    G = B.G
    n = [s - 2 * G for s in B.cls.shape]  # nz, ny, nx
    faces = []
    for d in range(3):
        if only_dir >= 0 and d != only_dir:
            continue
        ax = 2 - d
        for side in (0, 1):
            g = [slice(G, G + n[a]) for a in range(3)]
            i = list(g)
            g[ax] = slice(G - 1, G) if side == 0 else slice(G + n[ax], G + n[ax] + 1)
            i[ax] = slice(G, G + 1) if side == 0 else slice(G + n[ax] - 1, G + n[ax])
            faces.append((d, side, tuple(g), tuple(i)))
    return faces


def apply_bc(fab: np.ndarray, comp: int, B: BoxRef, bc, only_dir: int = -1):
    """applyBC's wall half on one FAB (in place): a face ghost cell beyond a wall takes +interior (Neumann, bc 1) or -interior
    (reflect-odd, bc 2).  Returns (mask of the face ghost cells of class 1 -- the coarse-fine ones, whose value is the oracle's --,
    mask of the wall cells written)"""
    cf = np.zeros(B.cls.shape, dtype=bool)
    wall = np.zeros(B.cls.shape, dtype=bool)
    for d, side, g, i in bc_faces(B, only_dir):
        k = B.cls[g]
        cf[g] = k == 1
        wall[g] = k == 2
        v = fab[comp][i]
        assert bc[d] in (1, 2) or not (k == 2).any(), "a periodic direction has no wall"
        fab[comp][g] = np.where(k == 2, -v if bc[d] == 2 else v, fab[comp][g])
    return cf, wall


# ----------------------------------------------------------------------------- what the limiter saw
def limiter_branches(R: LevelRef, boxrefs, comps, ngs: int):
    """over the parents of the compared class-1 cells of a level (interp_type 1): how many have every limited slope zero, a common
    factor below 1, and non-zero slopes with factor 1"""
    par = np.zeros(tuple(s // 1 for s in R.keep[comps[0]]["alpha"].shape), dtype=bool)
    r = R.shape[0] // par.shape[0]
    for B in boxrefs:
        m = (B.cls == 1) & (B.layer <= ngs)
        kz, jy, ix = np.nonzero(m)
        par[B.widx[0][kz] // r, B.widx[1][jy] // r, B.widx[2][ix] // r] = True
    zero = lim = free = 0
    for c in comps:
        sl, alpha = R.keep[c]["sl"], R.keep[c]["alpha"]
        some = (sl[0] != 0.0) | (sl[1] != 0.0) | (sl[2] != 0.0)
        zero += int((par & ~some).sum())
        lim += int((par & some & (alpha < 1.0)).sum())
        free += int((par & some & (alpha == 1.0)).sum())
    return zero, lim, free
