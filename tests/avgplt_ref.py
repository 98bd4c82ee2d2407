"""An independent numpy restatement of the average of plotfiles with non-matching AMR (avgPlotfiles.cpp; the semantics the
project states for it: include/peleanalysis_amd.h, pa_resample_*) on DENSE arrays.

For file f and level l, V(f, l) is an array over the whole level-l domain: the file's own data where one of its level-l boxes
holds the cell, elsewhere the interpolant of V(f, l-1) (interp_type 0: the parent; 1: the cell-conservative linear rule of
FillPatchTwoLevels, written out below in the operation order of the kernels).  The average of level l is
(((0.0 + V(1,l)) + V(2,l)) + ... + V(nf,l)) * (1.0 / nf), in file order.  Arrays are [nz, ny, nx]."""
import numpy as np


def pad_coarse(c, is_per):
    """one layer around the domain: the wrapped cell across a periodic face, the nearest cell inside across a wall"""
    for ax, d in ((0, 2), (1, 1), (2, 0)):
        pw = [(0, 0)] * 3
        pw[ax] = (1, 1)
        c = np.pad(c, pw, mode="wrap" if is_per[d] else "edge")
    return c


def interp_dense(c, r, is_per, interp_type, keep=None):
    """the whole fine level (ratio r) interpolated from the dense coarse array c.  keep: a dict that receives the per-parent
    intermediates of interp_type 1 (`sl`: the three limited slopes, `alpha`: the common factor), for a caller that has to know
    which branches of the limiter its data reached"""
    nz, ny, nx = c.shape
    fine = np.empty((nz * r, ny * r, nx * r))
    if interp_type == 0:
        for cz in range(r):
            for cy in range(r):
                for cx in range(r):
                    fine[cz::r, cy::r, cx::r] = c
        return fine
    P = pad_coarse(c, is_per)

    def nb(dx, dy, dz):
        return P[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    u0 = nb(0, 0, 0)
    sl = []
    for d in range(3):  # x, y, z
        e = [int(d == 0), int(d == 1), int(d == 2)]
        um, up = nb(-e[0], -e[1], -e[2]), nb(e[0], e[1], e[2])
        dc = 0.5 * (up - um)
        df = 2.0 * (up - u0)
        db = 2.0 * (u0 - um)
        sx = np.where(df * db >= 0.0, np.minimum(np.abs(df), np.abs(db)), 0.0)
        sl.append(np.copysign(1.0, dc) * np.minimum(sx, np.abs(dc)))
    some = (sl[0] != 0.0) | (sl[1] != 0.0) | (sl[2] != 0.0)
    w = float(r - 1)
    dumax = np.abs(sl[0]) * w / float(2 * r) + np.abs(sl[1]) * w / float(2 * r) + np.abs(sl[2]) * w / float(2 * r)
    umax, umin = u0.copy(), u0.copy()
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                v = nb(dx, dy, dz)
                umin = np.where(v < umin, v, umin)
                umax = np.where(v > umax, v, umax)
    alpha = np.ones_like(u0)
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.where(some & (dumax * alpha > (umax - u0)), (umax - u0) / dumax, alpha)
        alpha = np.where(some & (dumax * alpha > (u0 - umin)), (u0 - umin) / dumax, alpha)
    if keep is not None:
        keep.update(sl=sl, alpha=alpha)
    for cz in range(r):
        for cy in range(r):
            for cx in range(r):
                acc = u0
                for d, rem in enumerate((cx, cy, cz)):
                    xoff = (float(rem) + 0.5) / float(r) - 0.5
                    acc = acc + xoff * (sl[d] * alpha)
                fine[cz::r, cy::r, cx::r] = acc
    return fine


def occupancy(boxes, shape):
    """bool[nz, ny, nx]: cells inside one of the boxes (rows lo0 lo1 lo2 hi0 hi1 hi2; the domain starts at 0)"""
    occ = np.zeros(shape, dtype=bool)
    for lo0, lo1, lo2, hi0, hi1, hi2 in np.asarray(boxes).reshape(-1, 6):
        occ[lo2:hi2 + 1, lo1:hi1 + 1, lo0:hi0 + 1] = True
    return occ


def dense_of(mf, comp, shape, out=None):
    """the valid cells of component comp of a host multifab on a dense array over the domain (cells of no box keep `out`)"""
    a = np.full(shape, np.nan) if out is None else out
    for b in range(mf.level.nboxes):
        lo0, lo1, lo2, hi0, hi1, hi2 = (int(x) for x in mf.level.boxes[b])
        a[lo2:hi2 + 1, lo1:hi1 + 1, lo0:hi0 + 1] = mf.valid(b)[comp]
    return a


def file_levels_dense(file_mfs, comps, nlev, n0, ratio, is_per, interp_type):
    """V(f, l) for l < nlev: a list over levels of arrays [nvar, nz, ny, nx].  file_mfs: the file's host multifabs, level 0
    first (possibly fewer than nlev); comps: file component of every variable"""
    out = []
    for l in range(nlev):
        n = n0 * ratio ** l
        lev = np.empty((len(comps), n, n, n))
        for v, c in enumerate(comps):
            a = interp_dense(out[l - 1][v], ratio, is_per, interp_type) if l > 0 else np.full((n, n, n), np.nan)
            if l < len(file_mfs):
                dense_of(file_mfs[l], c, (n, n, n), a)
            lev[v] = a
        out.append(lev)
    return out


def average(files, comps_per_file, nlev, n0, ratio, is_per, interp_type):
    """(averages, masks): per level l < nlev the average [nvar, nz, ny, nx] over the WHOLE domain -- the output holds it on the
    union of the files' boxes -- and that union as bool[nz, ny, nx].  files: per file the list of its host multifabs"""
    nf = len(files)
    acc = None
    for f, mfs in enumerate(files):
        V = file_levels_dense(mfs, comps_per_file[f], nlev, n0, ratio, is_per, interp_type)
        if acc is None:
            acc = [np.zeros_like(v) for v in V]
        for l in range(nlev):
            acc[l] = acc[l] + V[l]  # (0.0 + V1) + V2 + ...
    factor = 1.0 / float(nf)
    masks = []
    for l in range(nlev):
        n = n0 * ratio ** l
        m = np.zeros((n, n, n), dtype=bool)
        for mfs in files:
            if l < len(mfs):
                m |= occupancy(mfs[l].level.boxes, (n, n, n))
        masks.append(m)
    return [a * factor for a in acc], masks
