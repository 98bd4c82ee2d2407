"""A dense numpy restatement of flattenAMRFile (flattenAMRFile.cpp:77-97; the semantics this project states for it:
include/peleanalysis_amd.h, pa_flatten_level) -- V(file, output_level) on the whole domain of that level.

Built on avgplt_ref.interp_dense and dense_of, which do not care about the shape; what is generalised here is the walk over the
levels of avgplt_ref.file_levels_dense, to domains that are not cubes.  The file's own cells are copied (numpy assignment keeps
their bits: a -0.0 and a NaN's payload survive), everything else is the interpolant of the level below.  Arrays are [nz, ny, nx]."""
import numpy as np

import avgplt_ref as AR


def level_shape(shape0, ratio, l):
    """(nz, ny, nx) of level l for a level-0 domain of shape0 = (nx, ny, nz) cells"""
    return tuple(int(n) * ratio ** l for n in reversed(shape0))


def file_levels_dense(file_mfs, comps, nlev, shape0, ratio, is_per, interp_type, keep=None):
    """V(f, l) for l < nlev: a list over levels of arrays [nvar, nz, ny, nx].  file_mfs: the file's host multifabs, level 0 first
    (levels from nlev on are ignored, as the reference ignores those finer than output_level); comps: file component of every
    variable; keep: a list that receives, per interpolated (level, variable), the limiter's intermediates of interp_type 1"""
    out = []
    for l in range(nlev):
        shp = level_shape(shape0, ratio, l)
        lev = np.empty((len(comps),) + shp)
        for v, c in enumerate(comps):
            if l > 0:
                k = {} if keep is not None and interp_type == 1 else None
                a = AR.interp_dense(out[l - 1][v], ratio, is_per, interp_type, keep=k)
                if k is not None:
                    keep.append(k)
            else:
                a = np.full(shp, np.nan)
            if l < len(file_mfs):
                AR.dense_of(file_mfs[l], c, shp, a)
            lev[v] = a
        out.append(lev)
    return out


def flatten(file_mfs, comps, output_level, shape0, ratio, is_per, interp_type):
    """the flattened level [nvar, nz, ny, nx] and the number of cells (per variable) that found no source data"""
    V = file_levels_dense(file_mfs, comps, output_level + 1, shape0, ratio, is_per, interp_type)[output_level]
    return V, no_source_cells(file_mfs, output_level, shape0, ratio)


def no_source_cells(file_mfs, output_level, shape0, ratio):
    """cells of the output level that neither the file's levels 0 .. output_level hold nor, recursively, a parent does"""
    have = None
    for l in range(output_level + 1):
        shp = level_shape(shape0, ratio, l)
        if have is not None:
            have = have.repeat(ratio, axis=0).repeat(ratio, axis=1).repeat(ratio, axis=2)
        else:
            have = np.zeros(shp, dtype=bool)
        if l < len(file_mfs):
            have = have | AR.occupancy(file_mfs[l].level.boxes, shp)
    return int((~have).sum())


def canonical_fab(dense, box, ng, is_per):
    """the FAB of `box` grown by ng from a dense level [nvar, nz, ny, nx]: a ghost cell holds the value of its canonical cell
    (wrapped across a periodic face, the nearest cell inside across a wall)"""
    idx = []
    for d in range(3):
        n = dense.shape[3 - d]
        i = np.arange(int(box[d]) - ng, int(box[3 + d]) + ng + 1)
        idx.append(np.mod(i, n) if is_per[d] else np.clip(i, 0, n - 1))
    return dense[:, idx[2][:, None, None], idx[1][None, :, None], idx[0][None, None, :]]
