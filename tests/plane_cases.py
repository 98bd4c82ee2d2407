"""The case matrix of the plane tools (avgToPlane3d.ex / slicePlot3d.ex / pa_plane_*), shared by the CPU and the GPU tier.

All cases are tiny.  Every level holds three components "a", "b", "c" of normal x 10^uniform(-6, 6) values with mixed signs, drawn
independently per level: twelve decades in one column, so the order of the additions shows in the bits of the sum.  Every level's
grids are whole refined cells of the next coarser level's."""
import functools

import numpy as np

from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, chop_box

NAMES = ["a", "b", "c"]
DIRS = (0, 1, 2)


def _boxes(*specs):
    return np.vstack([chop_box(lo, hi, ms) for lo, hi, ms in specs]).astype(np.int32)


# name -> dict(n0 = base cells (x, y, z), ratios, boxes = per level a box list (level 0: the domain chopped to `base_box`),
#              max_grid_size, finest (default: the last level), box (default: the finest domain), seed, special)
_THREE = dict(n0=(8, 8, 8), ratios=[2, 2], base_box=4,
              boxes=[_boxes(((2, 2, 2), (9, 5, 13), 8), ((2, 6, 2), (5, 13, 13), 8)),  # an L in the x-y plane
                     _boxes(((6, 4, 8), (13, 9, 15), 8), ((4, 14, 10), (9, 21, 19), 8))])
_SPECS = {
    "single": dict(n0=(8, 8, 8), ratios=[], base_box=4, boxes=[], max_grid_size=4, seed=1),
    # 16 fine cells split 6, 5, 5: the cut between fine 10 and 11 splits coarse cell 5
    "uneven_chunks": dict(n0=(8, 8, 8), ratios=[2], base_box=8, boxes=[_boxes(((4, 4, 4), (11, 11, 11), 8))], max_grid_size=6, seed=2),
    "three_levels": dict(_THREE, max_grid_size=7, seed=3),
    # 16 fine cells split 3, 3, 3, 3, 2, 2: the cuts behind fine 2, 5, 8 and 13 lie inside the coarse cells 0, 1, 2 and 3
    "ratio4": dict(n0=(4, 4, 4), ratios=[4], base_box=4, boxes=[_boxes(((4, 4, 4), (11, 11, 11), 8))], max_grid_size=3, seed=4),
    # odd low corners, odd thickness in every direction (23, 19, 15)
    "subbox_odd": dict(_THREE, max_grid_size=5, seed=5, box=(3, 5, 7, 25, 23, 21)),
    "below_finest": dict(_THREE, max_grid_size=7, seed=6, finest=1),
    "thin": dict(n0=(8, 8, 8), ratios=[2], base_box=4, boxes=[_boxes(((4, 4, 4), (11, 11, 11), 8))], max_grid_size=6, seed=7, special="thin"),
    # 72 x 68 x 12 fine cells: no image size is a multiple of 64 or 16, partial tiles in both image directions for every dir
    "wide": dict(n0=(36, 34, 6), ratios=[2], base_box=16, boxes=[_boxes(((10, 8, 2), (49, 41, 9), 16))], max_grid_size=5, seed=8),
    "nan_inf": dict(n0=(8, 8, 8), ratios=[2], base_box=8, boxes=[_boxes(((4, 4, 4), (11, 11, 11), 8))], max_grid_size=6, seed=9, special="nan_inf"),
}
CASES = list(_SPECS)
THIN_INDEX = 5  # case thin: the sub-box is the finest domain at this index along dir


class Case:
    def __init__(self, name):
        s = _SPECS[name]
        self.name = name
        self.ratios = list(s["ratios"])
        self.max_grid_size = s["max_grid_size"]
        n0 = np.array(s["n0"])
        levels, r = [], 1
        for l in range(len(self.ratios) + 1):
            if l:
                r *= self.ratios[l - 1]
            b = _boxes(((0, 0, 0), tuple(n0 - 1), s["base_box"])) if l == 0 else s["boxes"][l - 1]
            levels.append(Level(b, (0, 0, 0), tuple(n0 * r - 1), (0, 0, 0), np.zeros(3), np.ones(3)))
        self.levels = levels
        self.hier = Hierarchy(levels, self.ratios[0] if self.ratios else 2)
        self.finest = s.get("finest", len(levels) - 1)
        self._box = s.get("box")
        self.special = s.get("special")
        rng = np.random.default_rng(1000 + s["seed"])
        self.mfs = []
        for lv in levels:
            m = MultiFab(lv, len(NAMES), 0)
            for b in range(lv.nboxes):
                v = m.valid(b)
                v[...] = rng.standard_normal(v.shape) * 10.0 ** rng.uniform(-6.0, 6.0, v.shape)
                if self.special == "thin":
                    v[rng.uniform(size=v.shape) < 0.3] = -0.0
            self.mfs.append(m)
        if self.special == "nan_inf":  # one NaN and one +inf cell of component 0 on the fine level, in different columns for every dir
            f = self.mfs[1].valid(0)
            f[0, 1, 2, 3] = np.nan
            f[0, 5, 6, 4] = np.inf

    @property
    def nlev(self):
        """levels that are used: 0 .. finestLevel"""
        return self.finest + 1

    def domain(self):
        lv = self.levels[self.finest]
        return tuple(int(x) for x in lv.domlo) + tuple(int(x) for x in lv.domhi)

    def subbox(self, dir):
        """the sub-box of the sum, in the finest level's indices (lo0 lo1 lo2 hi0 hi1 hi2)"""
        b = list(self._box or self.domain())
        if self.special == "thin":
            b[dir] = b[3 + dir] = THIN_INDEX
        return tuple(b)

    def sliceloc(self, dir):
        b = self.subbox(dir)
        return b[dir] + (2 * (b[3 + dir] - b[dir] + 1)) // 3

    def slicebox(self, dir):
        b = list(self.subbox(dir))
        b[dir] = b[3 + dir] = self.sliceloc(dir)
        return tuple(b)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


@functools.lru_cache(maxsize=None)
def reference(name, dir):
    """the reference results of a case and a direction, computed once and shared (read-only): dict with
    sum / slice [3][height][width] (components a, b, c), and for component 0 of each: mn, mx and the pixel levels"""
    import plane_ref as PR
    c = case(name)
    out = {}
    sb = c.subbox(dir)
    F, nosrc = PR.composite(c.levels[:c.nlev], c.mfs[:c.nlev], c.ratios[:c.finest], sb[:3], sb[3:], (0, 1, 2))
    assert nosrc == 0
    out["F"] = F
    out["sum"] = PR.plane_sum(F, dir, sb[dir], c.max_grid_size)
    lb = c.slicebox(dir)
    Fs, nosrc = PR.composite(c.levels[:c.nlev], c.mfs[:c.nlev], c.ratios[:c.finest], lb[:3], lb[3:], (0, 1, 2))
    assert nosrc == 0
    out["slice"] = PR.plane_slice(Fs, dir)
    for what in ("sum", "slice"):
        mn, mx = PR.minmax(out[what][0])
        out[what + "_minmax"] = (mn, mx)
        out[what + "_pix"] = PR.pixelize(out[what][0], mn, mx)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def palette_bytes(alpha=False):
    """a palette file: 256 r, 256 g, 256 b (and 256 alpha) bytes, all channels different"""
    i = np.arange(256)
    ch = [(i * 7 + 3) % 256, (255 - i), (i * 13 + 101) % 256] + ([(i * 3) % 256] if alpha else [])
    return np.concatenate(ch).astype(np.uint8).tobytes()
