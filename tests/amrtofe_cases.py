"""The hierarchies of the amrToFE tests (CPU and GPU tier): the known-answer cases on an 8^3 unit cube, and the larger ones."""
import functools

import numpy as np

from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, field_flame, field_trig, fill_analytic, nested_hierarchy, union_hierarchy

import amrtofe_ref as R


def lv(boxes, n):
    """a level of the non-periodic unit cube with n^3 cells"""
    return Level(boxes, (0, 0, 0), (n - 1,) * 3, (0, 0, 0), np.zeros(3), np.ones(3))


BASE = [[0, 0, 0, 7, 7, 7]]
# name: (levels, ratios, box key, nodes, elements, the refinement stays off the wall and the box is the domain)
KNOWN = {
    "one": ([lv(BASE, 8)], [], None, 512, 343, True),
    "split_x4": ([lv([[0, 0, 0, 3, 7, 7], [4, 0, 0, 7, 7, 7]], 8)], [], None, 512, 343, True),
    "centred": ([lv(BASE, 8), lv([[4, 4, 4, 11, 11, 11]], 16)], [2], None, 960, 947, True),
    "centred_split_x8": ([lv(BASE, 8), lv([[4, 4, 4, 7, 11, 11], [8, 4, 4, 11, 11, 11]], 16)], [2], None, 960, 947, True),
    "L_shape": ([lv(BASE, 8), lv([[4, 4, 4, 11, 11, 7], [4, 4, 8, 7, 11, 11]], 16)], [2], None, 848, 823, True),
    "at_wall": ([lv(BASE, 8), lv([[0, 0, 0, 7, 7, 7]], 16)], [2], None, 960, 791, False),
    "ratio4": ([lv(BASE, 8), lv([[8, 8, 8, 23, 23, 23]], 32)], [4], None, 4544, 5131, True),
    "three": ([lv(BASE, 8), lv([[2, 2, 2, 13, 13, 13]], 16), lv([[8, 8, 8, 23, 23, 23]], 32)], [2, 2], None, 5608, 6381, True),
    "box_key": ([lv(BASE, 8), lv([[4, 4, 4, 11, 11, 11]], 16)], [2], (1, 1, 1, 4, 6, 6), 480, 486, False),
}


def _no_per(H):
    return [Level(l.boxes, l.domlo, l.domhi, (0, 0, 0), l.prob_lo, l.prob_hi) for l in H.levels]


def larger(name):
    """-> (levels, ratios, box key)"""
    if name.startswith("union"):
        H = union_hierarchy(int(name[5:]), nlev=3, n0=(16, 12, 20), is_per=(0, 0, 0))
    elif name == "nested16":
        H = nested_hierarchy(16, 3, 8, is_per=(0, 0, 0))
    elif name == "base32":  # the compaction spans several hundred workgroups, the element sort 32 key bits
        H = nested_hierarchy(32, 2, 16, is_per=(0, 0, 0))
    else:
        raise KeyError(name)
    levels = _no_per(H)
    return levels, [2] * (len(levels) - 1), None


LARGER = ("union3", "union9", "union10", "union11", "union12", "nested16", "base32")  # the seeds: two and three levels, 1 to 21 fine boxes


def case(name):
    if name in KNOWN:
        return KNOWN[name][:3]
    return larger(name)


@functools.lru_cache(maxsize=None)
def reference(name, finest_level=None, connect_cc=True, box=None):
    levels, ratios, key = case(name)
    return R.FeMeshRef(levels, ratios, box if box is not None else key, finest_level, connect_cc)


@functools.lru_cache(maxsize=None)
def states(name):
    """two components on the file's boxes: field_flame, field_trig"""
    out = []
    for l in case(name)[0]:
        m = MultiFab(l, 2, 0)
        fill_analytic(m, 0, lambda x, y, z: field_flame(x, y, z, 0) + 0 * (x + y + z))
        fill_analytic(m, 1, lambda x, y, z: field_trig(x, y, z, 1) + 0 * (x + y + z))
        out.append(m)
    return out


def hierarchy_of(name):
    levels, ratios, _ = case(name)
    return Hierarchy(list(levels), ratios[0] if ratios else 2)
