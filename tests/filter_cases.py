"""One case matrix of the filter kernels (csrc/pa_filter.hip) for both tiers: tests/test_filter_ref.py holds the numpy references
of tests/filter_ref.py to the oracle on it, tests/test_gpu_filter_shapes.py holds the kernels to the references on it.

A case is a list of boxes on one level, a filter half-width ng with its weights, and the launch that pa_filter_last_launch must
report for it in either filter mode.  The shapes are the smallest that reach each branch of the launch rule sep_shape() and of the
kernels behind it; the expected launches were worked out from the rule by hand, shape by shape, and are written down as numbers.

Inputs: 4 components cut out of ONE dense field over the level's bounding box, log-uniform in magnitude over 1e-8 .. 2e3 with about
30 % negative values (a per-cell bound has something to check where the values are small; nothing comes near the streaming
kernel's denormal exception), with ng + 1 ghost layers of which the outermost holds NaN: a read past ng poisons the result.
"""
import dataclasses
import functools
import zlib

import numpy as np

import filter_ref as R
from peleanalysis_amd.hierarchy import Level, MultiFab, chop_box

NCOMP = 4                 # components of every input and output multifab
COMPS = (0, 1, 2)         # the components any variant filters: (scomp 0, ncomp 2) and (scomp 1, ncomp 2)
RANGES = ((0, 2), (1, 2))  # (scomp, ncomp)


# ------------------------------------------------------------------------------------------------------------- weights
def weights(wname, ng):
    """(ng, w): "box" = PelePhysics' box filter of fgr = 2 ng; "t3" / "t4" / "t8" = its filter types 3, 4 and 8 at fgr = 4 (one
    division of exact integers each: the same doubles however they are written); "tri" = triangular weights k / (ng + 1)^2, which
    are no box weights: the only way to the LDS tile kernel at ng = 4, and at ng 3 / 6 / 8 the only weights that differ from tap to tap"""
    if wname == "box":
        fgr = 2 * ng
        w = np.full(2 * ng + 1, 1.0 / fgr)
        w[0] = 0.5 * w[0]
        w[-1] = w[0]
        return ng, w
    f2, f4 = 16.0, 256.0
    if wname == "t3":
        assert ng == 1
        return 1, np.array([f2 / 24.0, (12.0 - f2) / 12.0, f2 / 24.0])
    if wname == "t4":
        assert ng == 2
        a, b, c = (3.0 * f4 - 20.0 * f2) / 5760.0, (80.0 * f2 - 3.0 * f4) / 1440.0, (3.0 * f4 - 100.0 * f2 + 960.0) / 960.0
        return 2, np.array([a, b, c, b, a])
    if wname == "t8":
        assert ng == 2
        a, b, c = (f4 - 4.0 * f2) / 1152.0, (16.0 * f2 - f4) / 288.0, (f4 - 20.0 * f2 + 192.0) / 192.0
        return 2, np.array([a, b, c, b, a])
    assert wname == "tri"
    k = np.concatenate([np.arange(1, ng + 2), np.arange(ng, 0, -1)]).astype(np.float64)
    return ng, k / float((ng + 1) ** 2)


FILTER_TYPE = {"t3": 3, "t4": 4, "t8": 8}  # filter_type of pa_filter_weights / orc_filter_weights, at fgr = 4


# --------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    boxes: tuple      # ((lo0, lo1, lo2, hi0, hi1, hi2), ...)
    ng: int
    wname: str
    sep: tuple        # pa_filter_last_launch in separable mode
    exa: tuple        # ... in exact mode
    variants: bool    # also through pa_boxfilter_fab (one box), into an output with a ghost layer, with scomp = 1
    dim: int = 3

    @property
    def id(self):
        return f"{self.name}-ng{self.ng}-{self.wname}"

    @property
    def maxn(self):
        b = np.asarray(self.boxes)
        return tuple(int(v) for v in (b[:, 3:] - b[:, :3] + 1).max(axis=0))

    @property
    def ng_have(self):
        return self.ng + 1


def _cdiv(a, b):
    return (a + b - 1) // b


def _tap_info(maxn, ng, wname, refused=0):
    """the tap-order kernels' tilings, which do not depend on the shape: streaming (box weights, ng 1 / 2 / 4) 32 x 8 columns and
    segments of 32 planes; LDS tile (other weights, ng 1 / 2 / 4) 32 x 8 x 8, at ng 4 32 x 8 x 4; any other width one thread per
    cell in tiles of 32 x 8 (boxes up to 32 wide) or 64 x 4 columns and 16 planes"""
    nx, ny, nz = maxn
    if ng in (1, 2, 4) and wname == "box":
        ks = min(32, nz)
        return (2, ng, 256, 8, _cdiv(ny, 8), ks, _cdiv(nz, ks), refused)
    if ng in (1, 2, 4):
        tz = 4 if ng == 4 else 8
        return (3, ng, 256, 8, _cdiv(ny, 8), tz, _cdiv(nz, tz), refused)
    ty = 8 if nx <= 32 else 4
    return (4, ng, 256, ty, _cdiv(ny, ty), 16, _cdiv(nz, 16), refused)


def _box(nx, ny, nz, lo=(0, 0, 0)):
    return (lo[0], lo[1], lo[2], lo[0] + nx - 1, lo[1] + ny - 1, lo[2] + nz - 1)


def _mk(name, boxes, ng, wname, sep, variants=True):
    """sep: (threads, TY, y strips, kseg, z segments) of the separable launch, or None where the rule refuses the shape"""
    boxes = tuple(tuple(int(v) for v in b) for b in boxes)
    c = Case(name, boxes, ng, wname, (), (), variants)
    exa = _tap_info(c.maxn, ng, wname)
    s = (1, ng) + tuple(sep) + (0,) if sep is not None else _tap_info(c.maxn, ng, wname, refused=1)
    return dataclasses.replace(c, sep=s, exa=exa)


def _cases():
    out = []
    # separable, 1024 threads: nx >= 66 with ny >= 16 (ng 4: 16 * 33 pairs do not fit 512 threads either)
    for ng in (3, 4, 6, 8):
        out.append(_mk("b66x16x5", [_box(66, 16, 5)], ng, "box", (1024, 16, 1, 5, 1)))
    # 1024 threads, odd nx (padded LDS row, scalar stores), the one strip 18 rows of TY = 20
    # (box weights are all equal between the ends: only the triangular ones tell the interior taps of these widths apart)
    for ng in (3, 6, 8):
        out.append(_mk("b67x18x5", [_box(67, 18, 5)], ng, "box", (1024, 20, 1, 5, 1)))
        out.append(_mk("b67x18x5", [_box(67, 18, 5)], ng, "tri", (1024, 20, 1, 5, 1)))
    # several z segments, the last one short: 140 = 8 * 16 + 12 = 4 * 32 + 12 = 2 * 64 + 12
    for ng, ks, nzs in ((1, 16, 9), (2, 16, 9), (3, 16, 9), (4, 32, 5), (6, 32, 5), (8, 64, 3)):
        out.append(_mk("b8x8x140", [_box(8, 8, 140)], ng, "box", (512, 8, 1, ks, nzs)))
        if ng in (3, 6, 8):
            out.append(_mk("b8x8x140", [_box(8, 8, 140)], ng, "tri", (512, 8, 1, ks, nzs)))
    # 1024 threads and 2 z segments together (the largest case: 74k cells)
    out.append(_mk("b66x16x70", [_box(66, 16, 70)], 8, "box", (1024, 16, 1, 35, 2)))
    # TY cut from 12 / 16 to 4: 3 full strips, or 4 strips of which the last has ONE row
    for ng in (1, 2, 3, 6):
        nt = 512 if ng <= 2 else 1024
        out.append(_mk("b300x12x3", [_box(300, 12, 3)], ng, "box", (nt, 4, 3, 3, 1)))
        out.append(_mk("b301x13x3", [_box(301, 13, 3)], ng, "box", (nt, 4, 4, 3, 1)))
    # degenerate boxes, fewer than 8 of them in the 8-wide block numbering
    for ng in (1, 2, 3, 4, 6, 8):
        out.append(_mk("tiny3", [_box(1, 1, 1), _box(2, 3, 1, (4, 0, 0)), _box(7, 5, 3, (10, 0, 0))], ng, "box", (512, 8, 1, 3, 1)))
    # the rule refuses (no strip of 4 rows of a 600-wide box fits): the streaming kernel, refused flag set
    for ng in (1, 2, 4):
        out.append(_mk("b600x8x2", [_box(600, 8, 2)], ng, "box", None, variants=False))
    # boxes narrower, shorter and shallower than maxn; odd nx beside even nx in one launch
    mixed = [_box(66, 16, 9), _box(21, 16, 9, (66, 0, 0)), _box(66, 7, 4, (0, 16, 0))]
    out.append(_mk("mixed3", mixed, 3, "box", (1024, 16, 1, 9, 1)))
    out.append(_mk("mixed3", mixed, 2, "box", (512, 16, 1, 9, 1)))
    # the tap-order kernels: partial tiles in x, y and z (33 x 9 x 9); 3 z segments of the streaming kernel (32, 32, 6)
    for ng, wn in ((1, "box"), (2, "box"), (4, "box"), (1, "t3"), (2, "t4"), (2, "t8"), (4, "tri")):
        out.append(_mk("b33x9x9", [_box(33, 9, 9)], ng, wn, (512, 12, 1, 9, 1)))
        sep = {1: (512, 16, 1, 16, 5), 2: (512, 16, 1, 16, 5), 4: (1024, 16, 1, 18, 4)}[ng]
        out.append(_mk("b66x16x70", [_box(66, 16, 70)], ng, wn, sep))
    # widths no specialisation has: the generic kernel in either mode (the separable rule refuses the width)
    for ng in (5, 7):
        out.append(_mk("chop19x13x10", chop_box((0, 0, 0), (18, 12, 9), 9), ng, "box", None, variants=False))
    return out


def _cases2d():
    out = []
    for ng in (1, 2, 3):
        for name, boxes in (("p33x9", chop_box((0, 0, 0), (32, 8, 0), 17)), ("p7x5", [_box(7, 5, 1)])):
            boxes = tuple(tuple(int(v) for v in b) for b in boxes)
            c = Case(name, boxes, ng, "box", (), (), False, dim=2)
            nx, ny, nz = c.maxn
            info = (5, ng, 256, 8 if nx <= 32 else 4, _cdiv(ny, 8 if nx <= 32 else 4), 16, 1, 0)
            out.append(dataclasses.replace(c, sep=info, exa=info))
    return out


CASES = _cases()
CASES_2D = _cases2d()
assert len({c.id for c in CASES + CASES_2D}) == len(CASES) + len(CASES_2D)

# one dense field as one box, as a ragged chop (23 / 22 / 22 wide, 9 + 9 rows, 6 + 5 planes): the tiling-invariance cases
INVARIANCE_DOMAIN = (67, 18, 11)
INVARIANCE_CHOP = 24
INVARIANCE_NG = (1, 2, 3, 4, 6, 8)


# --------------------------------------------------------------------------------------------------------------- inputs
def dense_field(seed_name, lo, hi, grow):
    """(NCOMP, nz, ny, nx) over the box lo .. hi grown by `grow`: 10^U[-8, log10 2000) with a negative sign on about 30 %"""
    rng = np.random.default_rng(zlib.crc32(seed_name.encode()))
    shape = (NCOMP,) + tuple(int(hi[d] - lo[d] + 1 + 2 * grow) for d in (2, 1, 0))
    mag = 10.0 ** rng.uniform(-8.0, np.log10(2.0e3), size=shape)
    return np.where(rng.random(shape) < 0.3, -mag, mag)


def level_of(boxes):
    b = np.asarray(boxes, dtype=np.int32).reshape(-1, 6)
    lo, hi = b[:, :3].min(axis=0), b[:, 3:].max(axis=0)
    return Level(b, lo, hi, (0, 0, 0), (0.0, 0.0, 0.0), tuple(float(v) for v in (hi - lo + 1)))


def cut_input(level, dense, dense_lo, ng_have, dim=3):
    """the input multifab: every FAB cut out of the dense field (whose cell (0, 0, 0) is dense_lo), then NaN into the outermost
    ghost layer -- for a 2-D level into every ghost plane in z as well, which the 2-D kernel has no business reading"""
    mf = MultiFab(level, NCOMP, ng_have)
    for b in range(level.nboxes):
        f = mf.fab(b)
        o = level.boxes[b, :3] - ng_have - np.asarray(dense_lo)
        nz, ny, nx = f.shape[1:]
        f[:] = dense[:, o[2]:o[2] + nz, o[1]:o[1] + ny, o[0]:o[0] + nx]
        f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1], f[:, :, :, 0], f[:, :, :, -1] = (np.nan,) * 6
        if dim == 2:
            f[:, :ng_have], f[:, -ng_have:] = np.nan, np.nan
    return mf


@functools.lru_cache(maxsize=None)
def _inputs(case):
    lv = level_of(case.boxes)
    g = case.ng_have
    dense = dense_field(case.name, lv.domlo, lv.domhi, g)
    mf = cut_input(lv, dense, lv.domlo - g, g, case.dim)
    mf.data.setflags(write=False)
    dense.setflags(write=False)
    return lv, mf, dense


def level(case):
    return _inputs(case)[0]


def input_mf(case):
    """the case's input multifab (shared and read-only: copy it before an in-place change)"""
    return _inputs(case)[1]


def dense(case):
    """the dense field the FABs were cut from, over the level's bounding box grown by ng + 1 (no NaN layer)"""
    return _inputs(case)[2]


# ----------------------------------------------------------------------------------------------------------- references
def _per_box(case, fn):
    mf = input_mf(case)
    return [{c: fn(np.ascontiguousarray(mf.fab(b)[c])) for c in COMPS} for b in range(mf.level.nboxes)]


@functools.lru_cache(maxsize=None)
def ref_tap(case):
    """[box][comp] -> tap_order (tap_order2d for a 2-D case)"""
    w = weights(case.wname, case.ng)[1]
    fn = R.tap_order2d if case.dim == 2 else R.tap_order
    return _per_box(case, lambda f: fn(f, case.ng_have, case.ng, w))


@functools.lru_cache(maxsize=None)
def ref_exact(case):
    """[box][comp] -> (sum, M) in extended precision"""
    w = weights(case.wname, case.ng)[1]
    return _per_box(case, lambda f: R.exact(f, case.ng_have, case.ng, w))


@functools.lru_cache(maxsize=None)
def ref_model(case):
    """[box][comp] -> sep_model"""
    w = weights(case.wname, case.ng)[1]
    return _per_box(case, lambda f: R.sep_model(f, case.ng_have, case.ng, w))


# ------------------------------------------------------------------------------------------------------------ assertions
def assert_bits(got, want, what):
    """got == want bit for bit (two 3-D arrays of one box and component); the message names the first cell that differs"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape, f"{what}: shapes {g.shape} and {w.shape}"
    bad = np.argwhere(g.view(np.int64) != w.view(np.int64))
    if len(bad):
        k, j, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} of {g.size} cells differ bit for bit, first at (i,j,k)=({i},{j},{k}) local: "
                             f"got {g[k, j, i]!r} want {w[k, j, i]!r}")


def assert_bound(got, tot, mag, ng, what):
    """|got - exact| <= 1.01 gamma_(4 ng + 6) M in EVERY cell, each against its own M"""
    ok = R.within_bound(got, tot, mag, ng)
    if not ok.all():
        bad = np.argwhere(~ok)
        k, j, i = bad[0]
        err = abs(np.longdouble(got[k, j, i]) - tot[k, j, i])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} cells outside the rounding bound, first at (i,j,k)=({i},{j},{k}) local: "
                             f"got {got[k, j, i]!r}, |got - exact| = {float(err):.3e} = {float(err / (R.U * mag[k, j, i])):.2f} u M, "
                             f"bound {1.01 * R.sep_bound(ng) / R.U:.2f} u M")
