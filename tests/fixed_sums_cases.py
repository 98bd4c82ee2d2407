"""Inputs of tests/test_gpu_fixed_sums.py: data that make the LOW limbs of the 192-bit sums visible in the rounded result, written into
the variables jpdf, conditionalMean and integral / rmsVel sum.  Everything here runs on the CPU: the hierarchies, the data families, the
restatements' keys and terms, and the visibility condition on the big-integer model (tests/test_fixed_sums_cases.py asserts it).

Every domain has power-of-two cell sizes, so a weight w (a cell volume, area or length, or conditionalMean's integer weight) is a power
of two and the term w * v is the bit pattern of v, scaled: the families are designed as TERMS in units of the accumulator's quantum
2^(k-157) (M < 2^k the declared magnitude) and divided by the weight of their cell.

A GROUP is the set of cells whose terms meet in one sum (a bin; for integral a slot of one level, whose sum read adds to those of the
other levels); a group has a CLASS: 0 "tiny" (|sum| < 2^(k-100): wholly inside limb 0), 1 "mid" (2^(k-93) <= |sum| < 2^(k-40): the
mantissa straddles limbs 0 / 1), 2 "free".  Families:
  cancel       pairs +A (1 + j 2^-52), -A (1 + j' 2^-52) of equal weight; j' = j (tiny: the sum is 0) or one pair differs (mid, free)
  cancel_tail  such pairs with j' = j, and one or two terms +-A 2^-e (a random 53-bit mantissa), e in 60 .. 104 by class
  range        every cell a random sign and mantissa, 1 .. 150 binades below A: low bits fall under the quantum (the model truncates)
  ties         B, odd 2^-53 B, (+-2^-100 B or nothing) among cancelling pairs: a tie of the one rounding, decided by the tail or to even
  chains       +2^a, -2^b1, -2^a, +2^b2 quanta (or +(2^a - 2^b1), -(2^a - 2^b2) where those are doubles): carries and borrows across
               both limb boundaries in the partial sums of any order"""
import functools
import math

import numpy as np

import fixed192_ref as F
import integral_ref as I
import stats_ref as R
from peleanalysis_amd.hierarchy import Hierarchy, Level, MultiFab, cell_centers, field_flame, nested_hierarchy

A = 1.0
FAMILIES = ("cancel", "cancel_tail", "range", "ties", "chains")
VISIBLE = ("cancel", "cancel_tail", "ties", "chains")  # the families the visibility condition is asserted over
CHAIN_A, CHAIN_B = F.CHAIN_A, F.CHAIN_B


# ----------------------------------------------------------------------------- hierarchies
@functools.lru_cache(maxsize=None)
def hierarchies():
    """nested / union / ratio4: the 16^3-base hierarchies of the statistics tests (union's domain is 16 x 20 x 16: its length in y is
    1.25); odd: one level whose boxes are 12 and 5 cells wide; wide: one box whose rows fill wavefronts (64 cells); tall: four levels,
    128 slots along a direction.  Every cell size is a power of two."""
    S = R.stats_hierarchies()
    out = {"nested": S["nested"], "ratio4": S["ratio4"], "tall": nested_hierarchy(16, 4, 8), "cube": nested_hierarchy(16, 1, 16)}
    out["union"] = Hierarchy([Level(lv.boxes, lv.domlo, lv.domhi, lv.is_per, lv.prob_lo, np.array([1.0, 1.25, 1.0])) for lv in S["union"].levels], S["union"].ref_ratio)
    bx = [[x0, y0, z0, x1, y0 + 7, z0 + 7] for z0 in (0, 8) for y0 in (0, 8) for x0, x1 in ((0, 11), (12, 16))]
    out["odd"] = Hierarchy([Level(bx, (0, 0, 0), (16, 15, 15), (1, 1, 0), np.zeros(3), np.array([17.0 / 16.0, 1.0, 1.0]))], 2)
    out["wide"] = Hierarchy([Level([[0, 0, 0, 63, 7, 7]], (0, 0, 0), (63, 7, 7), (1, 1, 0), np.zeros(3), np.array([4.0, 0.5, 0.5]))], 2)
    for name, H in out.items():
        for lv in H.levels:
            assert all(math.frexp(float(d))[0] == 0.5 for d in lv.dx), f"{name}: a cell size is not a power of two"
    widths = {int(b[3] - b[0] + 1) for b in out["odd"].levels[0].boxes}
    assert widths == {12, 5}
    return out


def cell_ids(H):
    """per level, per box: int64 [nz][ny][nx], a number of its own for every valid cell of the hierarchy -> (ids, how many)"""
    ids, n = [], 0
    for lv in H.levels:
        per = []
        for b in range(lv.nboxes):
            sh = lv.box_shape(b)
            m = int(np.prod(sh))
            per.append(np.arange(n, n + m, dtype=np.int64).reshape(sh))
            n += m
        ids.append(per)
    return ids, n


def scatter(states, comp, ids, by_id):
    for l, s in enumerate(states):
        for b in range(s.level.nboxes):
            s.valid(b)[comp] = by_id[ids[l][b]]


def smooth_states(H, ncomp, seed):
    """every component the flame field (300 .. 2000) + noise: the bin variable, the condition variable"""
    from util import make_states
    return make_states(H, ncomp, 0, lambda x, y, z, m: field_flame(x, y, z, 0), seed=seed)


# ----------------------------------------------------------------------------- the families
def _mant(rng):
    return float(int(rng.integers(1 << 52, 1 << 53)))


def special_terms(family, cls, sign, k, rng):
    """the terms of a group that do not come in cancelling pairs, in absolute units (see the module's docstring)"""
    q = k - 157
    pm = lambda: float(rng.choice((-1, 1)))
    if family == "cancel_tail":
        out = []
        for z in range(int(rng.integers(1, 3))):  # free: the first tail decides the sign of the sum, the second lies below it
            e, sg = ((int(rng.integers(103, 105)), pm()), (int(rng.integers(60, 92)), float(sign)),
                     (int(rng.integers(60, 81)), float(sign)) if z == 0 else (int(rng.integers(85, 105)), pm()))[cls]
            out.append(sg * math.ldexp(_mant(rng), k - 1 - e - 52))
        return out + [0.0] * (2 - len(out))
    if family == "ties":
        odd, tail = float(rng.choice((1, 3, 5, (1 << 20) + 1))), float(rng.choice((-1, 0, 1)))
        if cls == 0:  # 2^56 quanta + odd half-ulps of it +- 1 quantum
            t = [math.ldexp(1.0, q + 56), odd * math.ldexp(1.0, q + 3), tail * math.ldexp(1.0, q)]
        else:
            B = math.ldexp(1.0, k - 50 if cls == 1 else k - 30)
            t = [B, odd * 2.0 ** -53 * B, tail * 2.0 ** -100 * B]
        return [sign * x for x in t]
    if family == "chains":
        if cls == 0:
            a, (b1, b2) = int(rng.choice(CHAIN_A)), rng.permutation(CHAIN_B[:4])[:2]
        elif cls == 1:
            a, (b1, b2) = int(rng.choice(CHAIN_A[3:])), rng.permutation((int(rng.choice((63, 64))), 76))
        else:
            a = int(rng.choice(CHAIN_A))
            b1, b2 = (int(rng.choice([b for b in CHAIN_B if b < a])) for _ in range(2))
        b1, b2 = int(b1), int(b2)
        Q = lambda i: math.ldexp(float(i), q)
        if a - b1 <= 53 and a - b2 <= 53 and rng.random() < 0.5:
            t = [Q((1 << a) - (1 << b1)), 0.0, -Q((1 << a) - (1 << b2)), 0.0]
        else:
            t = [Q(1 << a), -Q(1 << b1), -Q(1 << a), Q(1 << b2)]
        return [sign * x for x in t]
    return []


def family_values(family, gid, w, cls, k, seed, sign=None):
    """values for the cells of one summed variable.  gid: the group of every cell; w: its weight (a power of two); cls: the class of its
    group; sign: +-1, the sign of its group's sum (default: alternating); k: M < 2^k for the declared magnitude M of the accumulator.
    -> v with w * v the designed terms, exactly"""
    rng = np.random.default_rng(seed)
    n = len(gid)
    w = np.asarray(w, dtype=np.float64)
    assert np.all(np.frexp(w)[0] == 0.5), "a weight is not a power of two"
    if family == "range":
        m = rng.integers(1 << 52, 1 << 53, size=n).astype(np.float64)
        return rng.choice((-1.0, 1.0), size=n) * np.ldexp(m, -52 - rng.integers(1, 151, size=n)) * A
    order = np.lexsort((w, gid))
    g, ww = np.asarray(gid)[order], w[order]
    t = np.zeros(n)
    gstart = np.concatenate([[0], np.nonzero(np.diff(g))[0] + 1]) if n else np.zeros(0, np.int64)
    gend = np.concatenate([gstart[1:], [n]])
    nsp = {"cancel": 0, "cancel_tail": 2, "ties": 3, "chains": 4}[family]
    special = np.zeros(n, bool)
    signs = {}
    for rank, (a, b) in enumerate(zip(gstart.tolist(), gend.tolist())):
        signs[a] = sg = (-1 if rank % 2 == 0 else 1) if sign is None else int(sign[order[a]])
        if nsp and b - a >= nsp:
            t[a:a + nsp] = special_terms(family, int(cls[order[a]]), sg, k, rng)
            special[a:a + nsp] = True
    # the other cells in pairs of equal weight within their group
    pos = np.nonzero(~special)[0]
    if len(pos) > 1:
        pg, pw = g[pos], ww[pos]
        new = np.concatenate([[True], (pg[1:] != pg[:-1]) | (pw[1:] != pw[:-1])])
        run = np.cumsum(new) - 1
        first = np.nonzero(new)[0]
        r = np.arange(len(pos)) - first[run]
        rlen = np.diff(np.concatenate([first, [len(pos)]]))[run]
        plus = np.nonzero((r % 2 == 0) & (r + 1 < rlen))[0]
        j = rng.integers(1 << 12, 1 << 20, size=len(plus)).astype(np.float64)
        jm = j.copy()
        if family == "cancel":  # one pair of every mid / free group leaves sign * d * w A 2^-52
            pgp = pg[plus]
            firstpair = np.nonzero(np.concatenate([[True], pgp[1:] != pgp[:-1]]))[0] if len(plus) else []
            for z in firstpair:
                a = int(np.searchsorted(g, pgp[z]))
                if int(cls[order[a]]) != 0:
                    jm[z] = j[z] - signs[a] * float(rng.integers(1, 1 << 10))
        t[pos[plus]] = pw[plus] * A * (1.0 + j * 2.0 ** -52)
        t[pos[plus + 1]] = -(pw[plus] * A * (1.0 + jm * 2.0 ** -52))
    v = np.zeros(n)
    v[order] = t / ww
    assert np.array_equal(v[order] * ww, t)
    return v


def k_of(M):
    return math.frexp(float(M))[1]


def visibility(per_bin):
    """per_bin: for every non-empty bin the exact integer sums (in quanta) of the accumulators that carry the family.  Every (bin, accumulator)
    is counted on its own -> (how many, of which wholly inside limb 0, of which with a mantissa that straddles limbs 0 / 1, is any sum negative)"""
    e = [v for b in per_bin for v in b]
    return len(e), sum(abs(v) < 1 << 57 for v in e), sum(1 << 64 <= abs(v) < 1 << 117 for v in e), any(v < 0 for v in e)


# ----------------------------------------------------------------------------- jpdf
JPDF_CASES = [("nested", 2, 3), ("union", 4, 3), ("ratio4", 2, 5), ("odd", 3, 5)]


@functools.lru_cache(maxsize=None)
def jpdf_case(hname, nvars, nbins, family, mode="tuple"):
    """the summed variables are the binned ones: odd nbins on the axis -2 nbins A .. 2 nbins A (bins 4 A wide), so the middle bin straddles
    zero and holds the family's values; a cell's variable sits in the middle bin or at (c - mid) 4 A (1 + j 2^-52) in bin c, by a pattern
    in space that keeps most cells in the middle bin of all variables but one.  Groups: the cells of one level with the same bins in all variables.  Class: tiny where v + nvars is even, mid where it is odd.
    mode one_bin: every variable of every cell in the middle bin; all_different: `cube`, 2 variables, 64 bins, every cell its own bin."""
    H = hierarchies()[hname]
    seed = sum(map(ord, hname + family + mode)) + 31 * nvars + nbins
    rng = np.random.default_rng(seed)
    ids, ncell = cell_ids(H)
    states = [MultiFab(lv, nvars, 0) for lv in H.levels]
    rr = R.ref_ratios(H)
    vols = [float((lv.dx[0] * lv.dx[1]) * lv.dx[2]) for lv in H.levels]
    if mode == "all_different":
        assert H.nlev == 1 and nvars == 2 and nbins == 64 and ncell == 4096
        c = np.arange(ncell)
        u = rng.integers(1 << 52, 1 << 53, size=(2, ncell)).astype(np.float64) * 2.0 ** -54  # 0.25 .. 0.5, every mantissa bit random
        scatter(states, 0, ids, (c // 64) + 0.25 + u[0])
        scatter(states, 1, ids, (c % 64) + 0.25 + u[1])
        vabs, vmin, vmax = [64.0, 64.0], [0.0, 0.0], [64.0, 64.0]
    else:
        mid = nbins // 2
        vabs, vmin, vmax = [2.0 * nbins * A] * nvars, [-2.0 * nbins * A] * nvars, [2.0 * nbins * A] * nvars
        pattern = np.array([mid, mid, 0, mid, mid, nbins - 1, mid, mid] if nbins == 3 else [mid, mid, 0, 1, mid, 3, 4, mid])
        cid, cw, cc, clev = [], [], [[] for _ in range(nvars)], []
        for l, lv in enumerate(H.levels):
            unc = R.uncovered(lv, H.levels[l + 1] if l + 1 < H.nlev else None, rr[l] if l + 1 < H.nlev else 1)
            for b in range(lv.nboxes):
                x, y, z = cell_centers(lv, b, 0)
                m = unc[b]
                seg = np.floor(8.0 * (x + 0.5 * y + 0.25 * z) + np.zeros(m.shape)).astype(np.int64)
                cid.append(ids[l][b][m])
                cw.append(np.full(int(m.sum()), vols[l]))
                clev.append(np.full(int(m.sum()), l))
                for v in range(nvars):
                    cc[v].append(pattern[(seg[m] + 2 * v) % 8] if mode == "tuple" else np.full(int(m.sum()), mid))
        cid, cw, clev = np.concatenate(cid), np.concatenate(cw), np.concatenate(clev)
        cc = [np.concatenate(c) for c in cc]
        gid = clev.copy()
        for v in range(nvars):
            gid = gid * nbins + cc[v]
        k = k_of(vols[0] * vabs[0])
        for v in range(nvars):
            inmid = cc[v] == mid
            val = (cc[v] - mid) * 4.0 * A * (1.0 + rng.integers(0, 1 << 20, size=len(cid)) * 2.0 ** -52)
            val[inmid] = family_values(family, gid[inmid], cw[inmid], np.full(int(inmid.sum()), (v + nvars) % 2), k, seed + 7 * v)
            assert np.all(np.abs(val[inmid]) < 2.0 * A)
            by_id = np.zeros(ncell)
            by_id[cid] = val
            scatter(states, v, ids, by_id)
    res = R.jpdf_accumulate(H, states, nvars, nbins, vmin, vmax)
    assert not res["outside"].any() and not res["nan"].any()
    return dict(H=H, states=states, nvars=nvars, nbins=nbins, vmin=vmin, vmax=vmax, vabs=vabs, res=res, vol_max=vols[0])


def jpdf_holds_every_term(case):
    """no term of any accumulator loses bits below its quantum: then the contract's bound applies as well"""
    s_vol, s_x = F.jpdf_scales(case["vol_max"], case["vabs"])
    res = case["res"]
    return all(F.all_convert_exactly(res["terms"][p][0], s_vol) and F.all_convert_exactly(res["terms"][p][1], s_x[a]) and F.all_convert_exactly(res["terms"][p][2], s_x[b])
               for p, (a, b) in enumerate(res["pairs"]))


def jpdf_visibility(case):
    res, nb2 = case["res"], case["nbins"] ** 2
    _, s_x = F.jpdf_scales(case["vol_max"], case["vabs"])
    per_bin = []
    for p, (a, b) in enumerate(res["pairs"]):
        x1 = F.sum_by_bin(res["keys"][p], res["terms"][p][1], s_x[a], nb2)
        x2 = F.sum_by_bin(res["keys"][p], res["terms"][p][2], s_x[b], nb2)
        per_bin += [[x1[q], x2[q]] for q in np.unique(res["keys"][p]).tolist()]
    return visibility(per_bin)


# ----------------------------------------------------------------------------- conditionalMean
# name: hierarchy, averaged components, bins, minima / maxima, the table the launcher chooses for the combined kernel (2 LDS, 1 global)
CONDMEAN_CASES = [("nested", 2, 16, False, 2), ("union", 4, 24, True, 2), ("ratio4", 8, 512, False, 1), ("odd", 1, 8, True, 2)]
BMIN, BMAX = 300.0, 2000.5


def condmean_mode(nbins, navg, with_minmax, uncombined):
    """pa_condmean_add_level's choice: 0 one set of global atomics per cell; 1 runs -> global table; 2 runs -> LDS table (<= 48 KB).
    A restatement of pa_stats.hip (the stride of pa_condmean_create, the 48 KB test of pa_condmean_add_level): the library does not report
    the mode, so this MUST TRACK the launcher -- change both together, or a path loses its cases without a test failing."""
    stride = 1 + 6 * navg + (2 * navg if with_minmax else 0)
    return 0 if uncombined else (2 if nbins * stride * 8 <= 48 * 1024 else 1)


@functools.lru_cache(maxsize=None)
def condmean_case(hname, navg, nbins, family, mode="field"):
    """component 0 bins (the flame field; one_bin: a constant; all_different: `cube`, the cell's number, 4096 bins); components 1 .. navg
    carry the family.  Groups: the bins.  Class of bin b for component a: (b + a) % 3, sign by (b + a) % 2."""
    H = hierarchies()[hname]
    seed = sum(map(ord, hname + family + mode)) + 31 * navg + nbins
    ids, ncell = cell_ids(H)
    states = smooth_states(H, 1 + navg, seed)
    bmin, bmax = BMIN, BMAX
    if mode == "one_bin":
        for s in states:
            s.data[:] = 1000.0
    if mode == "all_different":
        assert H.nlev == 1 and nbins == ncell
        scatter(states, 0, ids, np.arange(ncell) + 0.5)
        bmin, bmax = 0.0, float(ncell)
    scatter(states, 1, ids, np.arange(ncell, dtype=np.float64))
    r0 = R.condmean_accumulate(H, states, 0, [1], nbins, bmin, bmax)
    w = r0["w"].astype(np.float64)
    cid = (r0["terms_sum"][0] / w).astype(np.int64)
    assert len(np.unique(cid)) == len(cid) and np.array_equal(cid * w, r0["terms_sum"][0])
    vabs = [1.5 * A] * navg
    wmax = R.condmean_plan(H)[0]["weight"]
    k = k_of(float(wmax) * vabs[0])
    for a in range(navg):
        by_id = np.zeros(ncell)
        by_id[cid] = family_values(family, r0["keys"], w, (r0["keys"] + a) % 3, k, seed + 7 * a, sign=1 - 2 * ((r0["keys"] + a) % 2))
        scatter(states, 1 + a, ids, by_id)
    res = R.condmean_accumulate(H, states, 0, list(range(1, 1 + navg)), nbins, bmin, bmax)
    assert np.array_equal(res["keys"], r0["keys"])
    return dict(H=H, states=states, navg=navg, nbins=nbins, bmin=bmin, bmax=bmax, vabs=vabs, res=res, weight_max=wmax)


def condmean_holds_every_term(case):
    s_sum, s_sq = F.condmean_scales(case["weight_max"], case["vabs"])
    res = case["res"]
    return all(F.all_convert_exactly(res["terms_sum"][a], s_sum[a]) and F.all_convert_exactly(res["terms_sq"][a], s_sq[a]) for a in range(case["navg"]))


def condmean_visibility(case):
    res = case["res"]
    s_sum, _ = F.condmean_scales(case["weight_max"], case["vabs"])
    sums = [F.sum_by_bin(res["keys"], res["terms_sum"][a], s_sum[a], case["nbins"]) for a in range(case["navg"])]
    return visibility([[s[b] for s in sums] for b in np.unique(res["keys"]).tolist()])


# ----------------------------------------------------------------------------- integral / rmsVel
KIND_DIR = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2), (3, 0)]
INT_HIERS = ("nested", "union", "ratio4", "odd")


def integral_paths(H, kind, dir_, nrows, uncombined, finest_level=None):
    """pa_integral_add_level's choices per level -> set of (wavefront sum: none / end / tile / step, table: 0 per cell, 1 global, 2 LDS).
    A restatement of pa_integral.hip (PA_INT_LDS_MAX = 32 KB, rows of whole wavefronts = every box a multiple of 64 wide, the stride of
    pa_integral_create): the library does not report its choice, so this MUST TRACK the launcher -- change both together."""
    fl = H.nlev - 1 if finest_level is None else finest_level
    out = set()
    for lv in H.levels[:fl + 1]:
        n = (lv.domhi - lv.domlo + 1).astype(np.int64)
        wr = "end" if kind == 3 else (("tile" if dir_ != 0 else "none") if kind == 2 else ("step" if dir_ == 0 else "none"))
        nslots = 1 if kind == 3 else (int(n[dir_]) if kind == 2 else int(n[(dir_ + 1) % 3] * n[(dir_ + 2) % 3]))
        lds = nslots * (1 + 3 * (nrows - 1)) * 8
        rows_of_waves = all((int(b[3]) - int(b[0]) + 1) % 64 == 0 for b in lv.boxes)
        mode = 2 if kind == 3 or (kind == 2 and not (dir_ != 0 and rows_of_waves) and lds <= 32 * 1024) else 1
        out.add(("none", 0) if uncombined else (wr, mode))
    return out


@functools.lru_cache(maxsize=None)
def integral_case(hname, kind, dir_, nv, family, squares=False, cond=False):
    """variables 0 .. nv-1 carry the family; with cond one more variable, the flame field, is the condition (and is summed like the others).
    Groups: the cells of one level in one slot of that level.  Class of a group for variable n: (the level-0 slot c above it + n) % 3, sign by (c + n) % 2."""
    H = hierarchies()[hname]
    seed = sum(map(ord, hname + family)) + 31 * nv + 7 * kind + dir_ + (100 if squares else 0) + (200 if cond else 0)
    ids, ncell = cell_ids(H)
    ncomp = nv + (1 if cond else 0)
    states = smooth_states(H, ncomp, seed)
    comps = list(range(ncomp))
    kw = dict(ccomp=nv, cmin=299.0, cmax=1990.0) if cond else {}
    scatter(states, 0, ids, np.arange(ncell, dtype=np.float64))
    r0 = I.integrate(H, states, comps, kind, dir_, **kw)
    w = np.asarray(r0["terms"][0])
    kid = (r0["terms"][1] / w).astype(np.int64)
    assert np.array_equal(kid * w, r0["terms"][1])
    minkey = np.full(ncell, np.iinfo(np.int64).max)
    np.minimum.at(minkey, kid, r0["keys"])
    wid = np.zeros(ncell)
    wid[kid] = w
    cid = np.unique(kid)
    lev = np.searchsorted(np.unique(w), wid[cid])
    mk = minkey[cid]
    R0 = r0["R"][0]
    coarse = np.zeros(len(cid), np.int64) if kind == 3 else (mk // R0 if kind == 2 else (mk // r0["shape"][1] // R0) * 4096 + (mk % r0["shape"][1]) // R0)
    vabs = [1.5 * A] * nv + ([4096.0] if cond else [])
    k = k_of(max(r0["weights"]) * vabs[0])
    for n in range(nv):
        by_id = np.zeros(ncell)
        by_id[cid] = family_values(family, mk * H.nlev + lev, wid[cid], (coarse + n) % 3, k, seed + 7 * n, sign=2 * ((coarse + n) % 2) - 1)
        scatter(states, n, ids, by_id)
    res = I.integrate(H, states, comps, kind, dir_, squares=squares, **kw)
    assert np.array_equal(res["keys"], r0["keys"])
    return dict(H=H, states=states, comps=comps, kind=kind, dir=dir_, nv=nv, squares=squares, kw=kw, vabs=vabs, res=res, w_max=max(r0["weights"]))


def integral_holds_every_term(case):
    _, s_row = F.integral_scales(case["w_max"], case["vabs"], case["squares"])
    return all(F.all_convert_exactly(case["res"]["terms"][1 + r], s_row[r]) for r in range(len(s_row)))


def integral_visibility(case):
    res = case["res"]
    _, s_row = F.integral_scales(case["w_max"], case["vabs"], case["squares"])
    sums = [F.sum_by_bin(res["keys"], res["terms"][1 + n], s_row[n], res["nslots"]) for n in range(case["nv"])]
    return visibility([[s[b] for s in sums] for b in np.unique(res["keys"]).tolist()])


def integral_cases():
    """every family through every kind and direction; the hierarchy, the rows of squares and the condition window rotate"""
    out = []
    for f, fam in enumerate(FAMILIES):
        for q, (kind, dir_) in enumerate(KIND_DIR):
            z = f + q
            out.append((INT_HIERS[z % 4], kind, dir_, 3 if kind > 1 else 2, fam, bool((z // 2) % 2), bool(z % 2)))
    return out


# ----------------------------------------------------------------------------- the visibility condition over the cases of a kernel
def pooled_visibility(kernel):
    """-> (bins, tiny, mid) summed over the cancel*, ties and chains cases of a kernel, and the cases without a negative sum"""
    tot, no_negative = np.zeros(3, np.int64), []
    if kernel == "jpdf":
        todo = [(jpdf_visibility, jpdf_case, (h, nv, nb, fam)) for h, nv, nb in JPDF_CASES for fam in VISIBLE]
    elif kernel == "condmean":
        todo = [(condmean_visibility, condmean_case, (h, na, nb, fam)) for h, na, nb, _, _ in CONDMEAN_CASES for fam in VISIBLE]
    else:
        todo = [(integral_visibility, integral_case, c) for c in integral_cases() if c[4] in VISIBLE]
    for vis, build, args in todo:
        n, tiny, mid, neg = vis(build(*args))
        tot += (n, tiny, mid)
        if not neg:
            no_negative.append(args)
    return tuple(int(x) for x in tot), no_negative
