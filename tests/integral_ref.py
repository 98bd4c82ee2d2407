"""numpy restatement of the reference's composite integrals -- integral.cpp (integrate1d / integrate2d / integrate3d, the mask of cells
under a finer level, the condition window, avg, the .dat and .ppm writers) -- and of the moments of rmsVel.cpp, from
peleanalysis_amd.hierarchy objects.  Reference lines are cited at every step; no text of the reference is used.

As for the binned statistics (tests/stats_ref.py) there is no golden file from the reference itself: neither tool compiles without
AMReX.  Known answers (tests/test_integral_ref.py) take its place.  The reference adds cell after cell in the order of its loops; next
to those serial sums every function returns, per output slot, the TERMS that go into it, so that a test can form math.fsum(t) and
sum |t| per slot: the bound of the numerics contract, |S - fsum(t)| <= n 2^-53 sum |t|, holds for any order of additions."""
import math

import numpy as np

from stats_ref import EPS, fsum_by_bin, ref_ratios, uncovered  # noqa: F401


# ----------------------------------------------------------------------------- geometry
def cum_ratios(H, finest_level):
    """refRatio of integral.cpp:20-22, :79-83 for every level: the product of the refinement ratios from the level to finestLevel"""
    rr = ref_ratios(H)
    R = [1] * (finest_level + 1)
    for l in range(finest_level - 1, -1, -1):
        R[l] = R[l + 1] * rr[l]
    return R


def level_weight(lev, kind, dir_):
    """dzLev (:21), areaLev (:80-82) or volLev (:124-127) of a level"""
    dx = lev.dx
    if kind == 3:
        return float((dx[0] * dx[1]) * dx[2])
    if kind == 2:
        return float(dx[(dir_ + 1) % 3] * dx[(dir_ + 2) % 3])
    return float(dx[dir_])


def out_shape(H, kind, dir_, finest_level):
    """the output arrays of integral.cpp:442-449, :497-501, :520 at the resolution of finestLevel"""
    lev = H.levels[finest_level]
    n = (lev.domhi - lev.domlo + 1).astype(np.int64)
    if kind == 3:
        return ()
    if kind == 2:
        return (int(n[dir_]),)
    return (int(n[(dir_ + 1) % 3]), int(n[(dir_ + 2) % 3]))


def domain_box(H, finest_level):
    lev = H.levels[finest_level]
    return tuple(int(v) for v in lev.domlo) + tuple(int(v) for v in lev.domhi)


# ----------------------------------------------------------------------------- integrate1d / 2d / 3d
def integrate(H, states, comps, kind, dir_=0, finest_level=None, ccomp=-1, cmin=0.0, cmax=0.0, squares=False):
    """integral.cpp:415-436 (the mask) and :13-149 (the three integrators) before the avg division.  comps: the components of `states`
    that are vars[0 .. nVars-1]; ccomp indexes comps (cComp, :362-366).  squares adds the rows (v * v) * w of rmsVel.cpp:109-111.
    -> dict: shape, nslots, keys (fine slot of every contribution, in the reference's visiting order), terms [nrows] (row 0: the
    weights), out [nrows] + shape (the serial sums in that order), weights [nlev], R [nlev]"""
    fl = H.nlev - 1 if finest_level is None else finest_level
    rr = ref_ratios(H)
    R = cum_ratios(H, fl)
    shape = out_shape(H, kind, dir_, fl)
    nslots = int(np.prod(shape, dtype=np.int64))
    nv = len(comps)
    nrows = 1 + nv * (2 if squares else 1)
    d1, d2 = (dir_ + 1) % 3, (dir_ + 2) % 3
    keys, terms = [], [[] for _ in range(nrows)]
    weights = [level_weight(H.levels[l], kind, dir_) for l in range(fl + 1)]
    order = range(fl + 1) if kind == 3 else range(fl, -1, -1)  # :123 against :20, :79
    for l in order:
        lev = H.levels[l]
        w = weights[l]
        unc = uncovered(lev, H.levels[l + 1] if l < fl else None, rr[l] if l < fl else 1)  # :425-436; finestLevel is never masked
        for b in range(lev.nboxes):
            v = states[l].valid(b)
            m = unc[b].copy()
            if ccomp >= 0:  # :28, :89, :133: a NaN fails both comparisons
                with np.errstate(invalid="ignore"):
                    cv = v[comps[ccomp]]
                    m &= (cv >= cmin) & (cv < cmax)
            kk, jj, ii = np.nonzero(m)  # k slowest: the order of AMREX_PARALLEL_FOR_3D on the host
            idx = [ii + int(lev.boxes[b, 0]) - int(lev.domlo[0]), jj + int(lev.boxes[b, 1]) - int(lev.domlo[1]), kk + int(lev.boxes[b, 2]) - int(lev.domlo[2])]
            r = R[l]
            if kind == 3:
                slot = np.zeros(len(ii), np.int64)[:, None]
            elif kind == 2:  # :93-97
                slot = r * idx[dir_][:, None] + np.arange(r)[None, :]
            else:            # :32-37
                s1 = r * idx[d1][:, None, None] + np.arange(r)[None, :, None]
                s2 = r * idx[d2][:, None, None] + np.arange(r)[None, None, :]
                slot = (s1 * shape[1] + s2).reshape(len(ii), r * r)
            rep = slot.shape[1]
            keys.append(slot.ravel())
            terms[0].append(np.full(len(ii) * rep, w))
            with np.errstate(all="ignore"):
                for n, c in enumerate(comps):
                    val = v[c][m]
                    terms[1 + n].append(np.repeat(w * val, rep))  # :36, :96, :136: one rounded product
                    if squares:
                        terms[1 + nv + n].append(np.repeat((val * val) * w, rep))  # rmsVel.cpp:109-111: ux*ux*dxyz
    keys = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    terms = [np.concatenate(t) if t else np.zeros(0) for t in terms]
    out = np.zeros((nrows, max(nslots, 1)))
    with np.errstate(all="ignore"):
        for r_ in range(nrows):
            out[r_] = np.bincount(keys, weights=terms[r_], minlength=nslots)  # adds in input order
    return dict(shape=shape, nslots=nslots, keys=keys, terms=terms, out=out.reshape((nrows,) + shape), weights=weights, R=R, nrows=nrows)


def measure_exact(res, H, finest_level=None):
    """row 0 as the correctly rounded exact sum: every slot holds count_l cells of weight w_l per level; the exact rational sum is
    formed with fractions and rounded once"""
    from fractions import Fraction
    nslots = res["nslots"]
    w = np.asarray(res["terms"][0])
    out = np.zeros(nslots)
    order = np.argsort(res["keys"], kind="stable")
    k, t = res["keys"][order], w[order]
    cuts = np.searchsorted(k, np.arange(nslots + 1))
    for s in range(nslots):
        seg = t[cuts[s]:cuts[s + 1]]
        if len(seg):
            vals, cnt = np.unique(seg, return_counts=True)
            out[s] = float(sum(Fraction(float(v)) * int(c) for v, c in zip(vals, cnt)))
    return out.reshape(res["shape"])


def ieee_sum_rule(terms):
    """what IEEE addition returns for these terms in ANY order when one of them is not finite, else None: NaN if a NaN or both
    infinities are among them, otherwise the infinity that is"""
    t = np.asarray(terms, dtype=np.float64)
    nan, pinf, ninf = bool(np.isnan(t).any()), bool(np.isposinf(t).any()), bool(np.isneginf(t).any())
    if nan or (pinf and ninf):
        return float("nan")
    if pinf:
        return float("inf")
    if ninf:
        return float("-inf")
    return None


def split_nonfinite(keys, terms, nslots):
    """-> (special {slot: value by ieee_sum_rule}, keys and terms with the contributions of those slots removed)"""
    t = np.asarray(terms, dtype=np.float64)
    bad = np.unique(keys[~np.isfinite(t)])
    special = {int(s): ieee_sum_rule(t[keys == s]) for s in bad}
    keep = ~np.isin(keys, bad)
    return special, keys[keep], t[keep]


def apply_avg(out):
    """:51-58, :107-112, :143-147: rows 1.. divided by row 0 where row 0 > 0"""
    o = np.array(out, dtype=np.float64, copy=True)
    pos = o[0] > 0.0
    with np.errstate(all="ignore"):
        for n in range(1, o.shape[0]):
            o[n] = np.where(pos, o[n] / o[0], o[n])
    return o


def coords(H, d, finest_level):
    """:60-70, :114-118: plo[d] + (i + 0.5) * dxFine"""
    lev = H.levels[finest_level]
    n = int(lev.domhi[d] - lev.domlo[d] + 1)
    dx = float(lev.dx[d])
    return np.array([float(lev.prob_lo[d]) + (i + 0.5) * dx for i in range(n)])


# ----------------------------------------------------------------------------- names and writers
def to_string(v):
    """std::to_string(double)"""
    return "%f" % v


def outfile_name(infile, kind, dir_, cvar="", cmin=0.0, cmax=0.0, avg=0):
    """:403-412"""
    s = infile + "_integral"
    if kind < 3:
        s += "_dir" + str(dir_)
    if cvar:
        s += "_c" + cvar + "_" + to_string(cmin) + "_" + to_string(cmax)
    if avg:
        s += "_avg"
    return s


def write_dat_1d(v):
    """:226-233: no newline"""
    return "".join("%e " % x for x in v)


def write_dat_2d(a):
    """:235-245"""
    return "".join("".join("%e " % x for x in row) + "\n" for row in a)


def colour_of(val, vmin, vmax):
    """:253: fmax(0., fmin(1.5, (val - vMin) / (vMax - vMin))) -- fmin / fmax return the other argument for a NaN"""
    with np.errstate(all="ignore"):
        q = (np.float64(val) - np.float64(vmin)) / (np.float64(vmax) - np.float64(vmin))
    return float(np.fmax(0.0, np.fmin(1.5, q)))


def rgb_of(colour, go_past_max):
    """:254-296, the branches in their order; (int) truncates"""
    c = colour
    if c < 0.125:
        return (0, 0, int((c + 0.125) * 1020.))
    if c < 0.375:
        return (0, int((c - 0.125) * 1020.), 255)
    if c < 0.625:
        return (int((c - 0.375) * 1020.), 255, int((0.625 - c) * 1020.))
    if c < 0.875:
        return (255, int((0.875 - c) * 1020.), 0)
    if c < 1.000:
        return (int((1.125 - c) * 1020.), 0, 0)
    if go_past_max == 1:
        if c < 1.125:
            return (int((c - 0.875) * 1020.), 0, int((c - 1.000) * 1020.))
        if c < 1.250:
            return (255, 0, int((c - 1.000) * 1020.))
        if c < 1.500:
            return (255, int((c - 1.250) * 1020.), 255)
        return (255, 255, 255)
    return (128, 0, 0)


def write_ppm(a, go_past_max, vmin, vmax):
    """:247-304: P6, dim2 wide and dim1 high, row i of the array in image row dim1 - i - 1"""
    a = np.asarray(a, dtype=np.float64)
    d1, d2 = a.shape
    buf = bytearray(3 * d1 * d2)
    for i in range(d1):
        for j in range(d2):
            bc = ((d1 - i - 1) * d2 + j) * 3
            r, g, b = rgb_of(colour_of(a[i, j], vmin, vmax), go_past_max)
            buf[bc], buf[bc + 1], buf[bc + 2] = r & 255, g & 255, b & 255
    return ("P6\n%i %i\n255\n" % (d2, d1)).encode() + bytes(buf)


def find_min_max(a):
    """:306-316: strict comparisons from a[0][0] -- a NaN never replaces, a leading NaN stays"""
    a = np.asarray(a, dtype=np.float64)
    mn = mx = float(a[0, 0])
    for v in a.ravel():
        if v < mn:
            mn = float(v)
        if v > mx:
            mx = float(v)
    return mn, mx


def integral_files(outfile, kind, dir_, names, out, H, finest_level, fmt="dat", go_past_max=1, useminmax=None):
    """:453-529: {file name: text or bytes} from the finished array `out` (after avg).  useminmax: {n (from 1): (vMin, vMax)}"""
    files = {}
    nv = len(names)
    if kind == 1:
        if fmt == "dat":
            files[outfile + "_x.dat"] = write_dat_1d(coords(H, (dir_ + 1) % 3, finest_level))
            files[outfile + "_y.dat"] = write_dat_1d(coords(H, (dir_ + 2) % 3, finest_level))
            files[outfile + "_length.dat"] = write_dat_2d(out[0])
            for n in range(nv):
                files[outfile + "_" + names[n] + ".dat"] = write_dat_2d(out[1 + n])
        else:
            mm = [find_min_max(out[0])]
            for n in range(1, nv + 1):
                mm.append(tuple(useminmax[n]) if useminmax and n in useminmax else find_min_max(out[n]))
            files[outfile + "_length.ppm"] = write_ppm(out[0], go_past_max, *mm[0])
            for n in range(nv):
                files[outfile + "_" + names[n] + ".ppm"] = write_ppm(out[1 + n], go_past_max, *mm[1 + n])
    elif kind == 2:
        files[outfile + "_x.dat"] = write_dat_1d(coords(H, dir_, finest_level))
        files[outfile + "_allVars.dat"] = write_dat_2d(out)
    else:
        files[outfile + "_allVars.dat"] = write_dat_1d(out)
    return files


def integral_stdout(infile, names, kind, nlev_loaded, fmt="dat", useminmax=None):
    """every line integral.cpp prints, in its order"""
    nv = len(names)
    s = "infile = %s\nnVars= %d\n" % (infile, nv)
    s += "".join("var[%d]= %s\n" % (n, names[n]) for n in range(nv))
    s += "integralDimension = %d\n" % kind
    for l in range(nlev_loaded):
        s += "Loading data on level %d\nData loaded\n" % l
    s += "Determining intersects...\nIntersects determined\n"
    for l in (range(nlev_loaded) if kind == 3 else range(nlev_loaded - 1, -1, -1)):
        s += "Integrating level %d\n" % l
    s += "Integration completed\nWriting data as %s\n" % (fmt if kind == 1 else "dat")
    if kind == 1 and fmt == "ppm":
        for n in range(1, nv + 1):
            s += "Reading min/max from command line\n" if useminmax and n in useminmax else "Using file values for min/max\n"
    return s


# ----------------------------------------------------------------------------- rmsVel.cpp
def rmsvel(H, states, comps=(0, 1, 2), finest_level=None):
    """rmsVel.cpp:55-126 for one plotfile: the boxes of finestLevel ONLY -- no composite, no mask (:72-78) -- weight dx*dy*dz of that
    level (:68).  -> dict: the integrate() result of that single level with squares, sums7 = fsum of the seven rows (vol, uxb, uyb,
    uzb, ux2, uy2, uz2), urms through the host arithmetic of :123-125, kappa = (the six moments) / (3 urms^2)"""
    fl = H.nlev - 1 if finest_level is None else min(finest_level, H.nlev - 1)
    lev = H.levels[fl]
    dx = lev.dx
    dxyz = float(dx[0] * dx[1] * dx[2])
    keys, terms = [], [[] for _ in range(7)]
    for b in range(lev.nboxes):
        v = states[fl].valid(b)
        n = v[comps[0]].size
        terms[0].append(np.full(n, dxyz))
        for q, c in enumerate(comps):
            u = v[c].ravel()
            terms[1 + q].append(u * dxyz)         # :106-108
            terms[4 + q].append((u * u) * dxyz)   # :109-111
        keys.append(np.zeros(n, np.int64))
    keys = np.concatenate(keys)
    terms = [np.concatenate(t) for t in terms]
    sums7 = [math.fsum(t) for t in terms]
    urms, kappa = rmsvel_finish(sums7)
    return dict(keys=keys, terms=terms, sums7=sums7, urms=urms, kappa=kappa, level=fl, dxyz=dxyz)


def rmsvel_finish(s7):
    """:123-125 in their order"""
    vol = s7[0]
    uxb, uyb, uzb = s7[1] / vol, s7[2] / vol, s7[3] / vol
    ux2, uy2, uz2 = s7[4] / vol, s7[5] / vol, s7[6] / vol
    var3 = (ux2 - uxb * uxb) + (uy2 - uyb * uyb) + (uz2 - uzb * uzb)
    urms = math.sqrt(var3 / 3.) if var3 >= 0 else float("nan")
    with np.errstate(all="ignore"):
        kappa = (ux2 + uy2 + uz2 + uxb * uxb + uyb * uyb + uzb * uzb) / (3. * urms * urms) if urms > 0 else float("inf")
    return urms, kappa


def rmsvel_file(times, urms):
    """:130-135"""
    return "".join("%e %e\n" % (t, u) for t, u in zip(times, urms))


def rmsvel_stdout(infiles, finest_levels_printed):
    """:41-42, :61-62, :76-77, :127-128; finest_levels_printed[i]: the level printed for file i, or None"""
    s = "".join("Loading %s\n" % f for f in infiles)
    for i in range(len(infiles)):
        if finest_levels_printed[i] is not None:
            s += "Finest level: %d\n" % finest_levels_printed[i]
        s += "Processing %d/%d\n" % (i, len(infiles))
    return s + "   ...done.\n"


# ----------------------------------------------------------------------------- inputs shared by the CPU and the GPU tier
def ppm_case():
    """the image the GPU tier checks: smooth inputs, so that the colour map does not change across the bound's bracket"""
    from stats_ref import stats_hierarchies
    from peleanalysis_amd.hierarchy import field_flame
    from util import make_states
    H = stats_hierarchies()["nested"]
    st = make_states(H, 2, 0, field_flame)
    return H, st



def ppm_bracket_pixels(res, avg, go_past_max=1):
    """-> (pixels, pixels whose colour differs between the ends, the rgb arrays at both ends) for rows 1.. of a kind-1 result with
    findMinMax scaling; the bracket of a sum is fsum +- n 2^-53 sum|t|, of a quotient the propagated one, of vMin / vMax their own"""
    ns = res["nslots"]
    e0 = fsum_by_bin(res["keys"], res["terms"][0], ns)[0]
    total = differ = 0
    ends = []
    for r in range(1, res["nrows"]):
        ex, sa, n, _ = fsum_by_bin(res["keys"], res["terms"][r], ns)
        d = n * EPS * sa
        lo, hi = ex - d, ex + d
        if avg:
            with np.errstate(all="ignore"):
                q = np.where(e0 > 0, ex / e0, ex)
                dq = np.where(e0 > 0, d / e0 + 2 * EPS * np.abs(q), d)
            lo, hi = q - dq, q + dq
        rgb = []
        for a, mm in ((lo, (lo.min(), lo.max())), (hi, (hi.min(), hi.max()))):
            rgb.append(np.array([rgb_of(colour_of(v, *mm), go_past_max) for v in a]))
        total += ns
        differ += int(np.any(rgb[0] != rgb[1], axis=1).sum())
        ends.append(rgb)
    return total, differ, ends



def rmsvel_cases():
    """two plotfiles with different times: velocities with a mean and a fluctuation of comparable size"""
    from stats_ref import stats_hierarchies
    from peleanalysis_amd.hierarchy import MultiFab, field_flame, fill_analytic
    H = stats_hierarchies()["nested"]
    out = []
    for t, seed in ((0.25, 3), (0.75, 5)):
        st = []
        for l, lev in enumerate(H.levels):
            s = MultiFab(lev, 4, 0)
            fill_analytic(s, 0, lambda x, y, z: 1.0 + np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0 * z)
            fill_analytic(s, 1, lambda x, y, z: -0.5 + np.cos(2 * np.pi * (x + t)) * np.sin(2 * np.pi * z) + 0 * y)
            fill_analytic(s, 2, lambda x, y, z: 0.25 * np.sin(4 * np.pi * z) + 0 * x + 0 * y)
            fill_analytic(s, 3, lambda x, y, z: field_flame(x, y, z, 0))
            rng = np.random.default_rng(seed + l)
            for b in range(lev.nboxes):
                s.valid(b)[:3] += 0.1 * rng.uniform(-1, 1, size=s.valid(b)[:3].shape)
            st.append(s)
        out.append((H, st, t))
    return out
