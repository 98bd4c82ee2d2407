"""Plain-Python restatement of the alternate-surface mode of stream.cpp (buildAltSurf; build_surface_at_isoVal :1841-2074,
add_thermal_thickness_to_surf :1554-1838, add_cold_strain_to_surf :1369-1552, add_angle_to_surf :1211-1367, the host post-step
:1041-1084 and write_iso :1166-1209): one scalar loop per line over Python floats (IEEE doubles; math.sqrt is correctly rounded,
math.acos is the C library's).  It shares no code with pa_streamalt.hip.  test_streamalt_ref.py pins it by known answers,
test_gpu_streamalt.py compares the kernel and the stream3d tool with it bit for bit / byte for byte.

A line is column i of a Str array st [ncs][nRKsteps][n]; j = lo .. hi, lo = -nRKh, hi = nRKsteps - 1 - nRKh, nRKh = (nRKsteps - 1) // 2,
point j at index j - lo.  `mistake` plants one deliberate error (test_streamalt_ref.py shows that the case matrix sees each):
"gt_for_ge", "weight_wrong_end", "reversed_sum", "frac_for_1mfrac", "h_round_up"."""
from __future__ import annotations

import math

import numpy as np

MISTAKES = ("gt_for_ge", "weight_wrong_end", "reversed_sum", "frac_for_1mfrac", "h_round_up")
DISTANCE_NAME = "distance_iso_to_alt"


def jrange(nRKsteps: int):
    nRKh = (nRKsteps - 1) // 2
    return -nRKh, nRKsteps - 1 - nRKh


def _div(a: float, b: float) -> float:
    """IEEE division (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def locate(v, lo: int, hi: int, val: float, mistake=None):
    """:1894-1927.  v[j - lo] = the component along the line -> (lIdx, rIdx, frac, branch): branch 0 val at or below v(lo) (nothing
    changes), 1 found, 2 scan exhausted, 3 above v(hi)"""
    V = lambda j: float(v[j - lo])  # noqa: E731
    lIdx, rIdx = lo, lo + 1
    lVal = rVal = V(lo)
    frac = 0.0
    if val > V(hi):
        return hi - 1, hi, 1.0, 3
    if val > lVal:
        found = False
        j = lo
        while j < hi and not found:
            rIdx = lIdx + 1
            rVal = V(rIdx)
            if ((val > lVal) if mistake == "gt_for_ge" else (val >= lVal)) and (val < rVal):
                found = True
            else:
                lIdx, lVal = rIdx, rVal
            j += 1
        frac = 0.0 if rVal == lVal else _div(val - lVal, rVal - lVal)
        return lIdx, rIdx, frac, 1 if found else 2
    return lIdx, rIdx, frac, 0


def lerp(a, lo: int, lIdx: int, rIdx: int, frac: float) -> float:
    xL, xR = float(a[lIdx - lo]), float(a[rIdx - lo])
    return xL + (xR - xL) * frac


def arc(x, lo: int, lIdx: int, rIdx: int, frac: float, mistake=None) -> float:
    """:1944-1972.  x [3][nj] -> the signed distance along the line from j = 0 to the located point"""
    def seg(j):
        dd = 0.0
        for d in range(3):
            xL, xR = float(x[d][j - lo]), float(x[d][j + 1 - lo])
            dd += (xR - xL) * (xR - xL)
        return math.sqrt(dd)
    distance = 0.0
    if lIdx < 0:
        js = list(range(lIdx, 0))
        if mistake == "reversed_sum":
            js.reverse()
        part = (lambda j: j == -1) if mistake == "weight_wrong_end" else (lambda j: j == lIdx)
        for j in js:
            w = (frac if mistake == "frac_for_1mfrac" else (1. - frac)) if part(j) else 1.0
            distance -= w * seg(j)
    else:
        js = list(range(0, rIdx))
        if mistake == "reversed_sum":
            js.reverse()
        part = (lambda j: j == 0) if mistake == "weight_wrong_end" else (lambda j: j == rIdx - 1)
        for j in js:
            distance += (frac if part(j) else 1.0) * seg(j)
    return distance


def cos_to_vertical(x, lo: int, hi: int, mistake=None) -> float:
    """:1247-1265 without the acos: dx[2] / mag around h = (int)(0.5 * (lo + hi))"""
    h = int(0.5 * (lo + hi))  # lo + hi is 0 or 1: truncation = floor
    if mistake == "h_round_up":
        h = int(math.ceil(0.5 * (lo + hi)))
    mag = 0.0
    dx = [0.0] * 3
    for d in range(3):
        dx[d] = float(x[d][h - 1 - lo]) - float(x[d][h + 1 - lo])
        mag += dx[d] * dx[d]
    return _div(dx[2], math.sqrt(mag))


def acos(c: float) -> float:
    try:
        return math.acos(c)
    except ValueError:
        return math.nan


def nout_nquery(carry, thickComp=-1, TComp=-1, addAngle=False):
    return 3 + len(carry) + 1 + (thickComp >= 0) + (TComp >= 0) + bool(addAngle), 1 + 2 * (thickComp >= 0) + (TComp >= 0)


def alt_surface(lines, ins, nRKsteps: int, nNodes: int, isoComp: int, altVal: float, carry=(), thickComp=-1, thickLo=0.0, thickHi=0.0, TComp=-1,
                TVal=0.0, strainComp=-1, addAngle=False, mistake=None):
    """Every line of lines[l][b] ([ncs][nRKsteps][n] or None) with the 1-based node ids ins[l][b] -> (out [nout][nNodes] in the
    order X Y Z, carry, distance, [thickness], [coldStrain], [COSINE of the angle]; branch int8 [nquery][nNodes]; lidx int64
    [nquery][nNodes]).  Nodes without a line keep NaN / -1."""
    lo, hi = jrange(nRKsteps)
    nout, nq = nout_nquery(carry, thickComp, TComp, addAngle)
    out = np.full((nout, nNodes), np.nan)
    branch = np.full((nq, nNodes), -1, dtype=np.int8)
    lidx = np.zeros((nq, nNodes), dtype=np.int64)
    for per_l, per_i in zip(lines, ins):
        for st, ids in zip(per_l, per_i):
            if st is None:
                continue
            for i, nid in enumerate(ids):
                idx = int(nid) - 1
                ln = st[:, :, i]
                x = ln[0:3]
                col, q = [], 0
                lI, rI, fr, code = locate(ln[isoComp], lo, hi, altVal, mistake)
                branch[q, idx], lidx[q, idx] = code, lI
                q += 1
                for d in range(3):
                    col.append(lerp(x[d], lo, lI, rI, fr))
                for c in carry:
                    col.append(lerp(ln[c], lo, lI, rI, fr))
                col.append(arc(x, lo, lI, rI, fr, mistake))
                if thickComp >= 0:
                    locs = []
                    for val in (thickLo, thickHi):
                        a, b, f, code = locate(ln[thickComp], lo, hi, val, mistake)
                        branch[q, idx], lidx[q, idx] = code, a
                        q += 1
                        locs.append(arc(x, lo, a, b, f, mistake))
                    col.append(locs[1] - locs[0])
                if TComp >= 0:
                    a, b, f, code = locate(ln[TComp], lo, hi, TVal, mistake)
                    branch[q, idx], lidx[q, idx] = code, a
                    q += 1
                    col.append(lerp(ln[strainComp], lo, a, b, f))
                if addAngle:
                    col.append(cos_to_vertical(x, lo, hi, mistake))
                out[:, idx] = col
    return out, branch, lidx


def surface_names(str_names, carry, thickComp=-1, TComp=-1, addAngle=False, advect=False):
    names = list(str_names[:3]) + [str_names[c] for c in carry] + [DISTANCE_NAME]
    if thickComp >= 0:
        names.append("thermalThickness" if advect else "thermalThickness_notAdv")
    if TComp >= 0:
        names.append("coldStrain")
    if addAngle:
        names.append("angleWRTvert")
    return names


def post_step(out, names, ncarry: int, addAngle: bool, advect: bool, dt: float = 0.0, iso_dist=None):
    """:1030-1084 on the kernel's array: acos of the cosine column, then either the input surface's distance ADDED to the new one
    and the rename to delta, or X += v * dt (the velocities are the first carried components) -> (out, names)"""
    out = np.array(out, dtype=np.float64)
    names = list(names)
    n = out.shape[1]
    if addAngle:
        for i in range(n):
            out[-1, i] = acos(float(out[-1, i]))
    if not advect:
        dc = 3 + ncarry
        if iso_dist is not None:
            for i in range(n):
                out[dc, i] = float(out[dc, i]) + float(iso_dist[i])
        names[dc] = "delta"
    else:
        for i in range(n):
            for d in range(3):
                out[d, i] = float(out[d, i]) + float(out[3 + d, i]) * dt
    return out, names


def mef_bytes(label: str, names, out, face, nElts: int) -> bytes:
    """write_iso (:1166-1209): label, names, "nElts nodesPerElt", the node FAB component-fastest, the 1-based int32 connectivity"""
    face = np.asarray(face, dtype="<i4")
    n = out.shape[1]
    h = label + "\n" + " ".join(names) + "\n" + "%d %d\n" % (nElts, len(face) // nElts)
    h += "FAB ((8, (64 11 52 0 1 12 0 1023)),(8, (8 7 6 5 4 3 2 1)))((0,0,0) (%d,0,0) (0,0,0)) %d\n" % (n - 1, len(names))
    return h.encode() + np.ascontiguousarray(out.T, dtype="<f8").tobytes() + face.tobytes()
