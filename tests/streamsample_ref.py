"""CPU restatement (numpy) of the reference's Src/sampleStreamlines.cpp with the Fortran of Src/sampleStreamlines_nd.f90: the
streamFile reader (read_ml_streamline_data), find_containing_box, the staged FAB of sample_pathlines (setVal(-20000), FillVar
level by level with piecewise-constant injection, the periodicShift pieces), interpstream / ntrpv, set_distance and both
writers (write_ml_streamline_data, dump_ml_streamline_data).  It is written the reference's way, box by staged box, so it is a
formulation independent of pa_streamsample.hip's per-cell rule.  Not a test module: test_streamsample_ref.py (CPU) and
test_gpu_streamsample.py (GPU, bit for bit) import it.

FillVar's semantics are recalled (AMReX is not part of this repository): every cell takes the value of the finest level <= lev
whose grids hold it, a coarse value injected into every fine cell under it."""
from __future__ import annotations

import itertools
import re

import numpy as np

import streamgrad_ref as G

STAGE_FILL = -20000.0  # sampleStreamlines.cpp:674


class SampleAbort(RuntimeError):
    pass


# ------------------------------------------------------------------------------------------------ Fortran
def _locate(x, dx, plo, blo, bhi):
    """ntrpv up to the sum (sampleStreamlines_nd.f90:67-83), no [plo, phi] test; x [n][3].  ok: b in [blo, bhi - 1]"""
    tmp = (x - plo) / dx - 0.5
    b = np.floor(tmp).astype(np.int64)
    n = (x - ((b + 0.5) * dx + plo)) / dx
    n = np.where(n < 1.0, n, 1.0)
    n = np.where(0.0 < n, n, 0.0)
    ok = np.all((b >= blo) & (b <= bhi - 1), axis=1)
    return ok, b, n


def loop_order(lo, hi):
    """the (i, j, k) points of a box in interpstream's order (:26-53): k, then j = 0 .. lo, then j = 1 .. hi, i innermost"""
    js = list(range(0, lo[1] - 1, -1)) + list(range(1, hi[1] + 1))
    return [(i, j, k) for k in range(lo[2], hi[2] + 1) for j in js for i in range(lo[0], hi[0] + 1)]


def interpstream(loc, loc_lo, fab, fab_lo, dx, plo):
    """loc [nl][nz][ny][nx] on loc_lo..; fab [np][..] on fab_lo...  -> strm [np][nz][ny][nx]; raises SampleAbort with the
    Fortran's message at the first failing point"""
    loc_lo = np.asarray(loc_lo, dtype=np.int64)
    loc_hi = loc_lo + np.array(loc.shape[:0:-1]) - 1
    fab_lo = np.asarray(fab_lo, dtype=np.int64)
    fab_hi = fab_lo + np.array(fab.shape[:0:-1]) - 1
    dx, plo = np.asarray(dx, np.float64), np.asarray(plo, np.float64)
    x = np.stack([loc[d].ravel() for d in range(3)], axis=1)
    ok, b, n = _locate(x, dx, plo, fab_lo, fab_hi)
    if not ok.all():
        okg = ok.reshape(loc.shape[1:])
        for i, j, k in loop_order(loc_lo, loc_hi):
            if not okg[k - loc_lo[2], j - loc_lo[1], i - loc_lo[0]]:
                raise SampleAbort("Seed not in valid region for interp" if j == 0 else "Interp bad, increase nGrow")
    r = b - fab_lo
    out = np.empty((fab.shape[0], x.shape[0]))
    for m in range(fab.shape[0]):
        A = fab[m]
        out[m] = G._sum8(n, lambda di, dj, dk: A[r[:, 2] + dk, r[:, 1] + dj, r[:, 0] + di])
    return out.reshape((fab.shape[0],) + loc.shape[1:])


def set_distance(loc, loc_lo):
    """sampleStreamlines_nd.f90:106-146; loc [>= 3][nz][ny][nx] on loc_lo.. -> res [nz][ny][nx] (res(i,0,0) = 0: k = 0)"""
    lo = np.asarray(loc_lo)
    nz, ny, nx = loc.shape[1:]
    res = np.zeros((nz, ny, nx))
    J = lambda j: j - lo[1]
    for kk in range(nz):
        d = np.zeros(nx)
        res[0 - lo[2], J(0)] = d
        for j in range(-1, lo[1] - 1, -1):
            dxyz = [loc[c, kk, J(j)] - loc[c, kk, J(j + 1)] for c in range(3)]
            d = d + np.sqrt(dxyz[0] * dxyz[0] + dxyz[1] * dxyz[1] + dxyz[2] * dxyz[2])
            res[kk, J(j)] = -d
        d = np.zeros(nx)
        for j in range(1, lo[1] + ny):
            dxyz = [loc[c, kk, J(j)] - loc[c, kk, J(j - 1)] for c in range(3)]
            d = d + np.sqrt(dxyz[0] * dxyz[0] + dxyz[1] * dxyz[1] + dxyz[2] * dxyz[2])
            res[kk, J(j)] = d
    return res


# ------------------------------------------------------------------------------------------------ the streamFile
def read_stream_dir(files):
    """read_ml_streamline_data (:434-501) over {relative path: bytes} -> dict(label, names, nElts, npe, face, ins, levels) with
    levels[l] = [(lo, hi, data [ncomp][nj][ni])] (Str boxes have k = 0 only) and ins[l][b] = the box's inside_nodes ids (empty array when none)"""
    h = files["Header"].decode().split()
    label, nlev, nc = h[0], int(h[1]), int(h[2])
    names = h[3:3 + nc]
    e = [int(v) for v in files["Elements"].decode().split()]
    nElts, npe = e[0], e[1]
    face = np.array(e[2:2 + nElts * npe], dtype=np.int32)
    p = 2 + nElts * npe
    levels = []
    for l in range(nlev):
        hdr = files["Level_%d/Str_H" % l].decode()
        dat = files["Level_%d/Str_D_00000" % l]
        lines = hdr.split("\n")
        ncomp, nb = int(lines[2]), int(lines[4][1:].split()[0])
        boxes = [tuple(int(v) for v in re.findall(r"-?\d+", lines[5 + q])[:6]) for q in range(nb)]
        offs = [int(lines[7 + nb + q].split()[2]) for q in range(nb)]
        fabs = []
        for bx, o in zip(boxes, offs):
            nl = dat.index(b"\n", o) + 1
            lo, hi = bx[:3], bx[3:]
            sh = (ncomp, hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
            a = np.frombuffer(dat, dtype="<f8", count=int(np.prod(sh)), offset=nl).reshape(sh)
            fabs.append((lo, hi, a[:, 0]))
        levels.append(fabs)
    ins = []
    for l in range(nlev):
        per = [np.zeros(0, np.int32) for _ in levels[l]]
        nz = e[p]
        p += 1
        for _ in range(nz):
            bid, n = e[p], e[p + 1]
            per[bid] = np.array(e[p + 2:p + 2 + n], dtype=np.int32)
            p += 2 + n
        ins.append(per)
    return dict(label=label, names=names, nElts=nElts, npe=npe, face=face, ins=ins, levels=levels)


def find_containing_box(xyz, dx, plo):
    """:503-536 over the seeds (i, 0) of a box: int() truncates toward zero.  xyz [3][..]: the seeds' coordinates"""
    lo, hi = [], []
    for d in range(3):
        s = xyz[d]
        lo.append(int(np.trunc((s.min() - plo[d]) / dx[d])))
        hi.append(int(np.trunc((s.max() - plo[d]) / dx[d])))
    return np.array(lo), np.array(hi)


# ------------------------------------------------------------------------------------------------ staged FABs
def _coarsen(a, r):
    return np.floor_divide(a, r)


def fill_var(levels, data, lev, lo, hi, K):
    """AmrData::FillVar onto the box lo..hi of level lev (inside its domain), recalled semantics: coarse to fine, every level
    <= lev writes the cells its grids hold, a coarse value injected into every fine cell under it.  data[l] = MultiFab (K
    components, valid cells).  -> [K][nz][ny][nx], STAGE_FILL where no level holds a cell"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    k, j, i = np.meshgrid(*[np.arange(lo[d], hi[d] + 1) for d in (2, 1, 0)], indexing="ij")
    out = np.full((K,) + i.shape, STAGE_FILL)
    for L in range(lev + 1):
        r = 1
        for q in range(L + 1, lev + 1):
            r *= G.ratio_of(levels[q], levels[q - 1])
        qi, qj, qk = _coarsen(i, r), _coarsen(j, r), _coarsen(k, r)
        lv = levels[L]
        for b in range(lv.nboxes):
            B = lv.boxes[b]
            m = (qi >= B[0]) & (qi <= B[3]) & (qj >= B[1]) & (qj <= B[4]) & (qk >= B[2]) & (qk <= B[5])
            if not m.any():
                continue
            v = data[L].valid(b)
            out[:, m] = v[:K, qk[m] - B[2], qj[m] - B[1], qi[m] - B[0]]
    return out


def _isect(alo, ahi, blo, bhi):
    lo, hi = np.maximum(alo, blo), np.minimum(ahi, bhi)
    return (lo, hi) if np.all(lo <= hi) else None


def staged_level(levels, data, lev, dba, is_per, K):
    """sample_pathlines :671-734 for the grown seed boxes dba of level lev -> [(lo, hi, fab [K][..])]"""
    lv = levels[lev]
    pdlo, pdhi = lv.domlo, lv.domhi
    plen = pdhi - pdlo + 1
    staged = []
    for lo, hi in dba:
        f = np.full((K,) + tuple((hi - lo + 1)[::-1]), STAGE_FILL)
        v = _isect(lo, hi, pdlo, pdhi)  # vba = intersect(dba, ProbDomain[lev]), then FillVar + copy
        if v is not None:
            f[:, v[0][2] - lo[2]:v[1][2] - lo[2] + 1, v[0][1] - lo[1]:v[1][1] - lo[1] + 1, v[0][0] - lo[0]:v[1][0] - lo[0] + 1] = fill_var(levels, data, lev, *v, K)
        staged.append((lo, hi, f))
    if any(is_per):  # Geometry::periodicShift pieces (:695-734), then a MultiFab copy-on-intersection into every staged FAB
        pieces = []
        for lo, hi in dba:
            for s in itertools.product(*[(-1, 0, 1) if is_per[d] else (0,) for d in range(3)]):
                if not any(s):
                    continue
                sh = np.array(s) * plen
                x = _isect(lo + sh, hi + sh, pdlo, pdhi)
                if x is None:
                    continue
                pieces.append((x[0] - sh, x[1] - sh, fill_var(levels, data, lev, x[0], x[1], K)))
        for lo, hi, f in staged:
            for plo_, phi_, a in pieces:
                x = _isect(lo, hi, plo_, phi_)
                if x is None:
                    continue
                a0, a1 = x[0] - plo_, x[1] - plo_
                f0, f1 = x[0] - lo, x[1] - lo
                f[:, f0[2]:f1[2] + 1, f0[1]:f1[1] + 1, f0[0]:f1[0] + 1] = a[:, a0[2]:a1[2] + 1, a0[1]:a1[1] + 1, a0[0]:a1[0] + 1]
    return staged


# ------------------------------------------------------------------------------------------------ the tool
def seed_boxes(path_levels, ins, file_dx, plo, nGrow):
    """per level, per Str box with lines: the grown seed box (lo, hi) of find_containing_box; None for boxes without lines"""
    out = []
    for l, fabs in enumerate(path_levels):
        per = []
        for (lo, hi, a), ids in zip(fabs, ins[l]):
            if len(ids) == 0:
                per.append(None)
                continue
            seeds = a[:3, 0 - lo[1]:1 - lo[1], :]
            blo, bhi = find_containing_box(seeds, file_dx[l], plo)
            per.append((blo - nGrow, bhi + nGrow))
        out.append(per)
    return out


def run_tool(levels, data, path, file_dx, plo, *, is_per=(1, 1, 1), nGrow=4):
    """sampleStreamlines.cpp main after the plotfile is read: data[l] = MultiFab of the K sampled components (valid cells);
    path = read_stream_dir(...).  -> per level per Str box (lo, hi, out [4+K][nj][ni]); raises SampleAbort"""
    K = data[0].ncomp
    nlev = len(levels)
    pl = path["levels"]
    boxes = seed_boxes(pl, path["ins"], file_dx, plo, nGrow)
    res = [[(lo, hi, np.zeros((4 + K,) + np.asarray(a).shape[1:])) for lo, hi, a in pl[l]] for l in range(nlev)]
    for l in range(nlev):
        good = [b for b, bx in enumerate(boxes[l]) if bx is not None]
        if not good:
            continue
        staged = staged_level(levels, data, l, [boxes[l][b] for b in good], is_per, K)
        for b, (slo, shi, f) in zip(good, staged):
            lo, hi, a = pl[l][b]
            res[l][b][2][4:] = interpstream(a[:, None], lo, f, slo, file_dx[l], plo)[:, 0]
    for l in range(nlev):  # set_sample_location (:779-785, fab by fab), set_sample_distance (:761-776)
        for (lo, hi, r), (_, _, a) in zip(res[l], pl[l]):
            r[:3] = a[:3]
            r[3] = set_distance(a[:, None], lo)[0]
    return res


def stream_file_bytes(names, path, res):
    """write_ml_streamline_data (:291-375): Header with the sample's names, Elements as read, Level_<l>/Str (VisMF, one process)"""
    files = G.stream_file_bytes(names, path["face"], path["nElts"], path["ins"], [[None] * len(per) for per in res], 1)
    for l, per in enumerate(res):
        hb, db = G.vismf_bytes([(lo, hi, a) for lo, hi, a in per])
        files["Level_%d/Str_H" % l] = hb
        files["Level_%d/Str_D_00000" % l] = db
    return files


def out_file_bytes(names, res):
    """dump_ml_streamline_data (:377-432), one process: {str_00000_<cnt>: bytes}, one file per non-null box"""
    files, cnt = {}, 0
    for per in res:
        for lo, hi, a in per:
            if tuple(lo) == (0, 0, 0) and tuple(hi) == (0, 0, 0):
                continue
            s = ["".join(n + " " for n in names) + "\n"]
            for j in range(a.shape[1]):
                for i in range(a.shape[2]):
                    s.append("".join("%g " % v for v in a[:, j, i]) + "\n")
            files["str_00000_%05d" % cnt] = "".join(s).encode()
            cnt += 1
    return files
