"""CPU restatement of the partStream tracer, written from the reference's text (test infrastructure, not product code):

  prepare_field   partStream.cpp:160-177   nGrow ghost layers: piecewise-constant values of the coarser level (the
                                           plotfile's ratio, :173-174), the level's own data on top (FillBoundary, :177);
                                           ghost cells outside the non-periodic domain (:139) hold 0.0 here, the reference
                                           leaves them unset
  where           InitParticles :83 / SetParticleLocation :139 -> Redistribute -> Where(): the finest level whose
                  BoxArray contains the cell of the position
  trace           SetParticleLocation :86-141 (any live line outside its grid grown by nGrow-1: all are re-assigned),
                  vnrml :143-157, ntrpv :159-206, RK4 :208-260 (the second step cut of :250 compares with plo, as written;
                  the +-1e-10 clamp of :256), ComputeNextLocation :262-306 (line numbers of StreamPC.cpp)

Nothing here is shared with oracle/pa_oracle_stream.c or the kernel: this one works on whole arrays of lines -- every RK
stage is one numpy expression over all lines of a FAB -- and the FABs are cut from one dense array per level.  Inside every
expression the operations come in the order of the reference's text and numpy does not contract a*b+c, so results can be
compared with the other two by bits.

The one case the reference's text leaves to the platform is defined here as in the kernel and the oracle: a position that is
not finite (vnrml of an exactly zero vector gives 0 * inf) lies in no FAB and on no grid -- tested before the conversion to
int, which is what x86 makes of it (INT_MIN fails ntrpv's box test: "bad RK")."""
import numpy as np

from peleanalysis_amd.hierarchy import MultiFab, _occupancy


class BadRK(RuntimeError):
    """the reference's Abort("bad RK") of StreamPC.cpp:297; .line is the 1-based number of the lowest failing line of the step"""

    def __init__(self, line):
        super().__init__(f"bad RK (line {line})")
        self.line = line


def ratios_of(levels):
    return [int(levels[l].domhi[0] - levels[l].domlo[0] + 1) // int(levels[l - 1].domhi[0] - levels[l - 1].domlo[0] + 1) for l in range(1, len(levels))]


def _dense_valid(level, mf, comps):
    """the level's own data on its whole domain [3][nz][ny][nx] (NaN where it has no grid)"""
    n = level.domhi - level.domlo + 1
    D = np.full((3, int(n[2]), int(n[1]), int(n[0])), np.nan)
    for b in range(level.nboxes):
        lo, hi = level.boxes[b, :3] - level.domlo, level.boxes[b, 3:] - level.domlo
        for d, c in enumerate(comps):
            D[d, lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = mf.valid(b)[c]
    return D


def prepare_field(levels, fields, comps, ngrow, ratio=None):
    """partStream.cpp:160-177 -> list of 3-component multifabs with ngrow ghost layers"""
    ratio = ratios_of(levels) if ratio is None else ([int(ratio)] * (len(levels) - 1) if np.ndim(ratio) == 0 else list(ratio))
    out, g = [], int(ngrow)
    for l, lv in enumerate(levels):
        assert not np.any(lv.is_per), "the reference's geometry is not periodic (partStream.cpp:139)"
        own = _dense_valid(lv, fields[l], comps)
        have = _occupancy(lv)
        if l > 0:  # FillPatchTwoLevels with PCInterp (:173-174): the value of the coarse cell that holds the fine cell ...
            r = ratio[l - 1]
            crse = _dense_valid(levels[l - 1], fields[l - 1], comps)
            idx = [np.arange(own.shape[1 + a]) // r for a in range(3)]
            D = crse[:, idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
            D[:, have] = own[:, have]  # ... under the level's own data
        else:
            D = own
        G = np.zeros((3,) + tuple(s + 2 * g for s in D.shape[1:]))  # outside the domain: 0.0
        G[:, g:-g, g:-g, g:-g] = D
        v = MultiFab(lv, 3, g)
        for b in range(lv.nboxes):
            lo, hi = lv.boxes[b, :3] - lv.domlo, lv.boxes[b, 3:] - lv.domlo  # box grown by g, in G's index space: lo .. hi + 2g
            f = G[:, lo[2]:hi[2] + 2 * g + 1, lo[1]:hi[1] + 2 * g + 1, lo[0]:hi[0] + 2 * g + 1]
            if np.isnan(f).any():
                raise ValueError(f"level {l} box {b}: ghost cells inside the domain without coarse data (not properly nested for nGrow = {g})")
            v.fab(b)[:] = f
        out.append(v)
    return out


def _cell(q):
    """floor'ed doubles -> int64; rows that are not finite get a cell no box contains"""
    ok = np.isfinite(q).all(axis=1)
    return np.where(ok[:, None], q, -1.0e9).astype(np.int64), ok


def where(levels, x):
    """Where(): (level, grid) of the finest level whose BoxArray contains the cell of x [n][3]; -1, -1 where none does"""
    n = len(x)
    lev, grd = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    fin = np.isfinite(x).all(axis=1)
    for l in range(len(levels) - 1, -1, -1):
        lv = levels[l]
        with np.errstate(invalid="ignore"):
            p, _ = _cell(np.floor((x - lv.prob_lo[None, :]) / lv.dx[None, :]))
        B = lv.boxes.astype(np.int64)
        inside = np.all((p[:, None, :] >= B[None, :, :3]) & (p[:, None, :] <= B[None, :, 3:]), axis=2) & fin[:, None]
        take = inside.any(axis=1) & (lev < 0)
        lev[take], grd[take] = l, inside.argmax(axis=1)[take]
    return lev, grd


def _vnrml(vec, dirn):
    """:143-157, vec [n][3], dirn [n] (+1 / -1)"""
    s = vec[:, 0] * vec[:, 0] + vec[:, 1] * vec[:, 1] + vec[:, 2] * vec[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        f = dirn * (1.0 / np.sqrt(s))
        return np.where((s < 1.0e12)[:, None], vec * f[:, None], 0.0)


def _ntrpv(x, fab, glo, ng, dx, plo):
    """:159-206 for all lines of one FAB: fab [3][nz][ny][nx] over the grown box whose low corner is glo -> (u [n][3], ok [n])"""
    with np.errstate(invalid="ignore"):
        b, ok = _cell(np.floor((x - plo) / dx - 0.5))
        w = (x - ((b + 0.5) * dx + plo)) / dx
        w = np.where(w < 1.0, w, 1.0)  # std::min(1., n)
        w = np.where(0.0 < w, w, 0.0)  # std::max(0., .)
    ghi = glo + np.array(fab.shape[:0:-1]) - 1
    ok = ok & np.all((b >= glo) & (b <= ghi - 1), axis=1)
    i, j, k = [np.clip(b[:, d] - glo[d], 0, fab.shape[3 - d] - 2) for d in range(3)]
    n0, n1, n2 = w[:, 0], w[:, 1], w[:, 2]
    u = np.empty_like(x)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            g = fab[c]
            u[:, c] = (+n0 * n1 * n2 * g[k + 1, j + 1, i + 1]
                       + n0 * (1 - n1) * n2 * g[k + 1, j, i + 1]
                       + n0 * n1 * (1 - n2) * g[k, j + 1, i + 1]
                       + n0 * (1 - n1) * (1 - n2) * g[k, j, i + 1]
                       + (1 - n0) * n1 * n2 * g[k + 1, j + 1, i]
                       + (1 - n0) * (1 - n1) * n2 * g[k + 1, j, i]
                       + (1 - n0) * n1 * (1 - n2) * g[k, j + 1, i]
                       + (1 - n0) * (1 - n1) * (1 - n2) * g[k, j, i])
    return u, ok


def _rk4(x, dt, fab, glo, ng, dx, plo, phi, dirn):
    """:208-260 -> (new x, ok, scale of the step cut)"""
    ks, xx, ok = [], x, np.ones(len(x), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for stage in range(4):
            vec, o = _ntrpv(xx, fab, glo, ng, dx, plo)
            ok &= o
            k = _vnrml(vec, dirn) * dt
            ks.append(k)
            if stage < 3:
                xx = x + (k * 0.5 if stage < 2 else k)
        third, sixth = 1.0 / 3.0, 1.0 / 6.0
        delta = (ks[0] + ks[3]) * sixth + (ks[1] + ks[2]) * third
        scale = np.ones(len(x))
        for d in range(3):
            s = np.abs((x[:, d] - plo[d]) / delta[:, d])
            scale = np.where((x[:, d] + delta[:, d] < plo[d]) & (s < scale), s, scale)
            s = np.abs((phi[d] - x[:, d]) / delta[:, d])
            scale = np.where((x[:, d] + delta[:, d] > plo[d]) & (s < scale), s, scale)  # :250 compares with plo, as written
        y = x + scale[:, None] * delta
        lo, hi = plo + 1.0e-10, phi - 1.0e-10
        m = np.where(lo[None, :] < y, y, lo[None, :])
        z = np.where(m < hi[None, :], m, hi[None, :])
    return z, ok, scale, np.any(z != y, axis=1)


def trace(levels, vfield, seeds, nsteps, dt, vcomp=0, info=None):
    """-> (pos [2 nseed][nsteps][3], number of redistributions); raises BadRK.  Line 2s runs forward from seed s, 2s+1 backward
    (InitParticles :54-81).  info (a dict): filled with the number of line steps that were cut (scale < 1) and clamped"""
    seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
    npl, ng = 2 * len(seeds), vfield[0].ng
    pos = np.zeros((npl, nsteps, 3))
    pos[:, 0, :] = np.repeat(seeds, 2, axis=0)
    dirn = np.where(np.arange(npl) % 2 == 0, 1.0, -1.0)
    lev, grd = where(levels, pos[:, 0, :])
    nred = ncut = nclamp = 0
    for step in range(nsteps - 1):
        x = pos[:, step, :]
        live = lev >= 0
        # SetParticleLocation: the grid grown by nGrow - 1, in physical coordinates (:106-115)
        leave = False
        for l, lv in enumerate(levels):
            q = np.nonzero(lev == l)[0]
            if len(q) == 0:
                continue
            B = lv.boxes[grd[q]].astype(np.int64)
            blo = lv.prob_lo[None, :] + (B[:, :3] - (ng - 1)) * lv.dx[None, :]
            bhi = lv.prob_lo[None, :] + (B[:, 3:] + (ng - 1) + 1) * lv.dx[None, :]
            leave = leave or bool(np.any((x[q] < blo) | (x[q] > bhi)))
        if leave:
            nred += 1
            nl, ngd = where(levels, x[live])
            lev[live], grd[live] = nl, ngd
        new = x.copy()
        bad = np.zeros(npl, dtype=bool)
        for l, lv in enumerate(levels):
            for b in np.unique(grd[lev == l]):
                q = np.nonzero((lev == l) & (grd == b))[0]
                fab = vfield[l].fab(int(b))[vcomp:vcomp + 3]
                y, ok, scale, clamped = _rk4(x[q], dt, fab, lv.boxes[b, :3].astype(np.int64) - ng, ng, lv.dx, lv.prob_lo, lv.prob_hi, dirn[q])
                new[q] = y
                bad[q] = ~ok
                ncut += int(np.sum(ok & (scale < 1.0)))
                nclamp += int(np.sum(ok & clamped))
        if bad.any():
            raise BadRK(int(np.argmax(bad)) + 1)
        pos[:, step + 1, :] = new
    if info is not None:
        info.update(ncut=ncut, nclamp=nclamp)
    return pos, nred
