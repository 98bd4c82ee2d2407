"""An independent numpy reference of the grad -> curvature path on DENSE arrays: the coarse-fine half of pa_apply_bc (the wall half is
ghost_ref.apply_bc's), pa_grad_run, the core of pa_curvature_run / pa_gradcurv_run (Progress, FlameNormal, MeanCurvature, the
threshold clip) and the options of pa_curvature_run (GaussianCurvature, StrainRate, the nine ROST components, VelFlameNormal:
Ref.options).  Restated from the header's contract (include/peleanalysis_amd.h, "ghost cells", "level-batched kernels", pa_curv_params
and the comment of pa_curvature_run), DESIGN.md section 1, the quirk list (Q1-Q3, Q12) and grad.cpp:158-236 /
curvature.cpp:137-160, 283-326, 408-570, 575-789 -- not from pa_curvopts.hip or oracle/.  No box is ever intersected with another one: per level an
occupancy array over the level's domain (1.0 on valid cells, NaN elsewhere; deep levels on a window, ghost_ref._window) answers "is this
position covered" by one lookup at the wrapped position, and every field is such a dense array as well.  Imports neither the oracle nor
the library.  Properly nested hierarchies only: a coarse value that is missing is counted, and the pipelines assert that none is.

Every value is computed in np.longdouble and carries a FIRST-ORDER bound e of the error of a float64 evaluation of the documented
operation order, so that the comparison is  |got - ref| <= 2 e  per cell (the factor 2 stands for the second-order terms).

The bound.  u = 2^-53 + u_ref, u_ref the unit roundoff of np.longdouble read from np.finfo at run time (2^-64 on x86; the sum stays
valid where long double is 64-bit), gamma_k = k u / (1 - k u).  A linear combination sum a_i v_i of values with bounds e_i, whose
longest path from an input to the result passes k roundings (those of the fp-evaluated weights a_i included), has
    e = gamma_k sum |a_i| |v_i| + sum |a_i| e_i.
Counted roundings k per stage (refinement ratios 2 and 4 only -- asserted --, so that xInt and every node difference is exact):
  tangential Lagrange weight     2   product of at most two exact differences (1), exact denominator, division (1)
  boundary value b              10   weight (2), product (1), then 7 sums: five more tangential terms, the centre value, the cross term
                                     (the cross term's own path is shorter: xi0 xi1 (1), / 4 (0), three sums, product, sum = 6)
  normal coefficient             5   numerator and denominator products of three exact differences (2 + 2), division (1)
  coarse-fine ghost value       17   b (10), coefficient (5), product (1), the last sum (1); an interior cell's path is 5 + 1 + 3 = 9
  wall ghost value               0   a copy or a negation
  centred difference             6   dxinv = 1 / ((hi - lo) / n) (3), the difference (1), the product (1), the sum of the two half
                                     fluxes (1); the factor 1/2 is exact.  sum |a_i||v_i| is taken as dxinv/2 (|c - m| + |p - c|): a
                                     difference's rounding is relative to the difference.  The centre value's own error cancels to first
                                     order (it enters the two half fluxes with opposite signs)
  |g|, |G|                       3   squares (1), two sums (2) give 3u on the sum, the root halves it and adds 1: 2.5 u;
                                     the input part is |delta g|_2 <= sqrt(sum e_d^2), which holds at every order
  normal n_d = G_d / (-|G|)      1   e = e_d / |G| + |G_d| e_|G| / |G|^2 + gamma_1 |n_d|   (<= 2 e_G / |G| + a few u: |G_d| <= |G|)
  curvature K                    8   a centred difference (6) and the two sums of the three of them (2); the factor 1/2 is exact
  Hessian H[d][m] = dG_d/dx_m    6   a centred difference of G_d = the cell-centred gradient of c BEFORE its normalisation, unclipped on every
                                     level (:487-488, :582-613).  Ghost cells of G_d: the level's own values across box faces and periodic
                                     sides, wall copies / negations with the call's bc (the same for the three components), coarse-fine
                                     values (17) from the COARSER LEVEL'S G_d; the bound of G enters as dxinv/2 (e_p + e_m)
  minor a b - c d                2   the two products (1) and their difference (1).  A product a b carries |a| e_b + |b| e_a + gamma_1 |a b|;
                                     the difference's own rounding is relative to the difference and is counted against |a b| + |c d|, the
                                     larger: e = gamma_2 (|a b| + |c d|) + |a| e_b + |b| e_a + |c| e_d + |d| e_c
  quadratic form Q = G^T A G     6   nine products A_ij G_j (1), the sums of three (2), the product with G_i (1), the sum of three (2):
                                     e = gamma_6 sum |A_ij| |G_i| |G_j| + sum (e_A_ij |G_i| |G_j| + |A_ij| (e_G_i |G_j| + |G_i| e_G_j))
  Kg = Q / ((gn gn) (gn gn))     4   gn = max(1e-14, |G|) (quirk Q12: pow(x, 4) is (x x)(x x)): three products and the division, and the
                                     relative bound of |G| four times: e = e_Q / gn^4 + |Kg| (4 e_|G| / |G| + gamma_4).  0 where clipped
  ROST q = 3 d + m = du_d/dx_m   6   a centred difference of u_d: exact inputs; ghost cells as G's, coarse data the coarser level's velocity
  StrainRate                     2   (ROST0 + ROST4) + ROST8 -- quirk Q3: the -nn:grad u of :736-744 is overwritten at :745-747 --:
                                     e = gamma_2 (|R0| + |R4| + |R8|) + e_0 + e_4 + e_8.  Never clipped
  VelFlameNormal                 3   (u0 n0 + u1 n1) + u2 n2 with the CLIPPED normal: products (1), two sums (2):
                                     e = gamma_3 sum |u_d n_d| + sum |u_d| e_n_d.  0 where clipped
G^T A^T G is the same sum as G^T A G: whether the nine lines of :630-638 are read as rows or as columns of the adjugate, or the Hessian's
two indices exchanged (adj(H^T) = adj(H)^T), cannot be seen in Kg -- next to walls and coarse-fine faces, where H is not symmetric, as
little as in the interior (test_gradcurv_ref.py::test_transposed_adjugate_is_no_mistake).  What can is the sign each minor carries.
The progress variable c = (s - pmin) * (1 / (pmax - pmin)) is formed in float64 in exactly that order, so Progress is compared bit for
bit, c enters the later stages without an error of its own, and the threshold clip (c < thr or c > 1 - thr in float64) is decided on
the very bits the kernels see.  Clipped cells hold exact zeros.

Measured (worst over the matrix of tests/gradcurv_cases.py; error / (2 e), and 2 e / L-inf of the reference's component per case):
  oracle (CPU tier, test_gradcurv_ref.py)   apply_bc ghosts  err/bound 0.104  bound/Linf 7.1e-15
                                            grad             err/bound 0.168  bound/Linf 1.5e-12
                                            FlameNormal      err/bound 0.136  bound/Linf 3.2e-12
                                            MeanCurvature    err/bound 0.085  bound/Linf 5.8e-11
                                            (the six cases older than `tall` and `kgwide` alone: 0.164, 0.129, 0.068, as before them)
                                            GaussianCurvature err/bound 0.062  bound/Linf 3.2e-11
                                            StrainRate       err/bound 0.167  bound/Linf 3.6e-13
                                            VelFlameNormal   err/bound 0.097  bound/Linf 2.6e-12
                                            ROST (9)         err/bound 0.192  bound/Linf 1.7e-12
  kernels (GPU tier, MI355X)                apply_bc ghosts  err/bound 0.104  bound/Linf 9.0e-15  (coarse-fine cells alone)
                                            grad             err/bound 0.168  bound/Linf 1.5e-12
                                            FlameNormal      err/bound 0.136  bound/Linf 3.2e-12
                                            MeanCurvature    err/bound 0.085  bound/Linf 5.8e-11
                                            GaussianCurvature err/bound 0.062  bound/Linf 3.2e-11  (paths 0, 1 and 2 alike)
                                            StrainRate       err/bound 0.167  bound/Linf 3.6e-13
                                            VelFlameNormal   err/bound 0.097  bound/Linf 2.6e-12
                                            ROST (9)         err/bound 0.192  bound/Linf 1.7e-12
                                            on every entry point and path: the kernels hold the oracle's bits
(bound / L-inf of every option is largest on `deep`, whose finest level has the smallest cells, but for VelFlameNormal: `wide`.)
Smallest |planted mistake's shift| / bound over the negative controls of test_gradcurv_ref.py: 7.0e+11 (unclipped coarse normals on case
`narrow`); over those of the options 1.3e+12 (coarse-fine ghost cells of G from the coarser level's normalised normal, on `tall`; that
test prints the table with -s)."""
import collections
import dataclasses

import numpy as np

import ghost_ref as GR

LD = np.longdouble
U_REF = LD(np.finfo(LD).eps) / 2
U = LD(2.0) ** -53 + U_REF
K_GHOST, K_DIFF, K_NORM, K_DIV, K_CURV = 17, 6, 3, 1, 8
K_MINOR, K_QUAD, K_QUOT, K_SUM3, K_DOT3 = 2, 6, 4, 2, 3
WHOLE_CELLS = 1 << 19   # a level with at most this many domain cells is held whole (if its coarser level is)
PLANTS = ("cross_off", "cross_on", "onesided2", "nx4", "bpoint_half", "inside_domain", "odd_sign", "unclipped_coarse_n", "k_not_halved", "plus_max",
          "adj_transposed", "adj_unsigned_minors", "kg_pow3", "coarse_G_normalised", "hessian_of_n", "strain_nn", "rost_transposed", "veln_unclipped_n", "vel_wall_even")
COUNT_KEYS = ("st1", "st2", "st3c", "st3o", "cross_on", "cross_off", "nx2", "nx3", "nx4", "clipped")


def gamma(k):
    return k * U / (1 - k * U)


@dataclasses.dataclass
class F:
    """a dense field of one level: value and first-order float64 error bound, NaN where the level has no valid cell"""
    v: np.ndarray
    e: np.ndarray


def _lagrange(x, nodes):
    """weights of the Lagrange interpolant through `nodes` at x (array), in long double"""
    w = []
    for j, xj in enumerate(nodes):
        num, den = np.ones_like(x), LD(1)
        for i, xi in enumerate(nodes):
            if i != j:
                num = num * (x - LD(xi))
                den = den * (LD(xj) - LD(xi))
        w.append(num / den)
    return w


class Ref:
    def __init__(self, levels, ratio=2, plant=None):
        assert plant is None or plant in PLANTS
        assert ratio in (2, 4), "the rounding counts above hold for power-of-two ratios"
        self.levels, self.r, self.plant = levels, int(ratio), plant
        self.counts = collections.Counter({k: 0 for k in COUNT_KEYS})
        self.min_normgrad = np.inf
        self.R, self.B = [], []
        for l, lv in enumerate(levels):
            prev = self.R[-1] if l else None
            n = lv.domhi.astype(np.int64) - lv.domlo + 1
            if prev is None or (prev.whole and int(np.prod(n)) <= WHOLE_CELLS):
                lo, hi, whole, clo = lv.domlo.astype(np.int64), lv.domhi.astype(np.int64), True, None
            else:
                lo, hi, whole, clo = GR._window(lv, 2 * self.r, self.r, prev)
                assert not whole
            shape = tuple(int(v) for v in (hi - lo + 1)[::-1])
            R = GR.LevelRef(lv, lo, shape, whole, {}, {}, {}, clo)
            self.R.append(R)
            R.D[0] = self.paint(l, [1.0] * lv.nboxes, np.float64)
            assert int(np.isfinite(R.D[0]).sum()) == lv.ncells, "boxes of a level overlap"
            self.B.append([GR.box_ref(R, b, 1, [0]) for b in range(lv.nboxes)])

    # ------------------------------------------------------------------ dense arrays
    def paint(self, l, boxvals, dtype=LD):
        R, lv = self.R[l], self.levels[l]
        a = np.full(R.shape, np.nan, dtype=dtype)
        for b in range(lv.nboxes):
            lo, hi = lv.boxes[b, :3] - R.lo, lv.boxes[b, 3:] - R.lo + 1
            a[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = boxvals[b]
        return a

    def valid(self, l, b, a):
        R, lv = self.R[l], self.levels[l]
        lo, hi = lv.boxes[b, :3] - R.lo, lv.boxes[b, 3:] - R.lo + 1
        return a[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]

    def field(self, l, mf, comp) -> F:
        """the valid cells of a host multifab's component: exact inputs"""
        v = self.paint(l, [mf.valid(b)[comp] for b in range(self.levels[l].nboxes)])
        return F(v, np.where(np.isnan(v), LD(np.nan), LD(0)))

    def _index(self, l, p):
        """(index arrays z y x into level l's dense arrays of the cells p = (x, y, z), wrapped; mask: not beyond a wall)"""
        R, lv = self.R[l], self.levels[l]
        inside = np.ones(np.shape(p[0]), dtype=bool)
        idx = []
        for d in range(3):
            lo, hi = int(lv.domlo[d]), int(lv.domhi[d])
            beyond = (p[d] < lo) | (p[d] > hi)
            if not R.whole:
                assert not beyond.any(), "a windowed level stays clear of the domain's faces"
                w = p[d] - R.lo[d]
                assert (w >= 0).all() and (w < R.shape[2 - d]).all(), "position outside the level's window"
            elif lv.is_per[d]:
                w = (p[d] - lo) % (hi - lo + 1)
            else:
                inside &= ~beyond
                w = np.clip(p[d], lo, hi) - lo
            idx.append(w)
        return (idx[2], idx[1], idx[0]), inside

    def uncovered(self, l, p):
        """inside the domain (periodic directions wrap) and no valid cell of level l: what a coarse-fine stencil may step on"""
        ix, inside = self._index(l, p)
        if self.plant == "inside_domain":
            return inside
        return inside & np.isnan(self.R[l].D[0][ix])

    def at(self, l, f: F, p):
        """(value, bound, found) of level l's field at the cells p; a cell beyond a wall or without data: 0, 0, False"""
        ix, inside = self._index(l, p)
        v, e = f.v[ix], f.e[ix]
        ok = inside & ~np.isnan(v)
        return np.where(ok, v, LD(0)), np.where(ok, e, LD(0)), ok

    # ------------------------------------------------------------------ applyBC
    def _cf(self, l, f: F, fc: F, q, d, side, nthick, record):
        """coarse-fine ghost values of the cells q = (x, y, z) (1-D arrays) beyond face (d, side) of a box nthick cells thick along d:
        (value, bound, coarse data missing)"""
        r = self.r
        qc = [np.floor_divide(q[a], r) for a in range(3)]
        tdir = [a for a in range(3) if a != d]
        n = q[0].shape[0]
        val, S, E = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
        miss = np.zeros(n, dtype=bool)

        def shifted(p, moves):
            s = [a.copy() for a in p]
            for a, m in moves:
                s[a] = s[a] + m
            return s

        def add(sel, w, pc):
            nonlocal miss
            v, e, ok = self.at(l - 1, fc, [a[sel] for a in pc])
            val[sel] += w * v
            S[sel] += np.abs(w) * np.abs(v)
            E[sel] += np.abs(w) * e
            miss[sel] |= ~ok

        xis = []
        for td in tdir:
            okm, okp = self.uncovered(l, shifted(q, [(td, -r)])), self.uncovered(l, shifted(q, [(td, r)]))
            lo, hi = np.where(okm, -1, 0), np.where(okp, 1, 0)
            onesided = np.zeros(n, dtype=bool)
            if self.plant != "onesided2":
                em = (lo == -1) & (hi == 0) & self.uncovered(l, shifted(q, [(td, -2 * r)]))
                ep = (hi == 1) & (lo == 0) & self.uncovered(l, shifted(q, [(td, 2 * r)]))
                lo, hi = np.where(em, -2, lo), np.where(ep, 2, hi)
                onesided = em | ep
            xi = LD(-0.5) + ((q[td] - qc[td] * r).astype(LD) + LD(0.5)) / LD(r)
            xis.append(xi)
            for a, b in sorted(set(zip(lo.tolist(), hi.tolist()))):
                sel = np.nonzero((lo == a) & (hi == b))[0]
                nodes = list(range(a, b + 1))
                for m, w in zip(nodes, _lagrange(xi[sel], nodes)):
                    add(sel, w, shifted(qc, [(td, m)]))
            if record:
                npts = hi - lo + 1
                self.counts["st1"] += int((npts == 1).sum())
                self.counts["st2"] += int((npts == 2).sum())
                self.counts["st3c"] += int(((npts == 3) & ~onesided).sum())
                self.counts["st3o"] += int(((npts == 3) & onesided).sum())
        add(np.arange(n), -np.ones(n, LD), qc)
        t0, t1 = tdir
        cross = np.ones(n, dtype=bool)
        for s0 in (-1, 1):
            for s1 in (-1, 1):
                cross &= self.uncovered(l, shifted(q, [(t0, s0 * r), (t1, s1 * r)]))
        if self.plant == "cross_off":
            cross[:] = False
        elif self.plant == "cross_on":
            cross[:] = True
        sel = np.nonzero(cross)[0]
        w = xis[0][sel] * xis[1][sel] / LD(4)
        for s0, s1, sg in ((1, 1, 1), (-1, 1, -1), (-1, -1, 1), (1, -1, -1)):
            add(sel, sg * w, shifted(qc, [(t0, s0), (t1, s1)]))
        if record:
            self.counts["cross_on"] += int(cross.sum())
            self.counts["cross_off"] += int((~cross).sum())
        # the polynomial in the normal direction
        nx = 4 if self.plant == "nx4" else min(nthick + 1, 4)
        if record:
            self.counts[f"nx{min(nthick + 1, 4)}"] += n
        nodes = [LD(-0.5) if self.plant == "bpoint_half" else -LD(r) / 2, LD(0.5), LD(1.5), LD(2.5)][:nx]
        if self.plant == "bpoint_half":  # the evaluation point coincides with the first node
            coef = [LD(1)] + [LD(0)] * (nx - 1)
        else:
            coef = [c[0] for c in _lagrange(np.array([LD(-0.5)]), nodes)]
        s = -1 if side else 1
        gv, gS, gE = coef[0] * val, abs(coef[0]) * S, abs(coef[0]) * E
        for m in range(1, nx):
            v, e, ok = self.at(l, f, shifted(q, [(d, s * m)]))
            v = np.where(ok, v, LD(np.nan))  # only a planted NX reads beyond the box
            gv, gS, gE = gv + coef[m] * v, gS + abs(coef[m]) * np.abs(v), gE + abs(coef[m]) * e
        return gv, gamma(K_GHOST) * gS + gE, miss

    def apply_bc_box(self, l, b, f: F, fc, bc, only_dir=-1, record=False, wall_even=False):
        """the box's FAB with one ghost layer after FillBoundary(1) + applyBC: (value, bound) arrays [nz + 2, ny + 2, nx + 2] -- face ghost
        cells resolved (edge and corner ghosts are not part of the operation) --, mask of the coarse-fine face ghost cells, mask of the wall
        ones, number of coarse-fine ghost cells whose coarse data is missing (all of them when fc is None; those are left NaN)"""
        B, lv = self.B[l][b], self.levels[l]
        ix = np.ix_(*B.widx)
        v, e = f.v[ix].copy(), f.e[ix].copy()
        blo = lv.boxes[b, :3].astype(np.int64)
        nbox = lv.boxes[b, 3:].astype(np.int64) - blo + 1
        zz, yy, xx = np.meshgrid(*[np.arange(blo[a] - 1, blo[a] + nbox[a] + 1) for a in (2, 1, 0)], indexing="ij")
        cfm, wallm = np.zeros(B.cls.shape, dtype=bool), np.zeros(B.cls.shape, dtype=bool)
        nmiss = 0
        for d, side, g, i in GR.bc_faces(B, only_dir):
            k = B.cls[g]
            wall, cf = k == 2, k == 1
            assert bc[d] in (1, 2) or not wall.any(), "a periodic direction has no wall"
            sign = 1 if (bc[d] == 1 or self.plant == "odd_sign" or wall_even) else -1
            nv, ne = np.where(wall, sign * v[i], v[g]), np.where(wall, e[i], e[g])
            wallm[g], cfm[g] = wall, cf
            if cf.any():
                if fc is None:
                    nmiss += int(cf.sum())
                    nv[cf], ne[cf] = LD(np.nan), LD(np.nan)
                else:
                    q = [xx[g][cf], yy[g][cf], zz[g][cf]]
                    cv, ce, miss = self._cf(l, f, fc, q, d, side, int(nbox[d]), record)
                    nv[cf], ne[cf] = cv, ce
                    nmiss += int(miss.sum())
            v[g], e[g] = nv, ne
        return v, e, cfm, wallm, nmiss

    # ------------------------------------------------------------------ stencils on one grown box
    def dxinv(self, l):
        lv = self.levels[l]
        n = (lv.domhi.astype(np.int64) - lv.domlo + 1).astype(LD)
        return LD(1) / ((lv.prob_hi.astype(LD) - lv.prob_lo.astype(LD)) / n)

    @staticmethod
    def _cdiff(v, e, d, dxinv):
        """centred difference along direction d over the valid cells of a 1-grown box: value, sum |a||v|, input part"""
        c = (slice(1, -1),) * 3
        m, p = list(c), list(c)
        m[2 - d], p[2 - d] = slice(0, -2), slice(2, None)
        m, p = tuple(m), tuple(p)
        h = dxinv / 2
        return h * (v[p] - v[m]), h * (np.abs(v[c] - v[m]) + np.abs(v[p] - v[c])), h * (e[p] + e[m])

    # ------------------------------------------------------------------ pipelines
    def grad(self, states, comp, bc):
        """pa_grad_run: per level [gx, gy, gz, |g|] as F"""
        out = []
        fs = [self.field(l, s, comp) for l, s in enumerate(states)]
        for l, lv in enumerate(self.levels):
            dxi = self.dxinv(l)
            per = [[] for _ in range(8)]
            for b in range(lv.nboxes):
                v, e, _, _, nmiss = self.apply_bc_box(l, b, fs[l], fs[l - 1] if l else None, bc, record=True)
                assert nmiss == 0, "not properly nested"
                g, ge = [], []
                for d in range(3):
                    gv, S, E = self._cdiff(v, e, d, dxi[d])
                    g.append(gv)
                    ge.append(gamma(K_DIFF) * S + E)
                mag = np.sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2])
                g.append(mag)
                ge.append(np.sqrt(ge[0] * ge[0] + ge[1] * ge[1] + ge[2] * ge[2]) + gamma(K_NORM) * mag)
                for c in range(4):
                    per[c].append(g[c])
                    per[4 + c].append(ge[c])
            out.append([F(self.paint(l, per[c]), self.paint(l, per[4 + c])) for c in range(4)])
        return out

    def progress(self, states, comp):
        """(pmin, pmax, per level the float64 progress variable as a dense float64 array)"""
        pmin = min(float(s.valid(b)[comp].min()) for s in states for b in range(s.level.nboxes))
        pmax = max(float(s.valid(b)[comp].max()) for s in states for b in range(s.level.nboxes))
        inv = np.float64(1.0) / (np.float64(pmax) - np.float64(pmin))
        cs = [self.paint(l, [(s.valid(b)[comp] - np.float64(pmin)) * inv for b in range(s.level.nboxes)], np.float64) for l, s in enumerate(states)]
        return pmin, pmax, cs

    def curvature(self, states, comp, bc, threshold=None):
        """the core of pa_curvature_run: per level a dict with "c" (float64 dense array: Progress), "n" (three F: FlameNormal), "K" (F:
        MeanCurvature) and "clip" (bool dense array)"""
        pmin, pmax, cs = self.progress(states, comp)
        out = []
        for l, lv in enumerate(self.levels):
            dxi = self.dxinv(l)
            cv = cs[l].astype(LD)
            fc = F(cv, np.where(np.isnan(cv), LD(np.nan), LD(0)))
            pn = [[] for _ in range(6)]
            pg = [[] for _ in range(8)]
            for b in range(lv.nboxes):
                v, e, _, _, nmiss = self.apply_bc_box(l, b, fc, out[l - 1]["cf"] if l else None, bc, record=True)
                assert nmiss == 0, "not properly nested"
                G, Ge = [], []
                for d in range(3):
                    gv, S, E = self._cdiff(v, e, d, dxi[d])
                    G.append(gv)
                    Ge.append(gamma(K_DIFF) * S + E)
                sn = np.sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2])
                sne = np.sqrt(Ge[0] * Ge[0] + Ge[1] * Ge[1] + Ge[2] * Ge[2]) + gamma(K_NORM) * sn
                self.min_normgrad = min(self.min_normgrad, float((sn - 2 * sne).min()))
                for d in range(3):
                    pg[d].append(G[d])
                    pg[3 + d].append(Ge[d])
                pg[6].append(sn)
                pg[7].append(sne)
                ng = np.maximum(LD(1e-14), sn)
                if self.plant != "plus_max":
                    ng = -ng
                for d in range(3):
                    nd = G[d] / ng
                    pn[d].append(nd)
                    pn[3 + d].append(Ge[d] / sn + np.abs(G[d]) * sne / (sn * sn) + gamma(K_DIV) * np.abs(nd))
            nf = [F(self.paint(l, pn[d]), self.paint(l, pn[3 + d])) for d in range(3)]  # before the clip: what the level's own stencils read
            crse_n = None
            if l:
                crse_n = out[l - 1]["n_unclipped" if self.plant == "unclipped_coarse_n" else "n"]
            pk = [[], []]
            for b in range(lv.nboxes):
                S, E, K = LD(0), LD(0), LD(0)
                for d in range(3):
                    v, e, _, _, nmiss = self.apply_bc_box(l, b, nf[d], crse_n[d] if l else None, bc, only_dir=d, record=True)
                    assert nmiss == 0, "not properly nested"
                    kv, Sd, Ed = self._cdiff(v, e, d, dxi[d])
                    K, S, E = K + kv, S + Sd, E + Ed
                half = LD(1) if self.plant == "k_not_halved" else LD(0.5)
                pk[0].append(half * K)
                pk[1].append(LD(0.5) * (gamma(K_CURV) * S + E))
            Kf = F(self.paint(l, pk[0]), self.paint(l, pk[1]))
            clip = np.zeros(cs[l].shape, dtype=bool)
            nout = nf
            if threshold is not None:
                thr = np.float64(threshold)
                with np.errstate(invalid="ignore"):
                    clip = (cs[l] < thr) | (cs[l] > np.float64(1.0) - thr)
                self.counts["clipped"] += int(clip.sum())
                Kf = F(np.where(clip, LD(0), Kf.v), np.where(clip, LD(0), Kf.e))
                nout = [F(np.where(clip, LD(0), f.v), np.where(clip, LD(0), f.e)) for f in nf]
            Gf = [F(self.paint(l, pg[d]), self.paint(l, pg[3 + d])) for d in range(3)]  # unnormalised and unclipped: what the options differentiate
            out.append(dict(c=cs[l], cf=fc, n=nout, n_unclipped=nf, K=Kf, clip=clip, pmin=pmin, pmax=pmax, G=Gf, normG=F(self.paint(l, pg[6]), self.paint(l, pg[7]))))
        return out

    def options(self, states, comp, vel_comp, bc, threshold=None, core=None):
        """the options of pa_curvature_run (curvature.cpp:575-789) on top of the core (`core`: what self.curvature returned for the same
        arguments, or None: computed here): per level a dict with "Kg" (F: GaussianCurvature), "SR" (F: StrainRate), "VN" (F: VelFlameNormal)
        and "ROST" (nine F, q = 3 d + m: d u_d / d x_m)"""
        if core is None:
            core = self.curvature(states, comp, bc, threshold)
        us = [[self.field(l, s, vel_comp + d) for d in range(3)] for l, s in enumerate(states)]
        out = []
        for l, lv in enumerate(self.levels):
            dxi = self.dxinv(l)
            o = core[l]
            G, clip = o["G"], o["clip"]
            # ---- :575-677  H[d][m] = d G_d / d x_m, ghost cells of G_d from the coarser level's G_d, the call's bc for every component
            src = o["n_unclipped"] if self.plant == "hessian_of_n" else G
            crse = None
            if l:
                crse = core[l - 1]["n" if self.plant in ("coarse_G_normalised", "hessian_of_n") else "G"]
            pk = [[], []]
            for b in range(lv.nboxes):
                H = [[None] * 3 for _ in range(3)]
                He = [[None] * 3 for _ in range(3)]
                for d in range(3):
                    v, e, _, _, nmiss = self.apply_bc_box(l, b, src[d], crse[d] if l else None, bc)
                    assert nmiss == 0, "not properly nested"
                    for m in range(3):
                        hv, S, E = self._cdiff(v, e, m, dxi[m])
                        H[d][m], He[d][m] = hv, gamma(K_DIFF) * S + E
                if self.plant == "adj_transposed":
                    H, He = [[H[m][d] for m in range(3)] for d in range(3)], [[He[m][d] for m in range(3)] for d in range(3)]

                def minor(a, b_, c, d_):
                    """H[a] H[b] - H[c] H[d] (index pairs): value and bound"""
                    p, q = H[a[0]][a[1]] * H[b_[0]][b_[1]], H[c[0]][c[1]] * H[d_[0]][d_[1]]
                    ein = (np.abs(H[a[0]][a[1]]) * He[b_[0]][b_[1]] + np.abs(H[b_[0]][b_[1]]) * He[a[0]][a[1]]
                           + np.abs(H[c[0]][c[1]]) * He[d_[0]][d_[1]] + np.abs(H[d_[0]][d_[1]]) * He[c[0]][c[1]])
                    return p - q, gamma(K_MINOR) * (np.abs(p) + np.abs(q)) + ein
                # A[i][j]: component j of the adjugate's row i, in the index order of :630-638
                A = [[minor((1, 1), (2, 2), (2, 1), (1, 2)), minor((0, 2), (2, 1), (2, 2), (0, 1)), minor((0, 1), (1, 2), (1, 1), (0, 2))],
                     [minor((1, 2), (2, 0), (2, 2), (1, 0)), minor((0, 0), (2, 2), (2, 0), (0, 2)), minor((0, 2), (1, 0), (1, 2), (0, 0))],
                     [minor((1, 0), (2, 1), (2, 0), (1, 1)), minor((0, 1), (2, 0), (2, 1), (0, 0)), minor((0, 0), (1, 1), (1, 0), (0, 1))]]
                g = [self.valid(l, b, G[d].v) for d in range(3)]
                ge = [self.valid(l, b, G[d].e) for d in range(3)]
                Q, QS, QE = LD(0), LD(0), LD(0)
                for i in range(3):
                    for j in range(3):
                        a, ae = A[i][j]
                        if self.plant == "adj_unsigned_minors" and (i + j) % 2:
                            a = -a
                        Q = Q + g[i] * (a * g[j])
                        QS = QS + np.abs(a) * np.abs(g[i]) * np.abs(g[j])
                        QE = QE + ae * np.abs(g[i]) * np.abs(g[j]) + np.abs(a) * (ge[i] * np.abs(g[j]) + np.abs(g[i]) * ge[j])
                sn, sne = self.valid(l, b, o["normG"].v), self.valid(l, b, o["normG"].e)
                gn = np.maximum(LD(1e-14), sn)
                den = (gn * gn) * gn if self.plant == "kg_pow3" else (gn * gn) * (gn * gn)
                kg = Q / den
                pk[0].append(kg)
                pk[1].append((gamma(K_QUAD) * QS + QE) / den + np.abs(kg) * (4 * sne / sn + gamma(K_QUOT)))
            Kg = F(np.where(clip, LD(0), self.paint(l, pk[0])), np.where(clip, LD(0), self.paint(l, pk[1])))
            # ---- :679-757  ROST q = 3 d + m = d u_d / d x_m, the velocity's ghost cells from the coarser level's velocity, the same bc
            pr = [[[], []] for _ in range(9)]
            for b in range(lv.nboxes):
                for d in range(3):
                    v, e, _, _, nmiss = self.apply_bc_box(l, b, us[l][d], us[l - 1][d] if l else None, bc, wall_even=self.plant == "vel_wall_even")
                    assert nmiss == 0, "not properly nested"
                    for m in range(3):
                        rv, S, E = self._cdiff(v, e, m, dxi[m])
                        q = 3 * m + d if self.plant == "rost_transposed" else 3 * d + m
                        pr[q][0].append(rv)
                        pr[q][1].append(gamma(K_DIFF) * S + E)
            R = [F(self.paint(l, pr[q][0]), self.paint(l, pr[q][1])) for q in range(9)]
            n = o["n"]
            if self.plant == "strain_nn":  # the first assignment of :736-744, which the second one overwrites (quirk Q3)
                sr = LD(0)
                for d in range(3):
                    for m in range(3):
                        sr = sr - R[3 * d + m].v * n[d].v * n[m].v
                SR = F(sr, R[0].e + R[4].e + R[8].e)
            else:  # not clipped
                SR = F((R[0].v + R[4].v) + R[8].v, gamma(K_SUM3) * (np.abs(R[0].v) + np.abs(R[4].v) + np.abs(R[8].v)) + (R[0].e + R[4].e + R[8].e))
            # ---- :761-789  u . n with the clipped normal, (u0 n0 + u1 n1) + u2 n2; an exact zero where clipped
            if self.plant == "veln_unclipped_n":
                n = o["n_unclipped"]
            u = us[l]
            vn = (u[0].v * n[0].v + u[1].v * n[1].v) + u[2].v * n[2].v
            vne = gamma(K_DOT3) * (np.abs(u[0].v * n[0].v) + np.abs(u[1].v * n[1].v) + np.abs(u[2].v * n[2].v)) + (np.abs(u[0].v) * n[0].e + np.abs(u[1].v) * n[1].e + np.abs(u[2].v) * n[2].e)
            if self.plant != "veln_unclipped_n":
                vn, vne = np.where(clip, LD(0), vn), np.where(clip, LD(0), vne)
            out.append(dict(Kg=Kg, SR=SR, VN=F(vn, vne), ROST=R))
        return out


def apply_bc(levels, l, fine, comp, crse, ccomp, bc, ratio=2, only_dir=-1, plant=None, ref=None):
    """pa_apply_bc on level l of `levels` (host multifabs; crse None: no coarse data): (per box (value, bound, coarse-fine mask, wall mask)
    on the box grown by ONE layer, the number of coarse-fine ghost cells without coarse data, the Ref that holds the branch counts)"""
    ref = ref or Ref(levels, ratio, plant)
    f = ref.field(l, fine, comp)
    fc = ref.field(l - 1, crse, ccomp) if (l and crse is not None) else None
    boxes, nmiss = [], 0
    for b in range(levels[l].nboxes):
        v, e, cfm, wallm, nm = ref.apply_bc_box(l, b, f, fc, bc, only_dir, record=True)
        boxes.append((v, e, cfm, wallm))
        nmiss += nm
    return boxes, nmiss, ref


def ring1(fab, ng):
    """the part of a FAB component [..., nz + 2 ng, ny + 2 ng, nx + 2 ng] that is the box grown by one layer (a view)"""
    s = slice(ng - 1, -(ng - 1)) if ng > 1 else slice(None)
    return fab[..., s, s, s]
