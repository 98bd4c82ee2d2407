// pa_fused_prep.hip -- fused grad -> curvature, stage 1 of 3: ghost preparation of the exact-normal pipeline (gfx950).
//
// Before the sweeps, for every special face (a box face with ghost cells that are not valid cells of the level): the coarse
// patches behind coarse-fine faces (k_cpatch*), the face ghosts of phi and the resolved ghost values of the progress variable in
// the level's compact face-major arrays (k_prep_faces_chunks), and the edge ghosts in their rings (k_find_ring once per level,
// k_prep_ring per pass).  The CG sweeps (pa_fused_sweep.hip) and the one-layer fix-up (pa_fused_fix.hip) read those arrays.
// Used by the exact-normal pipeline only (the first fused pipeline resolves a stored shell of c instead: pa_core.hip) and, with
// PHIONLY, as the applyBC of pa_grad_run and of pa_curvature_run's options.
// Entry points: pa_gradcurv_prep_levels (pa_internal.h); pa_level_cg, pa_cpatch_launch (pa_fused.h).
#include "pa_fused.h"
#include "pa_dist.h"
#include "pa_fabview.h"
#include <cstdlib>

// The sweep with CG (pa_fused_march3.h) takes the progress variable behind special faces from the level's compact
// face-major arrays, so N is final after the sweep and only the curvature of the FIRST layer behind a special face is
// left (its ghost normal is MLMG applyBC on n_d, curvature.cpp:510-531).  Per level: k_prep_faces (+ k_prep_ring) before
// the sweep, k_faces_curv_fast<1> + k_faces_curv<true> after it -- against progress shell + two applyBC launches before
// and three fix-up launches over two layers after it in the first pipeline (kept for the threshold clip, mixed faces and
// narrow boxes).
struct PrepArgs {
  int bc[3];
  int ratio, has_crse;
  double pmin, invd;
};

// Thread per ghost cell of a special face: the face ghost of phi (MLMG applyBC, as k_apply_bc_sfaces) and the resolved
// ghost value of c = the same boundary condition applied to c, whose interior values are (phi - pmin) * invd formed on the
// fly and whose coarse values are the affine view of the coarse phi -- the operations of k_apply_bc_sfaces<2> on a stored c.
struct PrepLev { DLevelView L; DMFView M; int comp; DLevelView LC; DMFView MC; int ccomp; PrepArgs A; int use_cp; long long cg_stride = 0, cp_stride = 0; const int2* wg = nullptr; int nwg = 0; const int* sfboxes = nullptr; };
// PHIONLY (the gradient tool's pass): only the face ghost of phi -- MLMG applyBC as k_apply_bc_sfaces does it, but on the per-face
// work tables and from the coarse PATCHES instead of owner-map lookups into the coarse FABs (the three applyBC launches of a
// 3-level hierarchy took 0.43 ms, this kernel 0.19 ms with the progress variable on top)
template <bool PATCH, bool PHIONLY>
__device__ __forceinline__ void prep_faces_cell(const PrepLev& Pl, int* nbad, const SlotK& sk, unsigned fy, long long t) {
  const DLevelView& L = Pl.L;
  const DMFView& M = Pl.M;
  const DLevelView& LC = Pl.LC;
  const int z = (int)blockIdx.z;  // component slot
  DMFView MC = Pl.MC;
  PrepArgs A = Pl.A;
  if (sk.prog) { A.pmin = MC.xa = sk.prog[2 * z]; A.invd = MC.xb = sk.prog[2 * z + 1]; }
  const int comp = Pl.comp + z, ccomp = Pl.ccomp + z;
  double* const cgz = L.cg + z * Pl.cg_stride;
  const double* const cpz = L.cp ? L.cp + z * Pl.cp_stride : nullptr;
  int b, dir, side, layer, q[3];
  DBox B;
  if (!sface_decode(L, fy, t, 1, b, B, dir, side, q, layer)) return;
  const unsigned code = L.sfcode[L.sfoff[fy] + t];
  const int cls = (int)(code & 3u);
  const int t0 = (dir == 0) ? 1 : 0, t1 = (dir == 2) ? 1 : 2;
  double* cgp = PHIONLY ? nullptr : cgz + L.cgoff[fy] + (long long)(q[t1] - B.lo[t1] + 1) * (B.hi[t0] - B.lo[t0] + 3) + (q[t0] - B.lo[t0] + 1);
  double* p = M.data + M.off[b];
  if (PHIONLY && cls == 0) return;  // a valid cell of the level: FillBoundary's
  if (cls == 0) {
    // a valid cell of the level (a face that is partly coarse-fine, partly covered by a neighbouring box): the progress variable
    // of the cell itself.  Read in the box that OWNS the cell when that box is local -- this kernel runs next to the local
    // FillBoundary, which is what fills the ghost cell -- and in the ghost cell when the owner is another rank's box (the
    // cross-rank exchange has completed on this stream before this launch)
    int sb, xw[3];
    double v;
    if (classify(L, q[0], q[1], q[2], sb, xw) == 0 && sb >= 0) v = M.data[M.off[sb] + fab_index(L.boxes[sb], M.ng, M.ncomp, comp, xw[0], xw[1], xw[2])];
    else v = p[fab_index(B, M.ng, M.ncomp, comp, q[0], q[1], q[2])];
    *cgp = (v - A.pmin) * A.invd;
    return;
  }
  const int s = side ? -1 : 1;
  if (cls == 2) {
    int in[3] = {q[0], q[1], q[2]};
    in[dir] += s;
    const double v = p[fab_index(B, M.ng, M.ncomp, comp, in[0], in[1], in[2])];
    const double vc = (v - A.pmin) * A.invd;
    const bool odd = A.bc[dir] == PA_BC_REFLECT_ODD;
    p[fab_index(B, M.ng, M.ncomp, comp, q[0], q[1], q[2])] = odd ? -v : v;
    if (!PHIONLY) *cgp = odd ? -vc : vc;
    return;
  }
  if (!A.has_crse) { atomicAdd(nbad, 1); return; }
  bool ok = true;
  double coef[4], bv[2];
  const int NX = cf_normal_coef(B.hi[dir] - B.lo[dir] + 1, A.ratio, coef);
  const int xf[2] = {0, 1};
  const long long cpo = (Pl.use_cp && L.cp) ? L.cpoff[fy] : -1;  // wave-uniform
  if (PATCH || cpo >= 0) cf_interp_patch<2>(code, cpz + cpo, B, side, MC, q, dir, xf, ok, bv);
  else cf_interp<2>(code, LC, MC, ccomp, q, dir, A.ratio, xf, ok, bv);
  if (!ok) atomicAdd(nbad, 1);
  double tp = 0.0, tc = 0.0;
  for (int m = 1; m < NX; ++m) {
    int pc[3] = {q[0], q[1], q[2]};
    pc[dir] += s * m;
    const double v = p[fab_index(B, M.ng, M.ncomp, comp, pc[0], pc[1], pc[2])];
    tp += v * coef[m];
    tc += ((v - A.pmin) * A.invd) * coef[m];
  }
  double gp = tp, gc = tc;
  gp += bv[0] * coef[0];
  gc += bv[1] * coef[0];
  p[fab_index(B, M.ng, M.ncomp, comp, q[0], q[1], q[2])] = gp;
  if (!PHIONLY) *cgp = gc;
}

// ---- round 6: the same work from the levels' CHUNK RECORDS (SfChunk, pa_internal.h).  A workgroup takes one record = a rectangle of
// 1024 ghost cells of one face, a thread the 2 x 2 block of ghost cells that share ONE coarse parent.  Chunks of one kind run
// straight-line code: no per-cell code, no code-dependent trip counts, the interpolation weights as literals -- so the 21 loads of
// a thread's four cells (9 coarse values of the parent's 3 x 3 neighbourhood, loaded once instead of four times, + 3 interior cells
// each) are issued together.  Before: one thread per cell behind the chain work table -> sfaces -> boxes -> offsets -> code ->
// weights + patch -> data (a wave lived 13 us, 3/4 of it waiting).  Per cell the operations and their order are those of
// prep_faces_cell / cf_interp_core with code PA_CODE_FULL, so the same bits; mixed chunks take prep_faces_cell itself.
template <int dir, bool PHIONLY>
__device__ __forceinline__ void prep_chunk_uniform(const PrepLev& Pl, const SfChunk& D, const PrepArgs& A, double xa, double xb, int comp, double* cgz, const double* cpz, int* nbad) {
  const int side = D.dir_side & 1;
  constexpr int t0 = dir == 0 ? 1 : 0, t1 = dir == 2 ? 1 : 2;
  const DMFView& M = Pl.M;
  const int n0 = D.hi[t0] - D.lo[t0] + 1, n1 = D.hi[t1] - D.lo[t1] + 1;
  const int hw = D.cw >> 1, sh = 31 - __builtin_clz((unsigned)hw);
  const int u = D.u0 + 2 * ((int)threadIdx.x & (hw - 1)), v = D.v0 + 2 * ((int)threadIdx.x >> sh);
  if (u >= n0 || v >= n1) return;  // (even extents: a block is inside the face or outside it)
  const int ng = M.ng;
  const long long nxg = D.hi[0] - D.lo[0] + 1 + 2 * ng, nyg = D.hi[1] - D.lo[1] + 1 + 2 * ng, nzg = D.hi[2] - D.lo[2] + 1 + 2 * ng;
  double* const p = M.data + M.off[D.box] + (long long)comp * pa_cstride(nxg * nyg * nzg, M.ncomp);
  const long long st[3] = {1, nxg, nxg * nyg};
  int q[3];
  q[dir] = side ? D.hi[dir] + 1 : D.lo[dir] - 1;
  q[t0] = D.lo[t0] + u;
  q[t1] = D.lo[t1] + v;
  const long long iq = ((long long)(q[2] - D.lo[2] + ng) * nyg + (q[1] - D.lo[1] + ng)) * nxg + (q[0] - D.lo[0] + ng);
  const long long sn = side ? -st[dir] : st[dir], s0 = st[t0], s1 = st[t1];
  double* const cgp = PHIONLY ? nullptr : cgz + D.cgoff + (long long)(v + 1) * (n0 + 2) + (u + 1);
  const bool odd = A.bc[dir] == PA_BC_REFLECT_ODD;
  if (D.flags & PA_SFC_WALL) {
    double w[2][2];
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int du = 0; du < 2; ++du) w[dv][du] = p[iq + dv * s1 + du * s0 + sn];
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int du = 0; du < 2; ++du) {
        const double x = w[dv][du], xc = (x - A.pmin) * A.invd;
        p[iq + dv * s1 + du * s0] = odd ? -x : x;
        if (!PHIONLY) cgp[dv * (n0 + 2) + du] = odd ? -xc : xc;
      }
    return;
  }
  // PA_SFC_FULL: the coarse parent of the block and its 3 x 3 neighbourhood in the face's coarse patch
  DBox B;
#pragma unroll
  for (int d = 0; d < 3; ++d) { B.lo[d] = D.lo[d]; B.hi[d] = D.hi[d]; }
  int plane, pu0, pv0, pw, ph;
  cpatch_geom(B, dir, side, plane, pu0, pv0, pw, ph);
  const double* const cb = cpz + D.cpoff + (long long)((q[t1] >> 1) - pv0) * pw + ((q[t0] >> 1) - pu0);
  double r[3][3];  // r[a1 + 1][a0 + 1] = coarse(qc + a0 e_t0 + a1 e_t1)
#pragma unroll
  for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
    for (int a0 = 0; a0 < 3; ++a0) r[a1][a0] = cb[(a1 - 1) * pw + (a0 - 1)];
  double f[2][2][3];  // the three cells behind the face of every ghost cell of the block
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du)
#pragma unroll
      for (int m = 0; m < 3; ++m) f[dv][du][m] = p[iq + dv * s1 + du * s0 + (m + 1) * sn];
  bool ok = true;
#pragma unroll
  for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
    for (int a0 = 0; a0 < 3; ++a0)
      if (__double_as_longlong(r[a1][a0]) == PA_CP_MISSING) { ok = false; r[a1][a0] = 0.0; }
  if (!ok) atomicAdd(nbad, 4);  // counted per ghost cell: the four cells of the block use all nine values
  double rc[3][3];  // the progress variable as the affine view of the coarse phi
#pragma unroll
  for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
    for (int a0 = 0; a0 < 3; ++a0) rc[a1][a0] = (r[a1][a0] - xa) * xb;
  constexpr double nc0 = k_cf_coef.nrm[4][0], nc1 = k_cf_coef.nrm[4][1], nc2 = k_cf_coef.nrm[4][2], nc3 = k_cf_coef.nrm[4][3];
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du) {
      // InterpBndryData, cf_interp_core with lo = -1, hi = 1 in both directions and the cross term, child (du, dv) of the parent
      const double c00 = du ? k_cf_coef.tan[1][1][1][0] : k_cf_coef.tan[0][1][1][0], c01 = du ? k_cf_coef.tan[1][1][1][1] : k_cf_coef.tan[0][1][1][1],
                   c02 = du ? k_cf_coef.tan[1][1][1][2] : k_cf_coef.tan[0][1][1][2];
      const double c10 = dv ? k_cf_coef.tan[1][1][1][0] : k_cf_coef.tan[0][1][1][0], c11 = dv ? k_cf_coef.tan[1][1][1][1] : k_cf_coef.tan[0][1][1][1],
                   c12 = dv ? k_cf_coef.tan[1][1][1][2] : k_cf_coef.tan[0][1][1][2];
      const double xi0 = du ? 0.25 : -0.25, xi1 = dv ? 0.25 : -0.25;
      double b0 = 0.0, b1 = 0.0;
      b0 += c00 * r[1][0];  b1 += c00 * rc[1][0];
      b0 += c01 * r[1][1];  b1 += c01 * rc[1][1];
      b0 += c02 * r[1][2];  b1 += c02 * rc[1][2];
      b0 += c10 * r[0][1];  b1 += c10 * rc[0][1];
      b0 += c11 * r[1][1];  b1 += c11 * rc[1][1];
      b0 += c12 * r[2][1];  b1 += c12 * rc[2][1];
      b0 -= r[1][1];        b1 -= rc[1][1];
      b0 += ((xi0 * xi1) * 0.25) * (((r[2][2] - r[2][0]) + r[0][0]) - r[0][2]);
      b1 += ((xi0 * xi1) * 0.25) * (((rc[2][2] - rc[2][0]) + rc[0][0]) - rc[0][2]);
      // MLMG applyBC across the face: points {-1 (the interpolated value), 0.5, 1.5, 2.5} seen from -0.5
      double tp = 0.0, tc = 0.0;
      tp += f[dv][du][0] * nc1;  tc += ((f[dv][du][0] - A.pmin) * A.invd) * nc1;
      tp += f[dv][du][1] * nc2;  tc += ((f[dv][du][1] - A.pmin) * A.invd) * nc2;
      tp += f[dv][du][2] * nc3;  tc += ((f[dv][du][2] - A.pmin) * A.invd) * nc3;
      double gp = tp, gc = tc;
      gp += b0 * nc0;
      gc += b1 * nc0;
      p[iq + dv * s1 + du * s0] = gp;
      if (!PHIONLY) cgp[dv * (n0 + 2) + du] = gc;
    }
}


// Any mix of cell kinds in the chunk (coarse-fine with any stencil, wall, valid cells of the level behind a partly covered face),
// block origins on even GLOBAL indices (u0 / v0 may be -1: cells outside the face are predicated off).  Everything a block may need
// is requested up front -- four codes, the 13 coarse values, three interior cells per ghost cell -- then each cell's value is chosen
// by selects; only a valid ghost cell (its value lives in the box that owns it: an owner-map lookup) takes a branch.
template <int dir, bool PHIONLY>
__device__ __forceinline__ void prep_chunk_mixed(const PrepLev& Pl, const SfChunk& D, const PrepArgs& A, double xa, double xb, int comp, double* cgz, const double* cpz,
                                                 int* nbad, const double* tabs) {
  const int side = D.dir_side & 1;
  constexpr int t0 = dir == 0 ? 1 : 0, t1 = dir == 2 ? 1 : 2;
  const DMFView& M = Pl.M;
  const DLevelView& L = Pl.L;
  const int n0 = D.hi[t0] - D.lo[t0] + 1, n1 = D.hi[t1] - D.lo[t1] + 1;
  const int hw = D.cw >> 1, sh = 31 - __builtin_clz((unsigned)hw);
  const int u = D.u0 + 2 * ((int)threadIdx.x & (hw - 1)), v = D.v0 + 2 * ((int)threadIdx.x >> sh);
  if (u >= n0 || v >= n1) return;
  const int ng = M.ng;
  const long long nxg = D.hi[0] - D.lo[0] + 1 + 2 * ng, nyg = D.hi[1] - D.lo[1] + 1 + 2 * ng, nzg = D.hi[2] - D.lo[2] + 1 + 2 * ng;
  double* const p = M.data + M.off[D.box] + (long long)comp * pa_cstride(nxg * nyg * nzg, M.ncomp);
  const long long st[3] = {1, nxg, nxg * nyg};
  int q[3];
  q[dir] = side ? D.hi[dir] + 1 : D.lo[dir] - 1;
  q[t0] = D.lo[t0] + u;
  q[t1] = D.lo[t1] + v;
  const long long iq = ((long long)(q[2] - D.lo[2] + ng) * nyg + (q[1] - D.lo[1] + ng)) * nxg + (q[0] - D.lo[0] + ng);
  const long long sn = side ? -st[dir] : st[dir], s0 = st[t0], s1 = st[t1];
  double* const cgp = PHIONLY ? nullptr : cgz + D.cgoff + (long long)(v + 1) * (n0 + 2) + (u + 1);
  const bool odd = A.bc[dir] == PA_BC_REFLECT_ODD;
  bool in[2][2];
  long long off[2][2];
  unsigned code[2][2];
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du) {
      const int uu = u + du, vv = v + dv;
      in[dv][du] = uu >= 0 && uu < n0 && vv >= 0 && vv < n1;
      const int uc = min(max(uu, 0), n0 - 1), vc = min(max(vv, 0), n1 - 1);
      off[dv][du] = (long long)(vc - v) * s1 + (long long)(uc - u) * s0;
      code[dv][du] = L.sfcode[D.sfoff + (long long)vc * n0 + uc];
    }
  const bool cf_here = (D.flags & PA_SFC_HAS_CF) != 0;  // (uniform) a chunk without coarse-fine cells may belong to a face without a patch
  CfBlock K;
  if (cf_here) {
    DBox B;
#pragma unroll
    for (int d = 0; d < 3; ++d) { B.lo[d] = D.lo[d]; B.hi[d] = D.hi[d]; }
    int plane, pu0, pv0, pw, ph;
    cpatch_geom(B, dir, side, plane, pu0, pv0, pw, ph);
    cf_block_load(cpz + D.cpoff + (long long)((q[t1] >> 1) - pv0) * pw + ((q[t0] >> 1) - pu0), pw, K);
  }
  double f[2][2][3];
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du)
#pragma unroll
      for (int m = 0; m < 3; ++m) f[dv][du][m] = p[iq + off[dv][du] + (m + 1) * sn];
  if (cf_here) cf_block_finish(K);
  constexpr double nc0 = k_cf_coef.nrm[4][0], nc1 = k_cf_coef.nrm[4][1], nc2 = k_cf_coef.nrm[4][2], nc3 = k_cf_coef.nrm[4][3];
  int nbad_here = 0;
  bool any_valid = false;
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du) {
      const unsigned cd = in[dv][du] ? code[dv][du] : 0u;
      const int cls = (int)(cd & 3u);
      any_valid = any_valid || (in[dv][du] && cls == 0);
      double gp, gc;
      {  // wall: the mirror image of the first cell
        const double x = f[dv][du][0], xc = (x - A.pmin) * A.invd;
        gp = odd ? -x : x;
        gc = odd ? -xc : xc;
      }
      if (cf_here) {  // coarse-fine: InterpBndryData + MLMG applyBC across the face (both formed, chosen by the class)
        double b[2];
        const bool bad = cf_block_interp<2>(K, cd, du, dv, tabs, xa, xb, b);
        double tp = 0.0, tc = 0.0;
        tp += f[dv][du][0] * nc1;  tc += ((f[dv][du][0] - A.pmin) * A.invd) * nc1;
        tp += f[dv][du][1] * nc2;  tc += ((f[dv][du][1] - A.pmin) * A.invd) * nc2;
        tp += f[dv][du][2] * nc3;  tc += ((f[dv][du][2] - A.pmin) * A.invd) * nc3;
        double hp = tp, hc = tc;
        hp += b[0] * nc0;
        hc += b[1] * nc0;
        gp = cls == 1 ? hp : gp;
        gc = cls == 1 ? hc : gc;
        nbad_here += (cls == 1 && bad) ? 1 : 0;
      }
      if (in[dv][du] && cls != 0) {
        p[iq + off[dv][du]] = gp;
        if (!PHIONLY) cgp[dv * (n0 + 2) + du] = gc;
      }
    }
  if (nbad_here) atomicAdd(nbad, nbad_here);
  if (!PHIONLY && any_valid) {
    // a valid cell of the level behind a partly covered face: the progress variable of the cell itself, read in the box that OWNS it
    // when that box is local (this kernel runs next to the local FillBoundary), in the ghost cell when another rank owns it
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int du = 0; du < 2; ++du) {
        if (!(in[dv][du] && (code[dv][du] & 3u) == 0u)) continue;
        int qq[3] = {q[0], q[1], q[2]};
        qq[t0] += du;
        qq[t1] += dv;
        int sb, xw[3];
        double x;
        if (classify(L, qq[0], qq[1], qq[2], sb, xw) == 0 && sb >= 0) x = M.data[M.off[sb] + fab_index(L.boxes[sb], M.ng, M.ncomp, comp, xw[0], xw[1], xw[2])];
        else x = p[iq + off[dv][du]];
        cgp[dv * (n0 + 2) + du] = (x - A.pmin) * A.invd;
      }
  }
}

// The edge ghost cells of c (outside the box in two directions a < c) that are the boundary ghost of a valid cell of a
// NEIGHBOURING box (k_apply_bc_edges): stored in the ring of the special face they continue.  WHICH edge ghost cells those are, the
// face they continue and their interpolation masks depend on the level's geometry only: a list built once per level
// (k_find_ring; until round 6 every pass re-derived it from three owner-map classifications per edge ghost cell of every box with a
// special face, a 40-us chain of dependent lookups for a few thousand values).  The values read ghost cells of phi that are valid
// cells of the level: from this box's FAB once FillBoundary has filled them (DIRECT = false), or -- DIRECT, an unsharded level -- in
// the box that owns them, so that the work does not wait for FillBoundary and runs next to it.
struct RingItem { int b, q[3], w /* dir | side << 2 | class << 3 */, ef, code, pad; };
__global__ __launch_bounds__(256) void k_find_ring(DLevelView L, const int* sfboxes, int nsfboxes, RingItem* items, int* count, int cap) {
  const int b = sfboxes[blockIdx.y];
  const DBox B = L.boxes[b];
  const int n[3] = {B.hi[0] - B.lo[0] + 1, B.hi[1] - B.lo[1] + 1, B.hi[2] - B.lo[2] + 1};
  long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  int e = -1, which = 0, pos = 0;
  for (int d = 0; d < 3; ++d) {
    if (t < 4LL * n[d]) { e = d; which = (int)((unsigned)t / (unsigned)n[d]); pos = (int)((unsigned)t % (unsigned)n[d]); break; }
    t -= 4LL * n[d];
  }
  if (e < 0) return;
  const int a = (e == 0) ? 1 : 0, c = (e == 2) ? 1 : 2;
  const int sa = which & 1, sc = which >> 1;
  int q[3];
  q[e] = B.lo[e] + pos;
  q[a] = sa ? B.hi[a] + 1 : B.lo[a] - 1;
  q[c] = sc ? B.hi[c] + 1 : B.lo[c] - 1;
  const int cls = classify(L, q[0], q[1], q[2]);
  if (cls == 0) return;
  int qa[3] = {q[0], q[1], q[2]}, qc[3] = {q[0], q[1], q[2]};
  qa[a] += sa ? -1 : 1;
  qc[c] += sc ? -1 : 1;
  const bool va = classify(L, qa[0], qa[1], qa[2]) == 0;
  const bool vc = classify(L, qc[0], qc[1], qc[2]) == 0;
  if (va == vc) return;
  const int dir = va ? a : c, sd = va ? sa : sc;
  if (cls == 2 && !((q[dir] < L.domlo[dir] || q[dir] > L.domhi[dir]) && !L.is_per[dir])) return;
  const int ef = L.sfindex[b * 6 + dir * 2 + sd];
  if (ef < 0) return;
  const int i = atomicAdd(count, 1);
  if (items && i < cap) {
    RingItem R;
    R.b = b; R.q[0] = q[0]; R.q[1] = q[1]; R.q[2] = q[2]; R.w = dir | (sd << 2) | (cls << 3); R.ef = ef;
    R.code = cls == 1 ? (int)(cf_masks(L, q, dir, 2) | 1u) : 0;
    R.pad = 0;
    items[i] = R;
  }
}

template <bool PATCH, bool DIRECT>
__device__ __forceinline__ void prep_ring_item(const PrepLev& Pl, const RingItem& R, int* nbad, const SlotK& sk) {
  const DLevelView& L = Pl.L;
  const DMFView& M = Pl.M;
  const DLevelView& LC = Pl.LC;
  const int z = (int)blockIdx.z;  // component slot
  DMFView MC = Pl.MC;
  PrepArgs A = Pl.A;
  if (sk.prog) { A.pmin = MC.xa = sk.prog[2 * z]; A.invd = MC.xb = sk.prog[2 * z + 1]; }
  const int comp = Pl.comp + z, ccomp = Pl.ccomp + z;
  double* const cgz = L.cg + z * Pl.cg_stride;
  const double* const cpz = L.cp ? L.cp + z * Pl.cp_stride : nullptr;
  const int b = R.b, dir = R.w & 3, sd = (R.w >> 2) & 1, cls = R.w >> 3, ef = R.ef;
  const int q[3] = {R.q[0], R.q[1], R.q[2]};
  const DBox B = L.boxes[b];
  const int n[3] = {B.hi[0] - B.lo[0] + 1, B.hi[1] - B.lo[1] + 1, B.hi[2] - B.lo[2] + 1};
  const int s = sd ? -1 : 1;
  if (cls == 1 && !A.has_crse) { atomicAdd(nbad, 1); return; }
  const double* p = M.data + M.off[b];
  auto phi_at = [&](const int x[3]) -> double {  // a cell one row / plane outside this box that is a valid cell of the level
    if (DIRECT) {
      int sb, xw[3];
      if (classify(L, x[0], x[1], x[2], sb, xw) == 0 && sb >= 0) return M.data[M.off[sb] + fab_index(L.boxes[sb], M.ng, M.ncomp, comp, xw[0], xw[1], xw[2])];
    }
    return p[fab_index(B, M.ng, M.ncomp, comp, x[0], x[1], x[2])];
  };
  double g;
  if (cls == 2) {
    int in[3] = {q[0], q[1], q[2]};
    in[dir] += s;
    const double v = (phi_at(in) - A.pmin) * A.invd;
    g = (A.bc[dir] == PA_BC_REFLECT_ODD) ? -v : v;
  } else {
    bool ok = true;
    double coef[4];
    const int NX = cf_normal_coef(n[dir], A.ratio, coef);
    double bv;
    const long long cpo = (Pl.use_cp && L.cp) ? L.cpoff[ef] : -1;
    if (PATCH || cpo >= 0) {  // the coarse values from the face's patch (its ring of two coarse cells covers the edge ghosts)
      const int xf[1] = {MC.xform};
      double b1[1];
      cf_interp_patch<1>((unsigned)R.code, cpz + cpo, B, sd, MC, q, dir, xf, ok, b1);
      bv = b1[0];
    } else {
      const int xf[1] = {MC.xform};
      double b1[1];
      cf_interp<1>((unsigned)R.code, LC, MC, ccomp, q, dir, A.ratio, xf, ok, b1);  // MC carries the affine view
      bv = b1[0];
    }
    if (!ok) atomicAdd(nbad, 1);
    double tmp = 0.0;
    for (int m = 1; m < NX; ++m) {
      int pc[3] = {q[0], q[1], q[2]};
      pc[dir] += s * m;
      tmp += ((phi_at(pc) - A.pmin) * A.invd) * coef[m];
    }
    g = tmp;
    g += bv * coef[0];
  }
  const int t0 = (dir == 0) ? 1 : 0, t1 = (dir == 2) ? 1 : 2;
  cgz[L.cgoff[ef] + (long long)(q[t1] - B.lo[t1] + 1) * (B.hi[t0] - B.lo[t0] + 3) + (q[t0] - B.lo[t0] + 1)] = g;
}
struct LevRings { const RingItem* it[PA_MAXB]; unsigned n[PA_MAXB]; unsigned w0[PA_MAXB + 1]; };  // level l of the batch owns workgroups w0[l] .. w0[l + 1] - 1
template <bool PATCH, bool DIRECT>
__device__ __forceinline__ void prep_ring_wg(const LevBatch<PrepLev>& Bt, const LevRings& Rg, int* nbad, const SlotK& sk, unsigned w) {
  int blev = 0;
  while (blev + 1 < Bt.n && w >= Rg.w0[blev + 1]) ++blev;
  const unsigned i = (w - Rg.w0[blev]) * 256u + threadIdx.x;
  if (i >= Rg.n[blev]) return;
  prep_ring_item<PATCH, DIRECT>(Bt.a[blev], Rg.it[blev][i], nbad, sk);
}
template <bool PATCH, bool DIRECT = false>
__global__ __launch_bounds__(256) void k_prep_ring(LevBatch<PrepLev> Bt, LevRings Rg, int* nbad, SlotK sk = SlotK()) {
  prep_ring_wg<PATCH, DIRECT>(Bt, Rg, nbad, sk, blockIdx.x);
}

template <bool PATCH, bool PHIONLY = false>
__global__ __launch_bounds__(256) void k_prep_faces_chunks(LevBatch<PrepLev> Bt, LevChunks Ck, LevRings Rg, int* nbad, SlotK sk = SlotK()) {
  // the levels' ring items in front (Rg.w0[Bt.n] workgroups, none when the ring has its own launch): independent of the faces -- they
  // read valid cells in the boxes that own them -- and a longer chain of dependent loads, so they run under the faces' workgroups
  const unsigned nrw = Rg.w0[Bt.n];
  if (blockIdx.x < nrw) { if (!PHIONLY) prep_ring_wg<PATCH, true>(Bt, Rg, nbad, sk, blockIdx.x); return; }
  const unsigned wx = blockIdx.x - nrw;
  int blev = 0;
  while (blev + 1 < Bt.n && wx >= Ck.w0[blev + 1]) ++blev;
  const PrepLev& Pl = Bt.a[blev];
  const SfChunk D = Ck.ck[blev][wx - Ck.w0[blev]];
  const int dir = D.dir_side >> 1;
  // (selects, not D.lo[dir]: a run-time index would send the record through scratch)
  const int e0 = D.hi[0] - D.lo[0] + 1, e1 = D.hi[1] - D.lo[1] + 1, e2 = D.hi[2] - D.lo[2] + 1;
  const int blen = dir == 0 ? e0 : (dir == 1 ? e1 : e2), n0 = dir == 0 ? e1 : e0, n1 = dir == 2 ? e1 : e2;
  const bool cfok = Pl.A.has_crse && Pl.A.ratio == 2 && Pl.use_cp && Pl.L.cp && D.cpoff >= 0 && blen >= 3;  // coarse-fine cells: from the face's coarse patch, four points across the face
  const bool straight = (D.flags & PA_SFC_WALL) != 0 || ((D.flags & PA_SFC_FULL) != 0 && cfok);
  const bool mixed = !straight && blen >= 3 && (cfok || !(D.flags & PA_SFC_HAS_CF));
  if (straight || mixed) {
    __shared__ double tabs[54];
    if (mixed) cf_tab_to_lds(tabs);  // (uniform per workgroup; before any thread leaves)
    const int z = (int)blockIdx.z;  // component slot
    PrepArgs A = Pl.A;
    double xa = Pl.MC.xa, xb = Pl.MC.xb;
    if (sk.prog) { A.pmin = xa = sk.prog[2 * z]; A.invd = xb = sk.prog[2 * z + 1]; }
    double* const cgz = PHIONLY ? nullptr : Pl.L.cg + z * Pl.cg_stride;
    const double* const cpz = Pl.L.cp ? Pl.L.cp + z * Pl.cp_stride : nullptr;
    if (straight) {
      switch (dir) {  // (uniform) compile-time directions: every index into lo / hi / strides is a constant
        case 0: prep_chunk_uniform<0, PHIONLY>(Pl, D, A, xa, xb, Pl.comp + z, cgz, cpz, nbad); break;
        case 1: prep_chunk_uniform<1, PHIONLY>(Pl, D, A, xa, xb, Pl.comp + z, cgz, cpz, nbad); break;
        default: prep_chunk_uniform<2, PHIONLY>(Pl, D, A, xa, xb, Pl.comp + z, cgz, cpz, nbad); break;
      }
    } else {
      switch (dir) {
        case 0: prep_chunk_mixed<0, PHIONLY>(Pl, D, A, xa, xb, Pl.comp + z, cgz, cpz, nbad, tabs); break;
        case 1: prep_chunk_mixed<1, PHIONLY>(Pl, D, A, xa, xb, Pl.comp + z, cgz, cpz, nbad, tabs); break;
        default: prep_chunk_mixed<2, PHIONLY>(Pl, D, A, xa, xb, Pl.comp + z, cgz, cpz, nbad, tabs); break;
      }
    }
    return;
  }
  // what is left: a level that interpolates through the owner map (no coarse patches), boxes thinner than three cells, a level
  // without a coarser one that has coarse-fine cells (counted as errors): cell by cell
  const int hw = D.cw >> 1, sh = 31 - __builtin_clz((unsigned)hw);
  const int u = D.u0 + 2 * ((int)threadIdx.x & (hw - 1)), v = D.v0 + 2 * ((int)threadIdx.x >> sh);
  for (int dv = 0; dv < 2; ++dv)
    for (int du = 0; du < 2; ++du)
      if (u + du >= 0 && v + dv >= 0 && u + du < n0 && v + dv < n1) prep_faces_cell<PATCH, PHIONLY>(Pl, nbad, sk, (unsigned)D.face, (long long)(v + dv) * n0 + (u + du));
}

// the level's compact ghost arrays, allocated on first use (a cache of the level object)
int pa_level_cg(pa_ctx* ctx, const pa_level* Lc, int nsets) {
  pa_level* L = const_cast<pa_level*>(Lc);
  if (L->d_cg && L->cg_sets >= nsets) return 0;
  if (L->d_cg) {  // more component slots than before: a larger buffer (every pass rewrites what it reads)
    PA_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) PA_HIP(hipStreamSynchronize(ctx->stream2));
    (void)hipFree(L->d_cg);
    L->d_cg = nullptr;
  }
  const size_t n = (size_t)std::max<long long>(L->cg_total, 8) * (size_t)nsets;
  PA_HIP(hipMalloc(&L->d_cg, sizeof(double) * n));
  PA_HIP(hipMemsetAsync(L->d_cg, pa_opt().scratch_poison ? 0xFF : 0, sizeof(double) * n, ctx->stream));
  L->cg_sets = nsets;
  L->view.cg = L->d_cg;
  return 0;
}
// PA_SCRATCH_POISON=1: the per-level arrays a pass rewrites before it reads them -- the compact ghost arrays (d_cg) and the compact
// first-layer arrays the sweep hands to the fix-up (d_ncg) -- start the pass as NaN (all bits set), like the work multifabs of
// pa_level_scratch.  Queued on the context's stream by the entry of a pass, BEFORE it forks a side stream: a kernel on any stream
// that reads one of them ahead of the kernel that writes it gets NaN, not what the previous pass left.  d_cp is not touched: its
// PA_CP_MISSING fill is what the gather's regions rely on.  Nothing is queued with the switch off.
int pa_poison_level_caches(pa_ctx* ctx, int nlev, pa_mf* const* state) {
  if (!pa_opt().scratch_poison) return 0;
  for (int l = 0; l < nlev; ++l) {
    const pa_level* L = state[l] ? state[l]->lev : nullptr;
    if (!L) continue;
    const size_t n1 = (size_t)std::max<long long>(L->cg_total, 8);
    if (L->d_cg) PA_HIP(hipMemsetAsync(L->d_cg, 0xFF, sizeof(double) * n1 * (size_t)L->cg_sets, ctx->stream));
    if (L->d_ncg) PA_HIP(hipMemsetAsync(L->d_ncg, 0xFF, sizeof(double) * 6 * n1, ctx->stream));
  }
  return 0;
}
// ... and a multifab the library keeps between passes (the coarse-source copies of a sharded level)
int pa_poison_mf(pa_ctx* ctx, pa_mf* m) {
  if (!pa_opt().scratch_poison || !m || m->total <= 0 || !m->data) return 0;
  PA_HIP(hipMemsetAsync(m->data, 0xFF, sizeof(double) * (size_t)m->total, ctx->stream));
  return 0;
}
// the level's ring items (k_find_ring), built on first use: count, then fill; sorted by (face, position) so that neighbouring threads
// touch neighbouring cells
static int level_ring(pa_ctx* ctx, const pa_level* Lc) {
  pa_level* L = const_cast<pa_level*>(Lc);
  if (L->nring >= 0) return 0;
  if (L->nsfboxes == 0 || L->sfaces.empty()) { L->nring = 0; return 0; }
  int* d_count = nullptr;
  auto fail = [&](const char* what) {
    if (d_count) (void)hipFree(d_count);
    if (L->d_ring) { (void)hipFree(L->d_ring); L->d_ring = nullptr; }
    (void)hipGetLastError();
    return pa_fail(ctx, std::string("ring list: ") + what);
  };
  if (hipMalloc(&d_count, sizeof(int)) != hipSuccess) return fail("device allocation failed");
  const long long nt = 4LL * (L->maxn[0] + L->maxn[1] + L->maxn[2]);
  int n = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 1) {
      if (n == 0) break;
      if (hipMalloc(&L->d_ring, sizeof(RingItem) * (size_t)n) != hipSuccess) { L->d_ring = nullptr; return fail("device allocation failed"); }
    }
    if (hipMemsetAsync(d_count, 0, sizeof(int), ctx->stream) != hipSuccess) return fail("memset failed");
    for (int y0 = 0; y0 < L->nsfboxes; y0 += 65535)
      hipLaunchKernelGGL(k_find_ring, dim3((unsigned)((nt + 255) / 256), (unsigned)std::min(65535, L->nsfboxes - y0)), dim3(256), 0, ctx->stream, L->view, L->d_sfboxes + y0,
                         L->nsfboxes - y0, pass ? (RingItem*)L->d_ring : nullptr, d_count, n);
    int m = 0;
    if (hipMemcpyAsync(&m, d_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("reading the count failed");
    if (pass == 1 && m != n) return fail("the two passes disagree");
    n = m;
  }
  (void)hipFree(d_count);
  d_count = nullptr;
  if (n > 1) {
    std::vector<RingItem> h((size_t)n);
    if (hipMemcpy(h.data(), L->d_ring, sizeof(RingItem) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return fail("download failed");
    std::sort(h.begin(), h.end(), [](const RingItem& a, const RingItem& b) {
      if (a.ef != b.ef) return a.ef < b.ef;
      if (a.q[2] != b.q[2]) return a.q[2] < b.q[2];
      if (a.q[1] != b.q[1]) return a.q[1] < b.q[1];
      return a.q[0] < b.q[0];
    });
    if (hipMemcpy(L->d_ring, h.data(), sizeof(RingItem) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return fail("upload failed");
  }
  L->nring = n;
  return 0;
}


// ---- coarse patches (DLevelView::cp, pa_internal.h): one thread per patch cell fetches the coarse value through the owner
// map of the coarse level (or of this rank's coarse-source copy) -- 1/4 of the fine face cells, once, instead of every
// fine ghost cell walking owner map -> box -> offset before its 5-11 coarse loads.  by_dir: the patch of a face of
// direction d holds component ccomp + d (the coarse normal the fix-up needs), else component ccomp for every face.
struct CpLev { DLevelView L; DLevelView LC; DMFView MC; int ccomp, by_dir; long long cp_stride = 0; int zstride = 1; };  // slot z: component ccomp + zstride z, patches + cp_stride z
__global__ __launch_bounds__(256) void k_cpatch(LevBatch<CpLev> Bt) {
  unsigned fy;
  const CpLev& P = Bt.a[Bt.find(blockIdx.y, fy)];
  const DLevelView& L = P.L;
  const long long off = L.cpoff[fy];
  if (off < 0) return;  // a wall face
  const int e = L.sfaces[fy], dir = (e % 6) >> 1, side = e & 1;
  const DBox B = L.boxes[e / 6];
  int plane, u0, v0, pw, ph;
  cpatch_geom(B, dir, side, plane, u0, v0, pw, ph);
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= (unsigned)(pw * ph)) return;
  const int t0 = dir == 0 ? 1 : 0, t1 = dir == 2 ? 1 : 2;
  const unsigned r = t / (unsigned)pw;
  int p[3];
  p[dir] = plane; p[t0] = u0 + (int)(t - r * (unsigned)pw); p[t1] = v0 + (int)r;
  double v = __longlong_as_double(PA_CP_MISSING);
  const int z = (int)blockIdx.z;
  if (wrap_cell(P.LC, p)) {
    const int cb = owner_of(P.LC, p);
    if (cb >= 0) v = P.MC.data[P.MC.off[cb] + fab_index(P.LC.boxes[cb], P.MC.ng, P.MC.ncomp, P.ccomp + P.zstride * z + (P.by_dir ? dir : 0), p[0], p[1], p[2])];
  }
  L.cp[z * P.cp_stride + off + t] = v;
}
// the same gather from the plan of copy regions (pa_dist.h: CpPlan): no owner-map lookups at all
struct CprLev { DLevelView L; DLevelView LC; DMFView MC; const int* regs; const int* wgs; int nwg, ccomp, by_dir; long long cp_stride = 0; int zstride = 1; };
__global__ __launch_bounds__(256) void k_cpatch_regions(LevBatch<CprLev> Bt) {
  const CprLev& P = Bt.a[blockIdx.y];
  if ((int)blockIdx.x >= P.nwg) return;
  const int* R = P.regs + 12 * P.wgs[2 * blockIdx.x];
  const unsigned t = (unsigned)P.wgs[2 * blockIdx.x + 1] * 256u + threadIdx.x, nu = (unsigned)R[7];
  if (t >= nu * (unsigned)R[8]) return;
  const unsigned b = nu == 1 ? t : __umulhi(t, (unsigned)R[10]), a = t - b * nu;
  const int dir = R[9], t0 = dir == 0 ? 1 : 0, t1 = dir == 2 ? 1 : 2;
  const DLevelView& L = P.L;
  const int e = L.sfaces[R[0]], side = e & 1;
  int plane, u0, v0, pw, ph;
  cpatch_geom(L.boxes[e / 6], dir, side, plane, u0, v0, pw, ph);
  int p[3] = {R[4], R[5], R[6]};
  p[t0] += (int)a; p[t1] += (int)b;
  const int z = (int)blockIdx.z;
  L.cp[z * P.cp_stride + L.cpoff[R[0]] + (long long)(R[3] + (int)b) * pw + (R[2] + (int)a)] =
      P.MC.data[P.MC.off[R[1]] + fab_index(P.LC.boxes[R[1]], P.MC.ng, P.MC.ncomp, P.ccomp + P.zstride * z + (P.by_dir ? dir : 0), p[0], p[1], p[2])];
}
__global__ __launch_bounds__(256) void k_cpatch_clear(double* cp, long long n) {
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t < n) cp[t] = __longlong_as_double(PA_CP_MISSING);
}
static int level_cp(pa_ctx* ctx, const pa_level* Lc, int nsets = 1) {
  pa_level* L = const_cast<pa_level*>(Lc);
  if (L->d_cp && L->cp_sets >= nsets) return 0;
  if (L->d_cp) {
    PA_HIP(hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) PA_HIP(hipStreamSynchronize(ctx->stream2));
    (void)hipFree(L->d_cp);
    L->d_cp = nullptr;
  }
  const long long n = pa_cp_stride(L) * nsets;
  PA_HIP(hipMalloc(&L->d_cp, sizeof(double) * (size_t)n));
  hipLaunchKernelGGL(k_cpatch_clear, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, L->d_cp, n);  // cells without a coarse owner stay "missing"
  L->cp_sets = nsets;
  L->view.cp = L->d_cp;
  return 0;
}
// gather the patches of levels [l0, l1) (those that have a coarse source): one launch
int pa_cpatch_launch(pa_ctx* ctx, int l0, int l1, pa_mf* const* fine, const pa_mf* const* crse, int ccomp, int by_dir, int nslots, int zstride) {
  {  // copy regions when every level of the batch has a plan
    LevBatch<CprLev> Br;
    bool regions = true;
    int mw = 0;
    for (int l = l0; l < l1 && regions; ++l) {
      const pa_level* L = fine[l]->lev;
      if (!crse[l] || L->boxes.empty() || L->sfaces.empty() || L->cp_total == 0) continue;
      if (level_cp(ctx, L, nslots)) return 1;
      const CpPlan* P = pa_cp_plan(ctx, L, crse[l]->lev);
      regions = P && P->ok;
      if (!regions || P->nwg == 0) continue;
      Br.a[Br.n] = CprLev{L->view, crse[l]->lev->view, crse[l]->view, P->d_regs, P->d_wgs, P->nwg, ccomp, by_dir, pa_cp_stride(L), zstride};
      ++Br.n;
      mw = std::max(mw, P->nwg);
    }
    if (regions) {
      if (Br.n) hipLaunchKernelGGL(k_cpatch_regions, dim3((unsigned)mw, (unsigned)Br.n, (unsigned)nslots), dim3(256), 0, ctx->stream, Br);
      return 0;
    }
  }
  LevBatch<CpLev> Bt;
  long long mp = 0;
  for (int l = l0; l < l1; ++l) {
    const pa_level* L = fine[l]->lev;
    if (!crse[l] || L->boxes.empty() || L->sfaces.empty() || L->cp_total == 0) continue;
    if (level_cp(ctx, L, nslots)) return 1;
    Bt.a[Bt.n] = CpLev{L->view, crse[l]->lev->view, crse[l]->view, ccomp, by_dir, pa_cp_stride(L), zstride};
    Bt.ycum[Bt.n + 1] = Bt.ycum[Bt.n] + (int)L->sfaces.size();
    ++Bt.n;
    const long long n0 = L->maxn[0] / 2 + 8, n1 = L->maxn[1] / 2 + 8, n2 = L->maxn[2] / 2 + 8;
    mp = std::max(mp, std::max(n1 * n2, std::max(n0 * n2, n0 * n1)));
  }
  if (Bt.n) hipLaunchKernelGGL(k_cpatch, dim3((unsigned)((mp + 255) / 256), (unsigned)Bt.ycum[Bt.n], (unsigned)nslots), dim3(256), 0, ctx->stream, Bt);
  return 0;
}

// before the sweeps: face ghosts of phi + resolved ghost c (faces and ring) of several levels, one launch pair for up to
// PA_MAXB levels.  crse[l]: the coarser level's phi (component ccomp) or this rank's coarse-source copy of it, null on
// level 0 / where this rank has no coarse-fine face; the local half of FillBoundary(2) must have run.
// phase: 1 = the faces (k_prep_faces: reads valid cells and coarse data only, so it may run NEXT TO FillBoundary), 2 = the
// ring (k_prep_ring: reads ghost cells FillBoundary fills), 3 = both
// nslots > 1: components comp .. comp + nslots - 1 (coarse components ccomp ..) in one launch each, slot z with the progress
// range prog[2 z], prog[2 z + 1] (device) and its own set of compact arrays / coarse patches (SlotK)
// phase & 4: the ring reads its neighbours' cells in the boxes that own them (unsharded levels only), not the ghost cells
// phase & 8 (with 1): only the face ghosts of phi (k_prep_faces<.., PHIONLY>): pa_grad_run's applyBC of every level in one launch
int pa_gradcurv_prep_levels(pa_ctx* ctx, int nlev, pa_mf* const* phi, int comp, const pa_mf* const* crse, int ccomp, const int32_t bc[3], double pmin, double pmax, int phase,
                            int nslots, const double* prog) {
  bool direct = (phase & 4) != 0;
  for (int l = 0; l < nlev; ++l) direct = direct && phi[l]->lev->nranks == 1;
  SlotK sk;
  sk.prog = prog;
  const bool use_cp = PA_USE_CPATCH;  // the patches are gathered with the faces (phase 1) and still hold the coarse phi when the ring runs (phase 2)
  for (int l0 = 0; l0 < nlev; l0 += PA_MAXB) {
    if (use_cp && (phase & 1) && pa_cpatch_launch(ctx, l0, std::min(nlev, l0 + PA_MAXB), phi, crse, ccomp, 0, nslots, 1)) return 1;  // before P.L = L->view picks up cp
    LevBatch<PrepLev> Bf;
    const pa_level* batch_lev[PA_MAXB] = {};
    long long ntf = 0;
    for (int l = l0; l < nlev && l < l0 + PA_MAXB; ++l) {
      const pa_level* L = phi[l]->lev;
      if (L->boxes.empty()) continue;
      if (!(phase & 8) && pa_level_cg(ctx, L, nslots)) return 1;  // phase & 8: phi only (the gradient tool), no compact arrays
      if (L->sfaces.empty()) continue;
      PrepLev P;
      P.cg_stride = pa_cg_stride(L); P.cp_stride = pa_cp_stride(L);
      for (int d = 0; d < 3; ++d) P.A.bc[d] = bc[d];
      P.A.ratio = 2; P.A.has_crse = crse[l] ? 1 : 0; P.A.pmin = pmin; P.A.invd = 1.0 / (pmax - pmin);
      P.L = L->view; P.M = phi[l]->view; P.comp = comp;
      P.LC = crse[l] ? crse[l]->lev->view : L->view;
      P.MC = crse[l] ? crse[l]->view : phi[l]->view;
      P.MC.xform = 1; P.MC.xa = pmin; P.MC.xb = P.A.invd;
      P.ccomp = ccomp;
      P.use_cp = (use_cp && crse[l] && L->cp_total > 0) ? 1 : 0;
      P.wg = (const int2*)L->d_sfwg; P.nwg = L->nsfwg; P.sfboxes = L->d_sfboxes;
      const long long n0 = L->maxn[0], n1 = L->maxn[1], n2 = L->maxn[2];
      ntf = std::max(ntf, std::max(n1 * n2, std::max(n0 * n2, n0 * n1)));
      batch_lev[Bf.n] = L;
      Bf.a[Bf.n] = P; Bf.ycum[Bf.n + 1] = Bf.ycum[Bf.n] + (int)L->sfaces.size(); ++Bf.n;
    }
    if (!Bf.n) continue;
    ProfScope prof(ctx, PA_TAG_BC);
    bool all_patch = true;  // every level of the batch that has a coarser level interpolates from patches: the owner-map path is not compiled in
    for (int q = 0; q < Bf.n; ++q) all_patch = all_patch && (Bf.a[q].use_cp || !Bf.a[q].A.has_crse);
    // the faces from the levels' chunk records (k_prep_faces_chunks; every level with special faces has them)
    LevChunks Ck;
    Ck.w0[0] = 0;
    for (int q = 0; q < Bf.n; ++q) {
      const pa_level* Lq = batch_lev[q];
      if (!Lq->d_sfchunk || Lq->nsfchunk <= 0) return pa_fail(ctx, "pa_gradcurv_prep_levels: a level without chunk records");
      Ck.ck[q] = Lq->d_sfchunk;
      Ck.w0[q + 1] = Ck.w0[q] + (unsigned)Lq->nsfchunk;
    }
    // the ring items of the batch's levels (level_ring): with the faces' launch when both are asked for and the ring reads its
    // neighbours in place (one rank), else a launch of their own
    LevRings Rg, Rnone;
    Rg.w0[0] = 0;
    for (int q = 0; q <= PA_MAXB; ++q) Rnone.w0[q] = 0;
    for (int q = 0; q < PA_MAXB; ++q) { Rnone.it[q] = nullptr; Rnone.n[q] = 0; }
    if (phase & 2)
      for (int q = 0; q < Bf.n; ++q) {
        const pa_level* Lq = batch_lev[q];
        if (level_ring(ctx, Lq)) return 1;
        Rg.it[q] = (const RingItem*)Lq->d_ring;
        Rg.n[q] = (unsigned)Lq->nring;
        Rg.w0[q + 1] = Rg.w0[q] + (unsigned)((Lq->nring + 255) / 256);
      }
    // (few items -- large faces -- hide under the faces: headline 5.913 -> 5.895 ms per pass; the long lists of a BoxArray of many small boxes
    // are latency-bound work that wants its own launch at its own occupancy: irregular hierarchy 6.39 against 6.48 ms merged)
    const bool ring_with_faces = (phase & 1) && (phase & 2) && !(phase & 8) && direct && Rg.w0[Bf.n] * 8u <= Ck.w0[Bf.n];
    if (phase & 1) {
      const LevRings& Rk = ring_with_faces ? Rg : Rnone;
      const dim3 gc(Rk.w0[Bf.n] + Ck.w0[Bf.n], 1, (unsigned)nslots);
      if (phase & 8) {
        if (all_patch) hipLaunchKernelGGL((k_prep_faces_chunks<true, true>), gc, dim3(256), 0, ctx->stream, Bf, Ck, Rk, ctx->d_flags, sk);
        else hipLaunchKernelGGL((k_prep_faces_chunks<false, true>), gc, dim3(256), 0, ctx->stream, Bf, Ck, Rk, ctx->d_flags, sk);
      } else {
        if (all_patch) hipLaunchKernelGGL((k_prep_faces_chunks<true, false>), gc, dim3(256), 0, ctx->stream, Bf, Ck, Rk, ctx->d_flags, sk);
        else hipLaunchKernelGGL((k_prep_faces_chunks<false, false>), gc, dim3(256), 0, ctx->stream, Bf, Ck, Rk, ctx->d_flags, sk);
      }
    }
    if ((phase & 2) && !ring_with_faces && Rg.w0[Bf.n] > 0) {
      const dim3 gr(Rg.w0[Bf.n], 1, (unsigned)nslots);
      if (all_patch && direct) hipLaunchKernelGGL((k_prep_ring<true, true>), gr, dim3(256), 0, ctx->stream, Bf, Rg, ctx->d_flags, sk);
      else if (direct) hipLaunchKernelGGL((k_prep_ring<false, true>), gr, dim3(256), 0, ctx->stream, Bf, Rg, ctx->d_flags, sk);
      else if (all_patch) hipLaunchKernelGGL(k_prep_ring<true>, gr, dim3(256), 0, ctx->stream, Bf, Rg, ctx->d_flags, sk);
      else hipLaunchKernelGGL(k_prep_ring<false>, gr, dim3(256), 0, ctx->stream, Bf, Rg, ctx->d_flags, sk);
    }
  }
  PA_HIP(hipGetLastError());
  return 0;
}
