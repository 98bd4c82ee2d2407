// pa_fused_irreg.hip -- fused grad -> curvature: which cells of a general BoxArray are irregular, and the Gaussian-curvature
// fix-up (gfx950).
//
// Exact-normal pipeline only.  k_find_irregular lists, once per level, the boundary cells whose curvature neither the sweep nor
// the face fix-up gets right; pa_gradcurv_fix_levels (pa_fused_fix.hip) recomputes them with k_curv_general*.  k_gauss_cells
// recomputes the Gaussian curvature of the KG sweep (pa_curvature_run's fast path) in the first layer behind special faces and in
// those irregular cells.  pa_fused2_level_ok says whether a level can take the exact-normal pipeline at all.
// Entry points: pa_level_irregular_cells (C ABI); pa_fused2_level_ok, pa_gauss_cells_levels (pa_internal.h); pa_level_irregular
// (pa_fused.h).
#include "pa_fused.h"
#include "pa_fabview.h"
#include <algorithm>

// ===================================================================================== irregular cells (general BoxArrays)
// The exact-normal pipeline leaves the flame normal exact in EVERY valid cell whatever the BoxArray looks like: a cell's normal
// needs the progress variable in the six face neighbours only, and a face ghost cell holds one well-defined value (a valid
// cell's, or the reference's boundary condition of the face's direction).  The CURVATURE of a boundary cell X of box B needs
// the normal of the ghost cell Y behind the face; where Y is a valid cell of a neighbouring box N, the sweep forms that
// normal from the progress variable around Y as B's FAB holds it, and that is N's view of it only if every tangential
// neighbour Z of Y is a valid cell too -- or the ghost cell of exactly one reader.  On general BoxArrays it is not:
//   * a face that is partly covered by a neighbour and partly coarse-fine: at the line where it changes, Z is a face ghost of
//     B (boundary condition normal to B's face) AND N's ghost cell in the tangential direction (another boundary value);
//   * a concave coarse-fine corner: the edge ghost Z has two valid neighbours in two boxes, each with its own boundary value.
// k_find_irregular lists those cells X (a property of the BoxArray, found once per level): a boundary cell with a valid ghost
// neighbour Y = X + s e_d is REGULAR if, for both tangential directions t and both signs, Z = Y +- e_t is
//   - a valid cell, reached through a FAB slot the sweep / the fix-up read as such: Z inside the face's extent, or an edge
//     ghost whose two faces (d and t) are both ordinary -- the ring of a special face holds no valid cells' values;
//   - or an edge ghost that is not a valid cell while W = X +- e_t is not one either and face d is ordinary: the convex corner
//     the face fix-up handles (X lies in the first layer behind the special face t, the ring of that face's compact array holds
//     N's boundary value: k_prep_ring);
// and the second ghost layer Y + s e_d is a valid cell (N at least two cells thick).  Everything else is irregular.  The
// rule is deliberately conservative: an irregular cell costs a few hundred dependent loads once per pass, a missed one a
// wrong curvature.  k_curv_general (pa_fused_fix.hip) then recomputes K of the listed cells.
__global__ __launch_bounds__(256) void k_find_irregular(DLevelView L, int y0, int4* items, int* count, int cap) {
  const int row = (int)blockIdx.y + y0, b = row / 6, f = row % 6;
  if (b >= L.nboxes) return;
  const DBox B = L.boxes[b];
  const int fdir = f >> 1, fside = f & 1;
  const int t0 = fdir == 0 ? 1 : 0, t1 = fdir == 2 ? 1 : 2;
  const unsigned n0 = B.hi[t0] - B.lo[t0] + 1, n1 = B.hi[t1] - B.lo[t1] + 1;
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= n0 * n1) return;
  int X[3];
  X[fdir] = fside ? B.hi[fdir] : B.lo[fdir];
  X[t0] = B.lo[t0] + (int)(t % n0);
  X[t1] = B.lo[t1] + (int)(t / n0);
  for (int g = 0; g < f; ++g)  // a cell on an edge / corner of the box belongs to the lowest-numbered face it touches
    if (X[g >> 1] == ((g & 1) ? B.hi[g >> 1] : B.lo[g >> 1])) return;
  bool irr = false;
  for (int g = 0; g < 6 && !irr; ++g) {
    const int d = g >> 1, sg = (g & 1) ? 1 : -1;
    if (X[d] != ((g & 1) ? B.hi[d] : B.lo[d])) continue;
    int Y[3] = {X[0], X[1], X[2]};
    Y[d] += sg;
    if (classify(L, Y[0], Y[1], Y[2]) != 0) continue;  // boundary condition on n itself: exact from the box's own normals
    const bool fd_special = L.sfindex[b * 6 + g] >= 0;
    // a valid ghost cell behind a SPECIAL face (one that is coarse-fine elsewhere): the sweep's ghost row / column / plane of
    // such a face comes from the compact array and its second stream -- the row beyond, which the ghost normal needs -- is
    // re-aimed at that array (pa_fused_march3.h), so no ghost normal behind a special face is usable.  In the interior of
    // the face k_faces_curv_fast forms the curvature with the neighbouring box's final normal (when that box is local);
    // cells on the face's perimeter and ghost cells owned by another rank's box are listed
    if (fd_special) {
      bool other = false;
      for (int tt = 0; tt < 3; ++tt) other = other || (tt != d && (X[tt] == B.lo[tt] || X[tt] == B.hi[tt]));
      int sb, yw[3];
      (void)classify(L, Y[0], Y[1], Y[2], sb, yw);
      if (other || sb < 0) irr = true;
      continue;
    }
    {
      int Y2[3] = {Y[0], Y[1], Y[2]};
      Y2[d] += sg;
      if (classify(L, Y2[0], Y2[1], Y2[2]) != 0) irr = true;
    }
    for (int tt = 0; tt < 3 && !irr; ++tt) {
      if (tt == d) continue;
      for (int s2 = 0; s2 < 2 && !irr; ++s2) {
        const int sg2 = s2 ? 1 : -1;
        int Z[3] = {Y[0], Y[1], Y[2]};
        Z[tt] += sg2;
        const bool zvalid = classify(L, Z[0], Z[1], Z[2]) == 0;
        if (Z[tt] >= B.lo[tt] && Z[tt] <= B.hi[tt]) { irr = !zvalid; continue; }
        int W[3] = {X[0], X[1], X[2]};
        W[tt] += sg2;
        const bool ft_special = L.sfindex[b * 6 + tt * 2 + s2] >= 0;
        if (!zvalid) irr = !(classify(L, W[0], W[1], W[2]) != 0 && !fd_special);
        else irr = fd_special || ft_special;
      }
    }
  }
  if (!irr) return;
  const int i = atomicAdd(count, 1);
  if (items && i < cap) items[i] = make_int4(b, X[0], X[1], X[2]);
}

// the level's list of irregular cells, built on first use (a cache of the level object, like pa_level_cg)
int pa_level_irregular(pa_ctx* ctx, const pa_level* Lc) {
  pa_level* L = const_cast<pa_level*>(Lc);
  if (L->nirr >= 0) return 0;
  const int nb = (int)L->boxes.size();
  if (nb == 0) { L->nirr = 0; return 0; }
  const long long n0 = L->maxn[0], n1 = L->maxn[1], n2 = L->maxn[2];
  const long long nf = std::max(n1 * n2, std::max(n0 * n2, n0 * n1));
  int* d_count = nullptr;
  // every error path releases the counter and the half-built list: nirr stays -1, so the next call starts over (advisor, round 4)
  auto fail = [&](const char* what) {
    if (d_count) (void)hipFree(d_count);
    if (L->d_irr) { (void)hipFree(L->d_irr); L->d_irr = nullptr; }
    (void)hipGetLastError();
    return pa_fail(ctx, std::string("irregular-cell list: ") + what);
  };
  if (L->d_irr) { (void)hipFree(L->d_irr); L->d_irr = nullptr; }  // left by a call that failed before this guard existed
  if (hipMalloc(&d_count, sizeof(int)) != hipSuccess) return fail("device allocation failed");
  int n = 0;
  for (int pass = 0; pass < 2; ++pass) {  // count, then fill
    if (pass == 1) {
      if (n == 0) break;
      if (hipMalloc(&L->d_irr, sizeof(int4) * (size_t)n) != hipSuccess) { L->d_irr = nullptr; return fail("device allocation failed"); }
    }
    if (hipMemsetAsync(d_count, 0, sizeof(int), ctx->stream) != hipSuccess) return fail("memset failed");
    for (int y0 = 0; y0 < nb * 6; y0 += 65535 / 6 * 6)
      hipLaunchKernelGGL(k_find_irregular, dim3((unsigned)((nf + 255) / 256), (unsigned)std::min(65535 / 6 * 6, nb * 6 - y0)), dim3(256), 0, ctx->stream, L->view, y0,
                         pass ? (int4*)L->d_irr : nullptr, d_count, n);
    int m = 0;
    if (hipMemcpyAsync(&m, d_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("reading the count failed");
    if (pass == 1 && m != n) return fail("the two passes disagree");
    n = m;
  }
  (void)hipFree(d_count);
  d_count = nullptr;
  if (n > 1) {  // the kernel appended the cells in any order: sort by (box, k, j, i) so that neighbouring threads touch neighbouring cells
    std::vector<int4> h((size_t)n);
    if (hipMemcpy(h.data(), L->d_irr, sizeof(int4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return fail("download failed");
    std::sort(h.begin(), h.end(), [](const int4& a, const int4& b) {
      if (a.x != b.x) return a.x < b.x;
      if (a.w != b.w) return a.w < b.w;
      if (a.z != b.z) return a.z < b.z;
      return a.y < b.y;
    });
    if (hipMemcpy(L->d_irr, h.data(), sizeof(int4) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) return fail("upload failed");
  }
  L->nirr = n;
  return 0;
}
extern "C" int64_t pa_level_irregular_cells(pa_ctx* ctx, const pa_level* L) {
  PaBind bind_(ctx);
  if (!ctx || !L) return -1;
  if (pa_level_irregular(ctx, L)) return -1;
  return L->nirr;
}

// can the exact-normal pipeline run on this level (same answer on every rank of a sharded level)?
bool pa_fused2_level_ok(const pa_level* L) {
  // ANY BoxArray whose boxes are at least three cells thick: general BoxArrays (concave coarse-fine corners, faces partly covered by a
  // neighbour) have their irregular cells listed per level and recomputed after the fix-up (k_curv_general); boxes at most 32 cells
  // wide run k_gradcurv_march3n's CG variant
  const std::vector<DBox>& all = L->gboxes.empty() ? L->boxes : L->gboxes;
  for (const DBox& B : all)
    for (int d = 0; d < 3; ++d)
      if (B.hi[d] - B.lo[d] + 1 < 3) return false;
  return true;
}

// ---- round 6: the Gaussian curvature of the cells the KG sweep cannot get right (pa_fused_march3.h, GOUT == 2): the first layer behind
// every special face -- its ghost G is the boundary condition on G (the caller has run FillBoundary + applyBC on the stored G), not what
// the sweep forms from ghost c -- and the level's irregular cells.  k_gauss_curv's operations (pa_curvopts.hip) on the stored G, a thread
// per 2 x 2 block of a chunk record / per listed cell; every other cell keeps the sweep's value, which is the same arithmetic on the
// same values.
struct GaussFixLev { DLevelView L; DMFView G, O; int pc, kgc; double thr; const SfChunk* ck; unsigned nck; const int4* irr; unsigned nirr; unsigned w0; };
__device__ __forceinline__ void gauss_cell(const GaussFixLev& A, int b, int i, int j, int k) {
  const DBox V = A.L.boxes[b];
  const FabView G = mf_view(A.G, V, b), O = mf_view(A.O, V, b);
  double H[3][3], g[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double c0 = G(i, j, k, d);
    g[d] = c0;
    H[d][0] = cdiff(A.L.dxinv[0], G(i - 1, j, k, d), c0, G(i + 1, j, k, d));
    H[d][1] = cdiff(A.L.dxinv[1], G(i, j - 1, k, d), c0, G(i, j + 1, k, d));
    H[d][2] = cdiff(A.L.dxinv[2], G(i, j, k - 1, d), c0, G(i, j, k + 1, d));
  }
  const double ax0 = H[1][1] * H[2][2] - H[2][1] * H[1][2];
  const double ay0 = H[1][2] * H[2][0] - H[2][2] * H[1][0];
  const double az0 = H[1][0] * H[2][1] - H[2][0] * H[1][1];
  const double ax1 = H[0][2] * H[2][1] - H[2][2] * H[0][1];
  const double ay1 = H[0][0] * H[2][2] - H[2][0] * H[0][2];
  const double az1 = H[0][1] * H[2][0] - H[2][1] * H[0][0];
  const double ax2 = H[0][1] * H[1][2] - H[1][1] * H[0][2];
  const double ay2 = H[0][2] * H[1][0] - H[1][2] * H[0][0];
  const double az2 = H[0][0] * H[1][1] - H[1][0] * H[0][1];
  const double cx = g[0], cy = g[1], cz = g[2];
  const double sn = sqrt(cx * cx + cy * cy + cz * cz);
  const double gn = (1e-14 < sn) ? sn : 1e-14;
  double kg = (cx * (ax0 * cx + ax1 * cy + ax2 * cz) + cy * (ay0 * cx + ay1 * cy + ay2 * cz) + cz * (az0 * cx + az1 * cy + az2 * cz)) / ((gn * gn) * (gn * gn));
  if (A.thr >= 0.0) {
    const double p = O(i, j, k, A.pc);
    if (p < A.thr || p > 1.0 - A.thr) kg = 0.0;
  }
  O(i, j, k, A.kgc) = kg;
}
__global__ __launch_bounds__(256) void k_gauss_cells(LevBatch<GaussFixLev> Bt) {
  int l = 0;
  while (l + 1 < Bt.n && blockIdx.x >= Bt.a[l + 1].w0) ++l;
  const GaussFixLev& A = Bt.a[l];
  const unsigned w = blockIdx.x - A.w0;
  if (w < A.nck) {  // a chunk of a special face: the first-layer cells behind its ghost cells
    const SfChunk D = A.ck[w];
    const int dir = D.dir_side >> 1, side = D.dir_side & 1;
    const int e0 = D.hi[0] - D.lo[0] + 1, e1 = D.hi[1] - D.lo[1] + 1, e2 = D.hi[2] - D.lo[2] + 1;
    const int n0 = dir == 0 ? e1 : e0, n1 = dir == 2 ? e1 : e2;
    // the chunk's cw x ch = 1024 cells, a cell per thread and pass with u fastest (consecutive lanes = consecutive cells along the row
    // for y and z faces; the 2 x 2 blocks of the boundary-condition kernels would read every other cell per pass)
    const int sh = 31 - __builtin_clz((unsigned)D.cw);
#pragma unroll 2
    for (int r = 0; r < 4; ++r) {
      const int c = (int)threadIdx.x + 256 * r;
      const int uu = D.u0 + (c & (D.cw - 1)), vv = D.v0 + (c >> sh);
      if (uu < 0 || vv < 0 || uu >= n0 || vv >= n1) continue;
      int i, j, k;
      if (dir == 0) { i = side ? D.hi[0] : D.lo[0]; j = D.lo[1] + uu; k = D.lo[2] + vv; }
      else if (dir == 1) { i = D.lo[0] + uu; j = side ? D.hi[1] : D.lo[1]; k = D.lo[2] + vv; }
      else { i = D.lo[0] + uu; j = D.lo[1] + vv; k = side ? D.hi[2] : D.lo[2]; }
      gauss_cell(A, D.box, i, j, k);
    }
    return;
  }
  const unsigned q = (w - A.nck) * 256u + threadIdx.x;
  if (q < A.nirr) {
    const int4 it = A.irr[q];
    gauss_cell(A, it.x, it.y, it.z, it.w);
  }
}
// G[l]: components 0 .. 2, >= 1 ghost layer, FillBoundary + applyBC done; out[l]: Progress at pc (read for the clip), Kg written at kgc
int pa_gauss_cells_levels(pa_ctx* ctx, int nlev, pa_mf* const* G, pa_mf* const* out, int pc, int kgc, double thr) {
  for (int l0 = 0; l0 < nlev; l0 += PA_MAXB) {
    LevBatch<GaussFixLev> Bt;
    unsigned w = 0;
    for (int l = l0; l < nlev && l < l0 + PA_MAXB; ++l) {
      const pa_level* L = out[l]->lev;
      if (L->boxes.empty()) continue;
      if (G[l]->lev != L || G[l]->ng < 1 || G[l]->ncomp < 3) return pa_fail(ctx, "pa_gauss_cells_levels: G needs 3 components and a ghost layer on the level of out");
      if (L->nirr < 0 && pa_level_irregular(ctx, L)) return 1;
      GaussFixLev A{L->view, G[l]->view, out[l]->view, pc, kgc, thr, L->d_sfchunk, (unsigned)L->nsfchunk, (const int4*)L->d_irr, (unsigned)std::max(L->nirr, 0), w};
      w += A.nck + (A.nirr + 255u) / 256u;
      Bt.a[Bt.n++] = A;
    }
    if (!Bt.n || w == 0) continue;
    hipLaunchKernelGGL(k_gauss_cells, dim3(w), dim3(256), 0, ctx->stream, Bt);
  }
  PA_HIP(hipGetLastError());
  return 0;
}
