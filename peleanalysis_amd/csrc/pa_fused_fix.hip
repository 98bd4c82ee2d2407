// pa_fused_fix.hip -- fused grad -> curvature, stage 3 of 3: the fix-up behind special faces (gfx950).
//
// After the sweeps, the cells whose result depends on a boundary condition the sweep cannot know are recomputed:
//   * the ghost NORMAL beyond a coarse-fine or physical face comes from MLMG applyBC on n_d itself (curvature.cpp:510-531;
//     SURVEY A.3), not from c;
//   * the ghost PROGRESS VARIABLE there comes from applyBC on c (curvature.cpp:443-457), which is not (phi_ghost - pmin) * invdenom
//     at coarse-fine and reflect_odd faces.
// First fused pipeline (PA_FUSED2=0, level 0 with boxes thinner than three cells): pa_gradcurv_faces_phase, per level, two layers
//   from a resolved shell copy of c -- k_faces_normal, k_faces_curv_fast<2>, k_faces_curv<false>.
// Exact-normal pipeline (default): pa_gradcurv_fix_levels, all levels per launch, the first layer only (the CG sweep left N
//   final: pa_fused_prep.hip) -- k_faces_fix_chunks + k_faces_curv_tab, with the threshold clip k_faces_curv_fast<1, .., CLIP> +
//   k_faces_curv_list + k_faces_curv_tab; then the level's irregular cells (listed by pa_fused_irreg.hip) through
//   k_curv_general*, which live here because this unit launches them.
// Entry points: pa_gradcurv_faces_level, pa_last_slow_cells (C ABI); pa_gradcurv_faces_phase, pa_gradcurv_fix_levels (pa_internal.h).
#include "pa_fused.h"
#include "pa_dist.h"
#include "pa_fabview.h"
#include "pa_fused_march.h"
#include <cstdlib>

#ifndef PA_FC_WAVES
#define PA_FC_WAVES 3  /* measured: 1 -> 1.30, 2 -> 1.34, 3 -> 1.21, 4 (spills) -> 2.28 ms of face fix-up per step */
#endif
struct Vec3 { double x, y, z; };

// Where the face fix-up reads the progress variable from.
// ShellAcc: the stored copy with resolved ghost cells (`work`, filled in a shell around the special faces).
struct ShellAcc {
  FabView C;
  int cc;
  __device__ __forceinline__ double operator()(int i, int j, int k) const { return C(i, j, k, cc); }
};
// CgAcc (exact-normal pipeline, below): nothing is stored but the ghost values behind special faces.  A cell of the box
// or a ghost cell that is a valid cell of the level: (phi - pmin) * invdenom; the ghost cell behind a special face: that
// face's compact array; an edge ghost (outside in two directions): the ring of the special one of the two faces.
struct CgAcc {
  const DLevelView* L;
  FabView P;
  DBox B;
  int b, pcomp;
  double pmin, invd;
  const double* cg;  // the component slot's set of compact arrays (L->cg + slot * stride)
  __device__ __forceinline__ double operator()(int i, int j, int k) const {
    const int p[3] = {i, j, k};
    int nout = 0, fd[2] = {0, 0}, fs[2] = {0, 0};
    bool near = true;  // within one cell of the box in every direction
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int o = p[d] < B.lo[d] ? B.lo[d] - p[d] : (p[d] > B.hi[d] ? p[d] - B.hi[d] : 0);
      if (o) {
        if (nout < 2) { fd[nout] = d; fs[nout] = p[d] > B.hi[d]; }
        ++nout;
        near = near && o == 1;
      }
    }
    int e = -1, d = 0;
    if (near && nout == 1) { d = fd[0]; e = L->sfindex[b * 6 + d * 2 + fs[0]]; }
    if (near && nout == 2) {
      const int ea = L->sfindex[b * 6 + fd[0] * 2 + fs[0]], ec = L->sfindex[b * 6 + fd[1] * 2 + fs[1]];
      if (ea >= 0 && ec >= 0) return 0.0;  // needed by nobody (its face-ring neighbours are not valid cells either)
      if (ea >= 0) { e = ea; d = fd[0]; }
      if (ec >= 0) { e = ec; d = fd[1]; }
    }
    if (e < 0) return (P(i, j, k, pcomp) - pmin) * invd;
    const int t0 = (d == 0) ? 1 : 0, t1 = (d == 2) ? 1 : 2;
    return cg[L->cgoff[e] + (long long)(p[t1] - B.lo[t1] + 1) * (B.hi[t0] - B.lo[t0] + 3) + (p[t0] - B.lo[t0] + 1)];
  }
};

// flame normal n = G/normgrad at cell (i,j,k), from c
template <typename Acc>
__device__ __forceinline__ Vec3 normal_at(const Acc& C, int i, int j, int k, const double dxinv[3]) {
  Vec3 n;
  normal_from(C(i - 1, j, k), C(i + 1, j, k), C(i, j - 1, k), C(i, j + 1, k), C(i, j, k - 1), C(i, j, k), C(i, j, k + 1), dxinv, n.x, n.y, n.z);
  return n;
}

struct FaceArgs {
  int bc[3];
  int ratio;
  int has_crse;
  int layers;  // cells per face normal that are recomputed (2)
  double thr;
  int perim_only;  // k_faces_curv: only the cells on the perimeter of each face (k_faces_curv_fast does the interior)
  double pmin, invd;  // CgAcc: progress variable from phi
};

// one level's arguments of the curvature fix-up kernels (several levels per launch: LevBatch)
struct FixArgs {
  DLevelView L;
  DMFView MC_;
  int ccomp;
  DLevelView LCr;
  DMFView MN;
  int cncomp0;
  DMFView MO;
  int ncomp0, kcomp;
  FaceArgs A;
  int use_cp = 0;  // the level's coarse patches hold the coarse normal component of each face's direction (k_cpatch ran)
  long long cg_stride = 0, cp_stride = 0;  // component slots (blockIdx.z): doubles between the slots' sets of compact arrays / coarse patches
  const int2* wg = nullptr; int nwg = 0;   // the level's work table {special face, chunk of 256 face cells} (pa_level::d_sfwg)
  const int2* pwg = nullptr; int npwg = 0; // ... {special face, chunk of 256 perimeter cells} (pa_level::d_pfwg)
  // NCG: this pass's sweep mirrored the first-layer data of the special x faces of boxes at least ncg_minw wide (pa_fused_march.h)
  const double* ncg = nullptr; long long ncgs = 0; int ncg_minw = 0;
};
typedef double pa_fix_d2 __attribute__((ext_vector_type(2)));
// the x faces the wide CG sweep mirrors (the tile that holds the face must hold the first three columns behind it: pa_fused_march3.h ncgl / ncgh)
__device__ __forceinline__ bool ncg_face_ok(const DBox& B, int side, int minw) {
  const int nx = B.hi[0] - B.lo[0] + 1;
  return nx >= minw && (side ? ((nx - 1) & 63) + 1 : min(nx, 64)) >= 3;
}
// workgroup -> (batch level, special face, first face cell) through the levels' work tables
template <typename BT>
__device__ __forceinline__ bool wg_decode(const BT& Bt, int& blev, unsigned& fy, long long& t, unsigned w = blockIdx.x) {
  blev = 0;
  while (blev + 1 < Bt.n && w >= (unsigned)Bt.a[blev].nwg) { w -= (unsigned)Bt.a[blev].nwg; ++blev; }
  if (w >= (unsigned)Bt.a[blev].nwg) return false;
  const int2 c = Bt.a[blev].wg[w];
  fy = (unsigned)c.x;
  t = (long long)c.y * 256 + threadIdx.x;
  return true;
}

__device__ __forceinline__ double comp_of(const Vec3& v, int d) { return d == 0 ? v.x : (d == 1 ? v.y : v.z); }

__device__ __forceinline__ bool in_box(const DBox& B, const int q[3]) {
  return q[0] >= B.lo[0] && q[0] <= B.hi[0] && q[1] >= B.lo[1] && q[1] <= B.hi[1] && q[2] >= B.lo[2] && q[2] <= B.hi[2];
}

// Phase A: thread per layer-1 cell of a special face whose ghost cell is not a valid cell.  Its
// normal depends on the resolved ghost c (applyBC on c), which the sweep did not have: recompute.
__global__ __launch_bounds__(256) void k_faces_normal(DLevelView L, DMFView MC_, int ccomp, DMFView MO, int ncomp0, FaceArgs A) {
  int b, dir, side, layer, q[3];
  DBox B;
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (!sface_decode(L, blockIdx.y, t, 1, b, B, dir, side, q, layer)) return;
  if ((L.sfcode[L.sfoff[blockIdx.y] + t] & 3u) == 0) return;  // ordinary same-level ghost: the sweep was exact
  int X[3] = {q[0], q[1], q[2]};
  X[dir] += side ? -1 : 1;
  const ShellAcc C = {mf_view(MC_, B, b), ccomp};
  const double dxinv[3] = {L.dxinv[0], L.dxinv[1], L.dxinv[2]};
  Vec3 no = normal_at(C, X[0], X[1], X[2], dxinv);
  if (A.thr >= 0.0) {
    const double c0 = C(X[0], X[1], X[2]);
    if (c0 < A.thr || c0 > 1.0 - A.thr) { no.x = 0.0; no.y = 0.0; no.z = 0.0; }
  }
  double* o = MO.data + MO.off[b];
  o[fab_index(B, MO.ng, MO.ncomp, ncomp0, X[0], X[1], X[2])] = no.x;
  o[fab_index(B, MO.ng, MO.ncomp, ncomp0 + 1, X[0], X[1], X[2])] = no.y;
  o[fab_index(B, MO.ng, MO.ncomp, ncomp0 + 2, X[0], X[1], X[2])] = no.z;
}

// Phase B: thread per (cell, layer 1..2) behind such a ghost cell: K = 0.5 * div n with the ghost
// normals of MLMG applyBC on n_d (curvature.cpp:510-546).  Normals of cells of this box are read
// back from the output (exact after phase A) unless the threshold clip zeroed them there; normals
// of valid cells of neighbouring boxes are recomputed from the local ghost c.
// CG = false: c from the stored shell copy MC_[ccomp]; CG = true: MC_[ccomp] is PHI and c comes through CgAcc.
// cells the clip-aware fast path hands to the general one (exact-normal pipeline with the threshold clip): {batch row, face cell}
struct SlowList {
  int* count; int2* items; int cap;
  // cells with a VALID ghost cell (general BoxArrays) that need the neighbouring box's unclipped normal: a list for k_curv_general
  int* gcount = nullptr; int4* gitems = nullptr; int gcap = 0; unsigned glev = 0;
};
// CGCLIP: the threshold clip in the exact-normal pipeline (compiled in only where it is used: 116 against 168 VGPRs)
template <bool CG, bool PATCH, bool CGCLIP = false>
__device__ __forceinline__ void faces_curv_cell(const LevBatch<FixArgs>& Bt, unsigned y, long long t, int perim_only, int* nbad, const SlotK& sk, int z) {
  unsigned fy;
  const FixArgs& Fx = Bt.a[Bt.find(y, fy)];
  const DLevelView& L = Fx.L;
  const DMFView& MC_ = Fx.MC_;
  const DLevelView& LCr = Fx.LCr;
  const DMFView& MN = Fx.MN;
  const DMFView& MO = Fx.MO;
  FaceArgs A = Fx.A;
  if (sk.prog) { A.pmin = sk.prog[2 * z]; A.invd = sk.prog[2 * z + 1]; }
  const int ccomp = Fx.ccomp + z, cncomp0 = Fx.cncomp0 + sk.cn_z * z, ncomp0 = Fx.ncomp0 + 8 * z, kcomp = Fx.kcomp + 8 * z;
  const double* cgz = L.cg + z * Fx.cg_stride;
  const double* cpz = L.cp ? L.cp + z * Fx.cp_stride : nullptr;
  int b, fdir, side, layer, q0[3];
  DBox B;
  if (perim_only) {
    // compact enumeration of the perimeter cells of the face (the interior belongs to k_faces_curv_fast):
    // two full rows in t0, then the two end columns of the rows in between; layers slowest
    const int e = L.sfaces[fy];
    b = e / 6; fdir = (e % 6) >> 1; side = e & 1;
    B = L.boxes[b];
    const int t0 = (fdir == 0) ? 1 : 0, t1 = (fdir == 2) ? 1 : 2;
    const unsigned n0 = B.hi[t0] - B.lo[t0] + 1, n1 = B.hi[t1] - B.lo[t1] + 1;
    const unsigned P = (n1 >= 2) ? 2 * n0 + 2 * (n1 - 2) : n0;
    if (t >= (long long)P * A.layers) return;
    unsigned r = (unsigned)t;
    layer = 0;
    while (r >= P) { r -= P; ++layer; }
    unsigned a0, a1;
    if (r < n0) { a0 = r; a1 = 0; }
    else if (r < 2 * n0) { a0 = r - n0; a1 = n1 - 1; }
    else { r -= 2 * n0; a0 = (r & 1u) ? n0 - 1 : 0; a1 = 1 + (r >> 1); }
    if (n0 == 1 && (r & 1u) && t >= 2 * (long long)n0) return;  // a single column: do not visit it twice
    q0[fdir] = side ? B.hi[fdir] + 1 : B.lo[fdir] - 1;
    q0[t0] = B.lo[t0] + (int)a0;
    q0[t1] = B.lo[t1] + (int)a1;
    if (layer >= B.hi[fdir] - B.lo[fdir] + 1) return;
    if ((L.sfcode[L.sfoff[fy] + a0 + (long long)n0 * a1] & 3u) == 0) return;
  } else {
    if (!sface_decode(L, fy, t, A.layers, b, B, fdir, side, q0, layer)) return;
    const int t0 = (fdir == 0) ? 1 : 0, t1 = (fdir == 2) ? 1 : 2;
    if (layer >= B.hi[fdir] - B.lo[fdir] + 1) return;
    if ((L.sfcode[L.sfoff[fy] + (t - (long long)layer * (B.hi[t0] - B.lo[t0] + 1) * (B.hi[t1] - B.lo[t1] + 1))] & 3u) == 0) return;
  }
  const int n[3] = {B.hi[0] - B.lo[0] + 1, B.hi[1] - B.lo[1] + 1, B.hi[2] - B.lo[2] + 1};
  int X[3] = {q0[0], q0[1], q0[2]};
  X[fdir] += side ? -(1 + layer) : (1 + layer);
  const ShellAcc Cs = {mf_view(MC_, B, b), ccomp};
  const CgAcc Cg = {&L, mf_view(MC_, B, b), B, b, ccomp, A.pmin, A.invd, cgz};
  const double dxinv[3] = {L.dxinv[0], L.dxinv[1], L.dxinv[2]};
  const double* o = MO.data + MO.off[b];
  auto C = [&](int i, int j, int k) -> double { return CG ? Cg(i, j, k) : Cs(i, j, k); };
  // component d of the (unclipped) normal at a valid cell p of this box
  auto nrm = [&](const int p[3], int d) -> double {
    if ((!CG || CGCLIP) && A.thr >= 0.0) {  // the sweep zeroed clipped normals in the output: the divergence needs the unclipped ones
      const double cp = C(p[0], p[1], p[2]);
      if (cp < A.thr || cp > 1.0 - A.thr) return comp_of(normal_at(C, p[0], p[1], p[2], dxinv), d);
    }
    return o[fab_index(B, MO.ng, MO.ncomp, ncomp0 + d, p[0], p[1], p[2])];
  };
  double curv = 0.0;
  bool ok = true;
  for (int d = 0; d < 3; ++d) {
    const double n0d = nrm(X, d);
    double nb[2];
    for (int s2 = 0; s2 < 2; ++s2) {
      const int sg = s2 ? 1 : -1;
      int q[3] = {X[0], X[1], X[2]};
      q[d] += sg;
      if (in_box(B, q)) { nb[s2] = nrm(q, d); continue; }
      // q is a ghost cell of face (d, s2) of this box: its masks are stored unless the face is ordinary
      unsigned code = 0;
      const int e2 = L.sfindex[b * 6 + d * 2 + s2];
      {
        const int u0 = (d == 0) ? 1 : 0, u1 = (d == 2) ? 1 : 2;
        if (e2 >= 0) code = L.sfcode[L.sfoff[e2] + (q[u0] - B.lo[u0]) + (long long)n[u0] * (q[u1] - B.lo[u1])];
      }
      const int cls = (int)(code & 3u);
      if (cls == 0) {
        nb[s2] = comp_of(normal_at(C, q[0], q[1], q[2], dxinv), d);
      } else if (cls == 2) {
        nb[s2] = (A.bc[d] == PA_BC_REFLECT_ODD) ? -n0d : n0d;
      } else {
        if (!A.has_crse) { ok = false; nb[s2] = 0.0; continue; }
        double coef[4];
        const int NX = cf_normal_coef(n[d], A.ratio, coef);
        const int xf[1] = {0};
        double bv1[1];
        const long long cpo = (Fx.use_cp && L.cp) ? L.cpoff[e2] : -1;  // that face's coarse patch holds component cncomp0 + d
        if (PATCH || cpo >= 0) cf_interp_patch<1>(code, cpz + cpo, B, s2, MN, q, d, xf, ok, bv1);
        else cf_interp<1>(code, LCr, MN, cncomp0 + d, q, d, A.ratio, xf, ok, bv1);
        const double bv = bv1[0];
        double tmp = 0.0;
        for (int m = 1; m < NX; ++m) {
          int pc[3] = {q[0], q[1], q[2]};
          pc[d] -= sg * m;  // into the box
          const double v = (m == 1) ? n0d : nrm(pc, d);
          tmp += v * coef[m];
        }
        double g = tmp;
        g += bv * coef[0];
        nb[s2] = g;
      }
    }
    curv += cdiff(dxinv[d], nb[0], n0d, nb[1]);
  }
  curv = curv * 0.5;
  if ((!CG || CGCLIP) && A.thr >= 0.0) {
    const double c0 = C(X[0], X[1], X[2]);
    if (c0 < A.thr || c0 > 1.0 - A.thr) curv = 0.0;
  }
  if (!ok) atomicAdd(nbad, 1);
  MO.data[MO.off[b] + fab_index(B, MO.ng, MO.ncomp, kcomp, X[0], X[1], X[2])] = curv;
}
template <bool CG, bool PATCH = false, bool CGCLIP = false>
__global__ __launch_bounds__(256, PA_FC_WAVES) void k_faces_curv(LevBatch<FixArgs> Bt, int* nbad, SlotK sk = SlotK()) {
  unsigned fy;
  const int perim = Bt.a[Bt.find(blockIdx.y, fy)].A.perim_only;
  faces_curv_cell<CG, PATCH, CGCLIP>(Bt, blockIdx.y, blockIdx.x * (long long)blockDim.x + threadIdx.x, perim, nbad, sk, (int)blockIdx.z);
}
// The perimeter cells through the levels' perimeter work tables (round 5): the grid of k_faces_curv is (longest perimeter of the
// batch / 256) x faces -- on a hierarchy whose faces differ in size (a 256^2 wall face next to the 32^2 .. 128^2 faces of a flame
// sheet) most workgroups find nothing to do: 333 -> 595 us when level 0 was re-tiled to 256^3 boxes.  One layer only.
template <bool CG, bool PATCH, bool CGCLIP>
__device__ __forceinline__ void faces_tab_wg(const LevBatch<FixArgs>& Bt, int* nbad, const SlotK& sk, unsigned w) {
  int blev = 0;
  while (blev + 1 < Bt.n && w >= (unsigned)Bt.a[blev].npwg) { w -= (unsigned)Bt.a[blev].npwg; ++blev; }
  if (w >= (unsigned)Bt.a[blev].npwg) return;
  const int2 it = Bt.a[blev].pwg[w];
  faces_curv_cell<CG, PATCH, CGCLIP>(Bt, (unsigned)Bt.ycum[blev] + (unsigned)it.x, (long long)it.y * 256 + threadIdx.x, 1, nbad, sk, (int)blockIdx.z);
}
template <bool CG, bool PATCH = false, bool CGCLIP = false>
__global__ __launch_bounds__(256, PA_FC_WAVES) void k_faces_curv_tab(LevBatch<FixArgs> Bt, int* nbad, SlotK sk = SlotK()) {
  faces_tab_wg<CG, PATCH, CGCLIP>(Bt, nbad, sk, blockIdx.x);
}
// the cells of SlowList through the general path (any cell of a face, one layer)
template <bool PATCH>
__global__ __launch_bounds__(256, PA_FC_WAVES) void k_faces_curv_list(LevBatch<FixArgs> Bt, int* nbad, SlowList sl, SlotK sk = SlotK()) {
  const int n = min(*sl.count, sl.cap);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int2 it = sl.items[i];  // x = batch row | slot << 24
    faces_curv_cell<true, PATCH, true>(Bt, (unsigned)it.x & 0xffffffu, it.y, 0, nbad, sk, (int)((unsigned)it.x >> 24));
  }
}

// Phase B, fast path: the interior cells of a special face (all four tangential neighbours inside the
// box), no threshold clip, boxes >= 3 cells thick.  One thread per face cell does BOTH layers: the
// normals it needs are plain loads from the output (exact after phase A), shared between the two
// layers, and only the ghost normal beyond the face needs the boundary condition.  Same operations in
// the same order as k_faces_curv (d = 0,1,2; cdiff; *0.5), which still handles the perimeter cells.
// CLIP (exact-normal pipeline with the threshold clip, curvature.cpp:549-570): the sweep wrote N = 0, K = 0 where the
// progress variable is outside [thr, 1 - thr].  A clipped cell keeps its K = 0; an unclipped one needs the UNCLIPPED normals
// of its neighbours: a stored component that is exactly 0.0 may be a clipped one -- then (and only then) the neighbour's
// progress variable is formed from phi and, if it is clipped, the cell is appended to SlowList and k_faces_curv_list
// recomputes it through the general path (normals from c: CgAcc, the same operations as the sweep's); inlining that
// recomputation here cost 2.4 KB of scratch per lane.  The coarse normal under a coarse-fine face is taken as stored =
// clipped (quirk Q2).
template <int FD, int NL, bool PATCH, bool CLIP = false>
__device__ __forceinline__ void faces_curv_fast_body(const DLevelView& L, const DLevelView& LCr, const DMFView& MN, int cncomp0, const DMFView& MO,
                                                     int ncomp0, int kcomp, const FaceArgs& A, int* nbad, int b, const DBox& B, int side,
                                                     const int q0[3], unsigned code, const double* patch, const DMFView& MP = DMFView(), int pcomp = 0, SlowList sl = SlowList(),
                                                     unsigned row = 0, long long tcell = 0, const double* ncgp = nullptr, long long ncgs = 0) {
  constexpr int T0 = (FD == 0) ? 1 : 0, T1 = (FD == 2) ? 1 : 2;
  const int cls = (int)(code & 3u);
  // cls == 0: a VALID ghost cell behind a special face (a face that is coarse-fine elsewhere; general BoxArrays).  The sweep's
  // ghost normals behind a special face are unusable (pa_fused_march3.h re-aims the stream they need at the compact array), so
  // the cell's curvature is formed here too, with the neighbour's FINAL normal read from the box that owns the ghost cell.
  // Exact-normal pipeline only (NL == 1: the normals are final once the sweeps are done); a ghost cell owned by another rank's
  // box is on the level's irregular list instead (k_find_irregular, k_curv_general rebuilds its normal).
  int sbn = -1, qw[3] = {0, 0, 0};
  if (cls == 0) {
    if (NL > 1) return;
    if (classify(L, q0[0], q0[1], q0[2], sbn, qw) != 0 || sbn < 0) return;
  }
  const int n[3] = {B.hi[0] - B.lo[0] + 1, B.hi[1] - B.lo[1] + 1, B.hi[2] - B.lo[2] + 1};
  const int sg = side ? 1 : -1;  // the ghost cell sits at X1 + sg e_FD
  int X1[3] = {q0[0], q0[1], q0[2]};
  X1[FD] -= sg;
  const long long nxo = n[0] + 2 * MO.ng, nyo = n[1] + 2 * MO.ng, nzo = n[2] + 2 * MO.ng;
  const long long cso = pa_cstride(nxo * nyo * nzo, MO.ncomp);
  const long long st[3] = {1, nxo, nxo * nyo};
  const long long idx1 = ((long long)(X1[2] - B.lo[2] + MO.ng) * nyo + (X1[1] - B.lo[1] + MO.ng)) * nxo + (X1[0] - B.lo[0] + MO.ng);
  const long long in = -sg * st[FD];
  double* o = MO.data + MO.off[b];
  const double* nf = o + (long long)(ncomp0 + FD) * cso + idx1;
  const double* n0p = o + (long long)(ncomp0 + T0) * cso + idx1;
  const double* n1p = o + (long long)(ncomp0 + T1) * cso + idx1;
  // NCG (x faces, one layer, no clip): N_x of the first three cells and the two tangential terms of K as the sweep formed them, from the
  // level's face-major arrays -- five contiguous streams instead of 8 bytes of five different lines
  const bool pre = FD == 0 && NL == 1 && !CLIP && ncgp != nullptr;
  double nfd1, nfd2, nfd3, a0m = 0, a0c = 0, a0p = 0, a1m = 0, a1c = 0, a1p = 0, t01n = 0, t11n = 0;
  if (pre) {  // three arrays of pairs: (N_x of the first, second cell), (N_x of the third cell, y term of K), (z term of K, -)
    const pa_fix_d2* np = (const pa_fix_d2*)ncgp;
    const pa_fix_d2 v0 = np[0], v1 = np[ncgs], v2 = np[2 * ncgs];
    nfd1 = v0.x; nfd2 = v0.y; nfd3 = v1.x; t01n = v1.y; t11n = v2.x;
  } else {
    nfd1 = nf[0]; nfd2 = nf[in]; nfd3 = nf[2 * in];
    a0m = n0p[-st[T0]]; a0c = n0p[0]; a0p = n0p[st[T0]];
    a1m = n1p[-st[T1]]; a1c = n1p[0]; a1p = n1p[st[T1]];
  }
  if (CLIP) {
    static_assert(!CLIP || NL == 1, "the clip-aware fast path fixes one layer");
    const FabView P = mf_view(MP, B, b);
    auto clipped = [&](int i, int j, int k) {
      const double c = (P(i, j, k, pcomp) - A.pmin) * A.invd;
      return c < A.thr || c > 1.0 - A.thr;
    };
    if (clipped(X1[0], X1[1], X1[2])) return;  // K = 0 from the sweep
    const int iv = -sg;  // one cell into the box along FD
    bool slow = false;   // a needed neighbour component that the sweep clipped: this cell goes through the general path
    if (cls == 0) {  // the neighbouring box's normal: clipped there if its progress variable (this FAB's ghost cell holds its phi) is
      const double gn = MO.data[MO.off[sbn] + fab_index(L.boxes[sbn], MO.ng, MO.ncomp, ncomp0 + FD, qw[0], qw[1], qw[2])];
      slow = gn == 0.0 && clipped(q0[0], q0[1], q0[2]);
    }
    slow = slow || (nfd2 == 0.0 && clipped(X1[0] + (FD == 0 ? iv : 0), X1[1] + (FD == 1 ? iv : 0), X1[2] + (FD == 2 ? iv : 0)));
    slow = slow || (nfd3 == 0.0 && clipped(X1[0] + (FD == 0 ? 2 * iv : 0), X1[1] + (FD == 1 ? 2 * iv : 0), X1[2] + (FD == 2 ? 2 * iv : 0)));
    slow = slow || (a0m == 0.0 && clipped(X1[0] - (T0 == 0), X1[1] - (T0 == 1), X1[2]));
    slow = slow || (a0p == 0.0 && clipped(X1[0] + (T0 == 0), X1[1] + (T0 == 1), X1[2]));
    slow = slow || (a1m == 0.0 && clipped(X1[0], X1[1] - (T1 == 1), X1[2] - (T1 == 2)));
    slow = slow || (a1p == 0.0 && clipped(X1[0], X1[1] + (T1 == 1), X1[2] + (T1 == 2)));
    if (slow && cls == 0) {  // k_curv_general<true> over the context's dynamic list: {box | batch level << 24 | slot << 27, cell}
      const int i = atomicAdd(sl.gcount, 1);
      if (i < sl.gcap) sl.gitems[i] = make_int4(b | (int)(sl.glev << 24) | (int)((row >> 24) << 27), X1[0], X1[1], X1[2]);
      else atomicAdd(nbad, 1);
      return;
    }
    if (slow) {
      const int i = atomicAdd(sl.count, 1);
      if (i < sl.cap) sl.items[i] = make_int2((int)row, (int)tcell);
      else atomicAdd(nbad, 1);
      return;
    }
  }
  double b0m = 0, b0c = 0, b0p = 0, b1m = 0, b1c = 0, b1p = 0;
  if (NL > 1) {
    b0m = n0p[in - st[T0]]; b0c = n0p[in]; b0p = n0p[in + st[T0]];
    b1m = n1p[in - st[T1]]; b1c = n1p[in]; b1p = n1p[in + st[T1]];
  }
  // ghost normal: MLMG applyBC on n_FD (curvature.cpp:510-531)
  double g;
  bool ok = true;
  if (cls == 0) {
    g = MO.data[MO.off[sbn] + fab_index(L.boxes[sbn], MO.ng, MO.ncomp, ncomp0 + FD, qw[0], qw[1], qw[2])];
  } else if (cls == 2) {
    g = (A.bc[FD] == PA_BC_REFLECT_ODD) ? -nfd1 : nfd1;
  } else {
    if (!A.has_crse) { ok = false; g = 0.0; }
    else {
      double coef[4];
      const int NX = cf_normal_coef(n[FD], A.ratio, coef);
      const int xf[1] = {0};
      double bv1[1];
      if (PATCH || patch) cf_interp_patch<1>(code, patch, B, side, MN, q0, FD, xf, ok, bv1);  // the face's coarse patch holds component cncomp0 + FD
      else cf_interp<1>(code, LCr, MN, cncomp0 + FD, q0, FD, A.ratio, xf, ok, bv1);
      double tmp = 0.0;
      for (int m = 1; m < NX; ++m) {
        const double v = (m == 1) ? nfd1 : (m == 2 ? nfd2 : nfd3);
        tmp += v * coef[m];
      }
      g = tmp;
      g += bv1[0] * coef[0];
    }
  }
  const double dx0 = L.dxinv[0], dx1 = L.dxinv[1], dx2 = L.dxinv[2];
  // face-normal terms: (minus neighbour, centre, plus neighbour)
  const double f1 = side ? cdiff(L.dxinv[FD], nfd2, nfd1, g) : cdiff(L.dxinv[FD], g, nfd1, nfd2);
  const double f2 = side ? cdiff(L.dxinv[FD], nfd3, nfd2, nfd1) : cdiff(L.dxinv[FD], nfd1, nfd2, nfd3);
  const double t01 = pre ? t01n : cdiff(L.dxinv[T0], a0m, a0c, a0p), t11 = pre ? t11n : cdiff(L.dxinv[T1], a1m, a1c, a1p);
  const double t02 = cdiff(L.dxinv[T0], b0m, b0c, b0p), t12 = cdiff(L.dxinv[T1], b1m, b1c, b1p);
  (void)dx0; (void)dx1; (void)dx2;
  double k1 = 0.0, k2 = 0.0;
  // d = 0, 1, 2 in order: the term of direction d is the face-normal one when d == FD, else T0's or T1's
  k1 += (FD == 0) ? f1 : t01;
  k1 += (FD == 1) ? f1 : (FD == 0 ? t01 : t11);
  k1 += (FD == 2) ? f1 : t11;
  k2 += (FD == 0) ? f2 : t02;
  k2 += (FD == 1) ? f2 : (FD == 0 ? t02 : t12);
  k2 += (FD == 2) ? f2 : t12;
  k1 = k1 * 0.5;
  k2 = k2 * 0.5;
  if (!ok) atomicAdd(nbad, 1);
  double* ko = o + (long long)kcomp * cso + idx1;
  ko[0] = k1;
  if (NL > 1) ko[in] = k2;
}

// PATCH: every coarse-fine face of every level of the batch has its coarse patch (the owner-map interpolation is not compiled in)
template <int NL, bool PATCH, bool CLIP>
__device__ __forceinline__ void faces_fast_cell(const LevBatch<FixArgs>& Bt, int* nbad, SlowList sl, const SlotK& sk, int blev, unsigned fy, long long t) {
  const FixArgs& Fx = Bt.a[blev];
  sl.glev = (unsigned)blev;
  const DLevelView& L = Fx.L;
  const DLevelView& LCr = Fx.LCr;
  const DMFView& MN = Fx.MN;
  const DMFView& MO = Fx.MO;
  const int z = (int)blockIdx.z;
  FaceArgs A = Fx.A;
  if (sk.prog) { A.pmin = sk.prog[2 * z]; A.invd = sk.prog[2 * z + 1]; }
  const int cncomp0 = Fx.cncomp0 + sk.cn_z * z, ncomp0 = Fx.ncomp0 + 8 * z, kcomp = Fx.kcomp + 8 * z;
  int b, fdir, side, layer, q0[3];
  DBox B;
  if (!sface_decode(L, fy, t, 1, b, B, fdir, side, q0, layer)) return;
  const int t0 = (fdir == 0) ? 1 : 0, t1 = (fdir == 2) ? 1 : 2;
  if (!(q0[t0] > B.lo[t0] && q0[t0] < B.hi[t0] && q0[t1] > B.lo[t1] && q0[t1] < B.hi[t1])) return;  // perimeter: k_faces_curv
  const unsigned code = L.sfcode[L.sfoff[fy] + t];
  const long long cpo = (Fx.use_cp && L.cp) ? L.cpoff[fy] : -1;  // wave-uniform
  const double* patch = cpo >= 0 ? L.cp + z * Fx.cp_stride + cpo : nullptr;
  const unsigned row = ((unsigned)Bt.ycum[blev] + fy) | ((unsigned)z << 24);  // batch row of the face; SlowList entries carry the slot
  const double* ncgp = nullptr;
  if (NL == 1 && !CLIP && fdir == 0 && Fx.ncg && z == 0 && ncg_face_ok(B, side, Fx.ncg_minw))
    ncgp = Fx.ncg + 2 * (L.cgoff[fy] + (long long)(q0[2] - B.lo[2] + 1) * (B.hi[1] - B.lo[1] + 3) + (q0[1] - B.lo[1] + 1));
  switch (fdir) {  // uniform per workgroup
    case 0: faces_curv_fast_body<0, NL, PATCH, CLIP>(L, LCr, MN, cncomp0, MO, ncomp0, kcomp, A, nbad, b, B, side, q0, code, patch, Fx.MC_, Fx.ccomp + z, sl, row, t, ncgp, Fx.ncgs); break;
    case 1: faces_curv_fast_body<1, NL, PATCH, CLIP>(L, LCr, MN, cncomp0, MO, ncomp0, kcomp, A, nbad, b, B, side, q0, code, patch, Fx.MC_, Fx.ccomp + z, sl, row, t); break;
    default: faces_curv_fast_body<2, NL, PATCH, CLIP>(L, LCr, MN, cncomp0, MO, ncomp0, kcomp, A, nbad, b, B, side, q0, code, patch, Fx.MC_, Fx.ccomp + z, sl, row, t); break;
  }
}
template <int NL, bool PATCH, bool CLIP>
__device__ __forceinline__ void faces_fast_wg(const LevBatch<FixArgs>& Bt, int* nbad, SlowList sl, const SlotK& sk, unsigned w) {
  unsigned fy;
  int blev;
  long long t;
  if (!wg_decode(Bt, blev, fy, t, w)) return;
  faces_fast_cell<NL, PATCH, CLIP>(Bt, nbad, sl, sk, blev, fy, t);
}

// ---- round 6: the face interiors from the levels' chunk records (see k_prep_faces_chunks below for the scheme): a thread takes the
// 2 x 2 block of first-layer cells whose ghost cells share one coarse parent.  Uniform chunks (all coarse-fine with the full
// stencil / all behind a wall) run straight-line code -- the parent's 3 x 3 coarse normals loaded once for the four cells, the
// tangential neighbours of a row or column of the block shared, interpolation weights as literals; per cell the operations and their
// order are faces_curv_fast_body<FD, 1, PATCH>'s with code PA_CODE_FULL (same bits).  Mixed chunks: faces_fast_cell per cell.
template <int FD>
__device__ __forceinline__ void fix_chunk_uniform(const FixArgs& Fx, const SfChunk& D, int z, int* nbad) {
  constexpr int T0 = (FD == 0) ? 1 : 0, T1 = (FD == 2) ? 1 : 2;
  const int side = D.dir_side & 1;
  const DMFView& MO = Fx.MO;
  const DLevelView& L = Fx.L;
  const int n[3] = {D.hi[0] - D.lo[0] + 1, D.hi[1] - D.lo[1] + 1, D.hi[2] - D.lo[2] + 1};
  const int n0 = n[T0], n1 = n[T1];
  const int hw = D.cw >> 1, sh = 31 - __builtin_clz((unsigned)hw);
  const int u = D.u0 + 2 * ((int)threadIdx.x & (hw - 1)), v = D.v0 + 2 * ((int)threadIdx.x >> sh);
  if (u >= n0 || v >= n1) return;
  const int ng = MO.ng, ncomp0 = Fx.ncomp0 + 8 * z, kcomp = Fx.kcomp + 8 * z;
  const long long nxo = n[0] + 2 * ng, nyo = n[1] + 2 * ng, nzo = n[2] + 2 * ng;
  const long long cso = pa_cstride(nxo * nyo * nzo, MO.ncomp);
  const long long st[3] = {1, nxo, nxo * nyo};
  int X1[3];
  X1[FD] = side ? D.hi[FD] : D.lo[FD];
  X1[T0] = D.lo[T0] + u;
  X1[T1] = D.lo[T1] + v;
  const long long idx1 = ((long long)(X1[2] - D.lo[2] + ng) * nyo + (X1[1] - D.lo[1] + ng)) * nxo + (X1[0] - D.lo[0] + ng);
  const long long in = side ? -st[FD] : st[FD], s0 = st[T0], s1 = st[T1];
  double* const o = MO.data + MO.off[D.box];
  const double* const nf = o + (long long)(ncomp0 + FD) * cso + idx1;
  const double* const n0p = o + (long long)(ncomp0 + T0) * cso + idx1;
  const double* const n1p = o + (long long)(ncomp0 + T1) * cso + idx1;
  double* const ko = o + (long long)kcomp * cso + idx1;
  DBox B;
#pragma unroll
  for (int d = 0; d < 3; ++d) { B.lo[d] = D.lo[d]; B.hi[d] = D.hi[d]; }
  const bool wall = (D.flags & PA_SFC_WALL) != 0;
  // NCG: this pass's sweep mirrored the first layer behind this x face (N_x of the first three cells, the y and z terms of K)
  const bool pre = FD == 0 && Fx.ncg && z == 0 && ncg_face_ok(B, side, Fx.ncg_minw);
  double nfd[2][2][3], A0[2][4], A1[2][4], t01n[2][2], t11n[2][2];
  // tangential neighbours: positions u - 1 .. u + 2 of each of the block's two rows (rows: v - 1 .. v + 2 of its two columns); a
  // position outside the face belongs to a perimeter cell, which is not written here -- clamped onto the face
  long long k0[4], k1o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    k0[k] = (long long)(min(max(u + k - 1, 0), n0 - 1) - u) * s0;
    k1o[k] = (long long)(min(max(v + k - 1, 0), n1 - 1) - v) * s1;
  }
  if (pre) {
    const pa_fix_d2* np = (const pa_fix_d2*)(Fx.ncg + 2 * (D.cgoff + (long long)(v + 1) * (n0 + 2) + (u + 1)));
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int du = 0; du < 2; ++du) {
        const pa_fix_d2 v0 = np[dv * (n0 + 2) + du], v1 = np[Fx.ncgs + dv * (n0 + 2) + du], v2 = np[2 * Fx.ncgs + dv * (n0 + 2) + du];
        nfd[dv][du][0] = v0.x; nfd[dv][du][1] = v0.y; nfd[dv][du][2] = v1.x; t01n[dv][du] = v1.y; t11n[dv][du] = v2.x;
      }
  } else {
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int du = 0; du < 2; ++du)
#pragma unroll
        for (int m = 0; m < 3; ++m) nfd[dv][du][m] = nf[dv * s1 + du * s0 + m * in];
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int k = 0; k < 4; ++k) A0[dv][k] = n0p[dv * s1 + k0[k]];
#pragma unroll
    for (int du = 0; du < 2; ++du)
#pragma unroll
      for (int k = 0; k < 4; ++k) A1[du][k] = n1p[du * s0 + k1o[k]];
  }
  double r[3][3];
  if (!wall) {
    int plane, pu0, pv0, pw, ph;
    cpatch_geom(B, FD, side, plane, pu0, pv0, pw, ph);
    const double* const cb = L.cp + z * Fx.cp_stride + D.cpoff + (long long)((X1[T1] >> 1) - pv0) * pw + ((X1[T0] >> 1) - pu0);
    bool ok = true;
#pragma unroll
    for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
      for (int a0 = 0; a0 < 3; ++a0) r[a1][a0] = cb[(a1 - 1) * pw + (a0 - 1)];
#pragma unroll
    for (int a1 = 0; a1 < 3; ++a1)
#pragma unroll
      for (int a0 = 0; a0 < 3; ++a0)
        if (__double_as_longlong(r[a1][a0]) == PA_CP_MISSING) { ok = false; r[a1][a0] = 0.0; }
    if (!ok) atomicAdd(nbad, ((int)(u > 0) + (int)(u + 1 < n0 - 1)) * ((int)(v > 0) + (int)(v + 1 < n1 - 1)));  // counted per face-interior cell of the block
  }
  const bool odd = Fx.A.bc[FD] == PA_BC_REFLECT_ODD;
  constexpr double nc0 = k_cf_coef.nrm[4][0], nc1 = k_cf_coef.nrm[4][1], nc2 = k_cf_coef.nrm[4][2], nc3 = k_cf_coef.nrm[4][3];
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du) {
      const double nfd1 = nfd[dv][du][0], nfd2 = nfd[dv][du][1], nfd3 = nfd[dv][du][2];
      double g;
      if (wall) {
        g = odd ? -nfd1 : nfd1;
      } else {
        const double c00 = du ? k_cf_coef.tan[1][1][1][0] : k_cf_coef.tan[0][1][1][0], c01 = du ? k_cf_coef.tan[1][1][1][1] : k_cf_coef.tan[0][1][1][1],
                     c02 = du ? k_cf_coef.tan[1][1][1][2] : k_cf_coef.tan[0][1][1][2];
        const double c10 = dv ? k_cf_coef.tan[1][1][1][0] : k_cf_coef.tan[0][1][1][0], c11 = dv ? k_cf_coef.tan[1][1][1][1] : k_cf_coef.tan[0][1][1][1],
                     c12 = dv ? k_cf_coef.tan[1][1][1][2] : k_cf_coef.tan[0][1][1][2];
        const double xi0 = du ? 0.25 : -0.25, xi1 = dv ? 0.25 : -0.25;
        double b0 = 0.0;
        b0 += c00 * r[1][0];
        b0 += c01 * r[1][1];
        b0 += c02 * r[1][2];
        b0 += c10 * r[0][1];
        b0 += c11 * r[1][1];
        b0 += c12 * r[2][1];
        b0 -= r[1][1];
        b0 += ((xi0 * xi1) * 0.25) * (((r[2][2] - r[2][0]) + r[0][0]) - r[0][2]);
        double tmp = 0.0;
        tmp += nfd1 * nc1;
        tmp += nfd2 * nc2;
        tmp += nfd3 * nc3;
        g = tmp;
        g += b0 * nc0;
      }
      const double f1 = side ? cdiff(L.dxinv[FD], nfd2, nfd1, g) : cdiff(L.dxinv[FD], g, nfd1, nfd2);
      const double t01 = pre ? t01n[dv][du] : cdiff(L.dxinv[T0], A0[dv][du], A0[dv][du + 1], A0[dv][du + 2]);
      const double t11 = pre ? t11n[dv][du] : cdiff(L.dxinv[T1], A1[du][dv], A1[du][dv + 1], A1[du][dv + 2]);
      double k1 = 0.0;
      k1 += (FD == 0) ? f1 : t01;
      k1 += (FD == 1) ? f1 : (FD == 0 ? t01 : t11);
      k1 += (FD == 2) ? f1 : t11;
      k1 = k1 * 0.5;
      const int uu = u + du, vv = v + dv;
      if (uu > 0 && uu < n0 - 1 && vv > 0 && vv < n1 - 1) ko[dv * s1 + du * s0] = k1;  // the perimeter is k_faces_curv_tab's
    }
}


// the face interiors of a chunk with any mix of cell kinds (see prep_chunk_mixed): the ghost normal of a first-layer cell is the
// boundary condition on n across a coarse-fine face, the mirror image behind a wall, or -- a valid ghost cell behind a partly
// covered face -- the neighbouring box's FINAL normal, read in the box that owns it (a branch, taken only by waves that have such
// cells; a ghost cell owned by another rank's box is on the level's irregular list: not written here)
template <int FD>
__device__ __forceinline__ void fix_chunk_mixed(const FixArgs& Fx, const SfChunk& D, int z, int* nbad, const double* tabs) {
  constexpr int T0 = (FD == 0) ? 1 : 0, T1 = (FD == 2) ? 1 : 2;
  const int side = D.dir_side & 1;
  const DMFView& MO = Fx.MO;
  const DLevelView& L = Fx.L;
  const int n[3] = {D.hi[0] - D.lo[0] + 1, D.hi[1] - D.lo[1] + 1, D.hi[2] - D.lo[2] + 1};
  const int n0 = n[T0], n1 = n[T1];
  const int hw = D.cw >> 1, sh = 31 - __builtin_clz((unsigned)hw);
  const int u = D.u0 + 2 * ((int)threadIdx.x & (hw - 1)), v = D.v0 + 2 * ((int)threadIdx.x >> sh);
  if (u >= n0 || v >= n1) return;
  const int ng = MO.ng, ncomp0 = Fx.ncomp0 + 8 * z, kcomp = Fx.kcomp + 8 * z;
  const long long nxo = n[0] + 2 * ng, nyo = n[1] + 2 * ng, nzo = n[2] + 2 * ng;
  const long long cso = pa_cstride(nxo * nyo * nzo, MO.ncomp);
  const long long st[3] = {1, nxo, nxo * nyo};
  int X1[3];
  X1[FD] = side ? D.hi[FD] : D.lo[FD];
  X1[T0] = D.lo[T0] + u;
  X1[T1] = D.lo[T1] + v;
  const long long idx1 = ((long long)(X1[2] - D.lo[2] + ng) * nyo + (X1[1] - D.lo[1] + ng)) * nxo + (X1[0] - D.lo[0] + ng);
  const long long in = side ? -st[FD] : st[FD], s0 = st[T0], s1 = st[T1];
  double* const o = MO.data + MO.off[D.box];
  const double* const nf = o + (long long)(ncomp0 + FD) * cso + idx1;
  const double* const n0p = o + (long long)(ncomp0 + T0) * cso + idx1;
  const double* const n1p = o + (long long)(ncomp0 + T1) * cso + idx1;
  double* const ko = o + (long long)kcomp * cso + idx1;
  DBox B;
#pragma unroll
  for (int d = 0; d < 3; ++d) { B.lo[d] = D.lo[d]; B.hi[d] = D.hi[d]; }
  const bool pre = FD == 0 && Fx.ncg && z == 0 && ncg_face_ok(B, side, Fx.ncg_minw);
  // only face-interior cells are written (the perimeter is k_faces_curv_tab's): every other cell of the block is folded onto the
  // nearest interior cell, so that all of its loads stay inside the FAB (faces at least three cells wide in both directions;
  // narrower ones have no interior cell)
  bool live[2][2];
  long long off[2][2], cgo[2][2];
  unsigned code[2][2];
  const int ulo = min(1, n0 - 1), uhi = max(n0 - 2, 0), vlo = min(1, n1 - 1), vhi = max(n1 - 2, 0);
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du) {
      const int uu = u + du, vv = v + dv;
      live[dv][du] = uu > 0 && uu < n0 - 1 && vv > 0 && vv < n1 - 1;
      const int uc = min(max(uu, ulo), uhi), vc = min(max(vv, vlo), vhi);
      off[dv][du] = (long long)(vc - v) * s1 + (long long)(uc - u) * s0;
      cgo[dv][du] = (long long)(vc + 1) * (n0 + 2) + (uc + 1);
      code[dv][du] = L.sfcode[D.sfoff + (long long)vc * n0 + uc];
    }
  if (n0 < 3 || n1 < 3) return;
  const bool cf_here = (D.flags & PA_SFC_HAS_CF) != 0;
  CfBlock K;
  if (cf_here) {
    int plane, pu0, pv0, pw, ph;
    cpatch_geom(B, FD, side, plane, pu0, pv0, pw, ph);
    cf_block_load(L.cp + z * Fx.cp_stride + D.cpoff + (long long)((X1[T1] >> 1) - pv0) * pw + ((X1[T0] >> 1) - pu0), pw, K);
  }
  double nfd[2][2][3], a0[2][2][3], a1[2][2][3], t01n[2][2], t11n[2][2];
  if (pre) {
    const pa_fix_d2* np = (const pa_fix_d2*)(Fx.ncg + 2 * D.cgoff);
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int du = 0; du < 2; ++du) {
        const pa_fix_d2 v0 = np[cgo[dv][du]], v1 = np[Fx.ncgs + cgo[dv][du]], v2 = np[2 * Fx.ncgs + cgo[dv][du]];
        nfd[dv][du][0] = v0.x; nfd[dv][du][1] = v0.y; nfd[dv][du][2] = v1.x; t01n[dv][du] = v1.y; t11n[dv][du] = v2.x;
      }
  } else {
#pragma unroll
    for (int dv = 0; dv < 2; ++dv)
#pragma unroll
      for (int du = 0; du < 2; ++du) {
#pragma unroll
        for (int m = 0; m < 3; ++m) nfd[dv][du][m] = nf[off[dv][du] + m * in];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          a0[dv][du][k] = n0p[off[dv][du] + (k - 1) * s0];
          a1[dv][du][k] = n1p[off[dv][du] + (k - 1) * s1];
        }
      }
  }
  if (cf_here) cf_block_finish(K);
  const bool odd = Fx.A.bc[FD] == PA_BC_REFLECT_ODD;
  constexpr double nc0 = k_cf_coef.nrm[4][0], nc1 = k_cf_coef.nrm[4][1], nc2 = k_cf_coef.nrm[4][2], nc3 = k_cf_coef.nrm[4][3];
  int nbad_here = 0;
#pragma unroll
  for (int dv = 0; dv < 2; ++dv)
#pragma unroll
    for (int du = 0; du < 2; ++du) {
      const unsigned cd = live[dv][du] ? code[dv][du] : 2u;
      const int cls = (int)(cd & 3u);
      const double nfd1 = nfd[dv][du][0], nfd2 = nfd[dv][du][1], nfd3 = nfd[dv][du][2];
      double g = odd ? -nfd1 : nfd1;  // wall
      bool write = live[dv][du];
      if (cf_here) {
        double b[1];
        const bool bad = cf_block_interp<1>(K, cd, du, dv, tabs, 0.0, 1.0, b);
        double tmp = 0.0;
        tmp += nfd1 * nc1;
        tmp += nfd2 * nc2;
        tmp += nfd3 * nc3;
        double h = tmp;
        h += b[0] * nc0;
        g = cls == 1 ? h : g;
        nbad_here += (cls == 1 && bad) ? 1 : 0;
      }
      if (cls == 0) {  // (rare) the ghost cell is a valid cell of a neighbouring box
        int q0[3] = {X1[0], X1[1], X1[2]};
        q0[FD] += side ? 1 : -1;
        q0[T0] += du;
        q0[T1] += dv;
        int sbn = -1, qw[3];
        if (classify(L, q0[0], q0[1], q0[2], sbn, qw) == 0 && sbn >= 0) g = MO.data[MO.off[sbn] + fab_index(L.boxes[sbn], MO.ng, MO.ncomp, ncomp0 + FD, qw[0], qw[1], qw[2])];
        else write = false;
      }
      const double f1 = side ? cdiff(L.dxinv[FD], nfd2, nfd1, g) : cdiff(L.dxinv[FD], g, nfd1, nfd2);
      const double t01 = pre ? t01n[dv][du] : cdiff(L.dxinv[T0], a0[dv][du][0], a0[dv][du][1], a0[dv][du][2]);
      const double t11 = pre ? t11n[dv][du] : cdiff(L.dxinv[T1], a1[dv][du][0], a1[dv][du][1], a1[dv][du][2]);
      double k1 = 0.0;
      k1 += (FD == 0) ? f1 : t01;
      k1 += (FD == 1) ? f1 : (FD == 0 ? t01 : t11);
      k1 += (FD == 2) ? f1 : t11;
      k1 = k1 * 0.5;
      if (write) ko[off[dv][du]] = k1;
    }
  if (nbad_here) atomicAdd(nbad, nbad_here);
}

// nperim > 0: the first nperim workgroups take the face PERIMETERS' work tables (faces_tab_wg: other cells, the same final normals, long
// chains of dependent loads -- in front, so that they run under the interiors instead of after them)
template <bool PATCH>
__global__ __launch_bounds__(256) void k_faces_fix_chunks(LevBatch<FixArgs> Bt, LevChunks Ck, int* nbad, SlotK sk, unsigned nperim) {
  if (blockIdx.x < nperim) { faces_tab_wg<true, PATCH, false>(Bt, nbad, sk, blockIdx.x); return; }
  const unsigned wx = blockIdx.x - nperim;
  int blev = 0;
  while (blev + 1 < Bt.n && wx >= Ck.w0[blev + 1]) ++blev;
  const FixArgs& Fx = Bt.a[blev];
  const SfChunk D = Ck.ck[blev][wx - Ck.w0[blev]];
  const int dir = D.dir_side >> 1;
  const int e0 = D.hi[0] - D.lo[0] + 1, e1 = D.hi[1] - D.lo[1] + 1, e2 = D.hi[2] - D.lo[2] + 1;
  const int blen = dir == 0 ? e0 : (dir == 1 ? e1 : e2), n0 = dir == 0 ? e1 : e0, n1 = dir == 2 ? e1 : e2;
  const bool cfok = Fx.A.has_crse && Fx.A.ratio == 2 && Fx.use_cp && Fx.L.cp && D.cpoff >= 0;
  const bool straight = blen >= 3 && ((D.flags & PA_SFC_WALL) != 0 || ((D.flags & PA_SFC_FULL) != 0 && cfok));
  const bool mixed = !straight && blen >= 3 && (cfok || !(D.flags & PA_SFC_HAS_CF));
  if (straight) {
    switch (dir) {  // (uniform)
      case 0: fix_chunk_uniform<0>(Fx, D, (int)blockIdx.z, nbad); break;
      case 1: fix_chunk_uniform<1>(Fx, D, (int)blockIdx.z, nbad); break;
      default: fix_chunk_uniform<2>(Fx, D, (int)blockIdx.z, nbad); break;
    }
    return;
  }
  if (mixed) {
    __shared__ double tabs[54];
    cf_tab_to_lds(tabs);
    switch (dir) {
      case 0: fix_chunk_mixed<0>(Fx, D, (int)blockIdx.z, nbad, tabs); break;
      case 1: fix_chunk_mixed<1>(Fx, D, (int)blockIdx.z, nbad, tabs); break;
      default: fix_chunk_mixed<2>(Fx, D, (int)blockIdx.z, nbad, tabs); break;
    }
    return;
  }
  const int hw = D.cw >> 1, sh = 31 - __builtin_clz((unsigned)hw);
  const int u = D.u0 + 2 * ((int)threadIdx.x & (hw - 1)), v = D.v0 + 2 * ((int)threadIdx.x >> sh);
  for (int dv = 0; dv < 2; ++dv)
    for (int du = 0; du < 2; ++du)
      if (u + du >= 0 && v + dv >= 0 && u + du < n0 && v + dv < n1) faces_fast_cell<1, PATCH, false>(Bt, nbad, SlowList(), sk, blev, (unsigned)D.face, (long long)(v + dv) * n0 + (u + du));
}

template <int NL, bool PATCH = false, bool CLIP = false>
__global__ __launch_bounds__(256) void k_faces_curv_fast(LevBatch<FixArgs> Bt, int* nbad, SlowList sl = SlowList(), SlotK sk = SlotK()) {
  faces_fast_wg<NL, PATCH, CLIP>(Bt, nbad, sl, sk, blockIdx.x);
}

// phase: 1 = recompute the layer-1 normals (k_faces_normal), 2 = curvature of layers 1-2 (needs phase 1 of this
// level AND of the coarser level), 3 = both
extern "C" int pa_gradcurv_faces_level(pa_ctx* ctx, const pa_mf* c, int ccomp, const pa_mf* crse_n, int cncomp0, const int32_t bc[3],
                                       int ratio, double thr, pa_mf* out, int ncomp0, int kcomp) {
  PaBind bind_(ctx);
  return pa_gradcurv_faces_phase(ctx, c, ccomp, crse_n, cncomp0, bc, ratio, thr, out, ncomp0, kcomp, 3);
}
int pa_gradcurv_faces_phase(pa_ctx* ctx, const pa_mf* c, int ccomp, const pa_mf* crse_n, int cncomp0, const int32_t bc[3], int ratio, double thr,
                            pa_mf* out, int ncomp0, int kcomp, int phase) {
  if (!ctx || !c || !out) return pa_fail(ctx, "pa_gradcurv_faces_level: null argument");
  if (c->lev != out->lev) return pa_fail(ctx, "pa_gradcurv_faces_level: different levels");
  if (c->ng < 2) return pa_fail(ctx, "pa_gradcurv_faces_level: c needs >= 2 ghost layers");
  if (ccomp >= c->ncomp || kcomp >= out->ncomp || ncomp0 + 3 > out->ncomp || (crse_n && cncomp0 + 3 > crse_n->ncomp))
    return pa_fail(ctx, "pa_gradcurv_faces_level: component range");
  if (crse_n && ratio != 2) return pa_fail(ctx, "pa_gradcurv_faces_level: only refinement ratio 2 is supported");
  const pa_level* L = c->lev;
  for (const DBox& B : L->boxes)
    for (int d = 0; d < 3; ++d)
      if (crse_n && B.hi[d] - B.lo[d] + 1 < 3) return pa_fail(ctx, "pa_gradcurv_faces_level: boxes thinner than 3 cells need the pass-by-pass path");
  // sharded coarse level: the three components of the coarse normal from this rank's coarse-source copy
  if (crse_n && (phase & 2) && pa_coarse_source(ctx, L, crse_n, cncomp0, 3, 0, 0, 0, &crse_n, &cncomp0)) return 1;
  FaceArgs A;
  for (int d = 0; d < 3; ++d) A.bc[d] = bc[d];
  A.ratio = ratio; A.has_crse = crse_n ? 1 : 0; A.thr = thr; A.layers = 2; A.perim_only = 0; A.pmin = 0.0; A.invd = 1.0;
  // fast path for the interior of the faces: no threshold clip, every box >= 3 cells thick
  bool fast = !(thr >= 0.0);
  for (const DBox& B : c->lev->boxes)
    for (int d = 0; d < 3; ++d) fast = fast && (B.hi[d] - B.lo[d] + 1 >= 3);
  if (L->sfaces.empty()) return 0;
  const long long n0 = L->maxn[0], n1 = L->maxn[1], n2 = L->maxn[2];
  const long long nf = std::max(n1 * n2, std::max(n0 * n2, n0 * n1));
  const unsigned nsf = (unsigned)L->sfaces.size();
  ProfScope prof(ctx, PA_TAG_GRADCURV_FACES);
  if (phase & 1) hipLaunchKernelGGL(k_faces_normal, dim3((unsigned)((nf + 255) / 256), nsf), dim3(256), 0, ctx->stream, L->view, c->view, ccomp, out->view, ncomp0, A);
  if (!(phase & 2)) {
    PA_HIP(hipGetLastError());
    return 0;
  }
  LevBatch<FixArgs> Bt;
  Bt.n = 1;
  Bt.ycum[1] = (int)nsf;
  Bt.a[0] = FixArgs{L->view, c->view, ccomp, crse_n ? crse_n->lev->view : L->view, crse_n ? crse_n->view : c->view, cncomp0, out->view, ncomp0, kcomp, A};
  Bt.a[0].wg = (const int2*)L->d_sfwg;
  Bt.a[0].nwg = L->nsfwg;
  if (fast) {
    hipLaunchKernelGGL(k_faces_curv_fast<2>, dim3((unsigned)L->nsfwg), dim3(256), 0, ctx->stream, Bt, ctx->d_flags);
    Bt.a[0].A.perim_only = 1;
  }
  const long long ncell = fast ? 2 * (std::max(n0, std::max(n1, n2)) + std::max(n0, std::max(n1, n2))) : nf;  // perimeter <= 4 * longest edge
  hipLaunchKernelGGL(k_faces_curv<false>, dim3((unsigned)((ncell * A.layers + 255) / 256), nsf), dim3(256), 0, ctx->stream, Bt, ctx->d_flags);
  PA_HIP(hipGetLastError());
  return 0;
}

// the context's lists of cells for k_faces_curv_list and (general BoxArrays) k_curv_general (grow-never: 1 M entries each);
// layout: [count, gcount, pad, pad][int2 x CAP][int4 x CAP]
static int pa_slow_list(pa_ctx* ctx, SlowList* sl) {
  constexpr int CAP = 1 << 20;
  if (!ctx->d_slow) {
    PA_HIP(hipMalloc(&ctx->d_slow, (sizeof(int2) + sizeof(int4)) * (size_t)CAP + 16));
  }
  sl->count = (int*)ctx->d_slow;
  sl->items = (int2*)((char*)ctx->d_slow + 16);
  sl->cap = CAP;
  sl->gcount = sl->count + 1;
  sl->gitems = (int4*)((char*)ctx->d_slow + 16 + sizeof(int2) * (size_t)CAP);
  sl->gcap = CAP;
  return 0;
}

// diagnostic (tests): how many cells the clip-aware fix-up of the LAST pass handed to its general path; -1: never used
extern "C" int pa_last_slow_cells(pa_ctx* ctx) {
  PaBind bind_(ctx);
  if (!ctx) return -1;
  if (!ctx->d_slow) return -1;
  int n = -1;
  if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipMemcpy(&n, ctx->d_slow, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return n;
}

// ===================================================================================== irregular cells (general BoxArrays)
// k_curv_general recomputes K of a level's irregular cells (pa_fused_irreg.hip says which cells those are and why) from the FINAL
// normals of the box and from normals of ghost cells rebuilt as their owner sees them (gen_c: valid cell -> phi of B's FAB, which
// FillBoundary(2) filled everywhere; otherwise the boundary condition of the direction Z - Y, MLMG applyBC / InterpBndryData as
// k_prep_faces) -- nothing in it depends on compact arrays, rings or stored masks.
struct GenLev {
  DLevelView L; DMFView MP; int pcomp;          // the level and its phi (2 ghost layers, FillBoundary done)
  DLevelView LCp; DMFView MCp; int cpcomp;      // coarse phi (or this rank's coarse-source copy of it)
  DLevelView LCn; DMFView MCn; int cncomp0;     // coarse flame normal (likewise)
  DMFView MO; int ncomp0, kcomp;
  FaceArgs A;
  const int4* items; int n;
  // dynamic list (filled by k_faces_curv_fast<CLIP> in this pass): the count lives on the device, an item's first word carries
  // box | batch level << 24 | slot << 27 and only the items of batch level `lev` are this launch's
  const int* ncount = nullptr; int lev = -1;
  int use_cp = 0; long long cp_stride = 0;  // the level's coarse patches hold the coarse normal component of each face's direction
};
struct GenBox {
  const DLevelView* L; const DLevelView* LCp; DMFView MCp; int cpcomp;
  DBox B; FabView P; int pcomp, has_crse, bc[3]; double pmin, invd;
  __device__ __forceinline__ double c_in(const int p[3]) const { return (P(p[0], p[1], p[2], pcomp) - pmin) * invd; }
};
// the progress variable at Z = Y + sg e_dir as the owner of the valid cell Y sees it (Y: a cell of the box or in the first ghost layer)
__device__ __noinline__ double gen_c(const GenBox& g, const int Y[3], int dir, int sg, bool& ok) {
  int Z[3] = {Y[0], Y[1], Y[2]};
  Z[dir] += sg;
  if (in_box(g.B, Z)) return g.c_in(Z);
  const int cls = classify(*g.L, Z[0], Z[1], Z[2]);
  if (cls == 0) return g.c_in(Z);
  if (cls == 2) {
    const double v = g.c_in(Y);
    return (g.bc[dir] == PA_BC_REFLECT_ODD) ? -v : v;
  }
  if (!g.has_crse) { ok = false; return 0.0; }
  int blen = 3;  // thickness of Y's box along dir (levels with boxes thinner than 3 cells do not take this pipeline)
  if (in_box(g.B, Y)) blen = g.B.hi[dir] - g.B.lo[dir] + 1;
  else {
    int sb, yw[3];
    if (classify(*g.L, Y[0], Y[1], Y[2], sb, yw) == 0 && sb >= 0) blen = g.L->boxes[sb].hi[dir] - g.L->boxes[sb].lo[dir] + 1;
  }
  double coef[4];
  const int NX = cf_normal_coef(blen, 2, coef);
  const double bv = cf_bndry_value(*g.L, *g.LCp, g.MCp, g.cpcomp, Z, dir, 2, ok);  // MCp carries the affine view of the coarse phi
  double tmp = 0.0;
  for (int m = 1; m < NX; ++m) {
    int pc[3] = {Z[0], Z[1], Z[2]};
    pc[dir] -= sg * m;
    tmp += g.c_in(pc) * coef[m];
  }
  double r = tmp;
  r += bv * coef[0];
  return r;
}
__device__ __noinline__ Vec3 gen_normal(const GenBox& g, const int Y[3], const double dxinv[3], bool& ok) {
  Vec3 n;
  const double cxm = gen_c(g, Y, 0, -1, ok), cxp = gen_c(g, Y, 0, 1, ok), cym = gen_c(g, Y, 1, -1, ok), cyp = gen_c(g, Y, 1, 1, ok);
  const double czm = gen_c(g, Y, 2, -1, ok), czp = gen_c(g, Y, 2, 1, ok);
  normal_from(cxm, cxp, cym, cyp, czm, g.c_in(Y), czp, dxinv, n.x, n.y, n.z);
  return n;
}

// the coarse-normal boundary value of the cell's own coarse-fine face (out of line: the common irregular cell has none)
__device__ __noinline__ double gen_crse_normal(const DLevelView& L, const DLevelView& LCn, const DMFView& MCn, int comp, const int q[3], int d, int ratio, bool& ok) {
  return cf_bndry_value(L, LCn, MCn, comp, q, d, ratio, ok);
}
// GEN: the code that rebuilds a ghost normal from the progress variable is compiled in (needed where the ghost cell's owner is
// another rank's box, or -- CLIP -- where the sweep zeroed a stored normal); PATCH: the coarse-fine boundary value of the
// cell's own face comes from the face's coarse patch (the owner-map interpolation is not compiled in).  The common case --
// one rank, no clip, patches on -- is <false, false, true>: a handful of loads per cell, no calls.
template <bool CLIP, bool GEN, bool PATCH>
__device__ __forceinline__ void curv_general_body(const GenLev& G, int* nbad, const SlotK& sk, const long long i0, const long long stride) {
  const DLevelView& L = G.L;
  const double dxinv[3] = {L.dxinv[0], L.dxinv[1], L.dxinv[2]};
  const long long ntot = G.ncount ? min(*G.ncount, G.n) : G.n;
  for (long long i = i0; i < ntot; i += stride) {  // (64-bit: i0 + stride must not wrap)
    const int4 it = G.items[i];
    int z = (int)blockIdx.z, b = it.x;
    if (G.lev >= 0) {
      if (((it.x >> 24) & 7) != G.lev) continue;
      z = (int)((unsigned)it.x >> 27);
      b = it.x & 0xffffff;
    }
    FaceArgs A = G.A;
    if (sk.prog) { A.pmin = sk.prog[2 * z]; A.invd = sk.prog[2 * z + 1]; }
    const int cncomp0 = G.cncomp0 + sk.cn_z * z, ncomp0 = G.ncomp0 + 8 * z, kcomp = G.kcomp + 8 * z;
    const int X[3] = {it.y, it.z, it.w};
    GenBox g;
    g.L = &G.L; g.LCp = &G.LCp; g.MCp = G.MCp; g.cpcomp = G.cpcomp + z;
    g.MCp.xform = 1; g.MCp.xa = A.pmin; g.MCp.xb = A.invd;
    g.B = L.boxes[b];
    g.P = mf_view(G.MP, g.B, b);
    g.pcomp = G.pcomp + z; g.has_crse = A.has_crse; g.pmin = A.pmin; g.invd = A.invd;
    for (int d = 0; d < 3; ++d) g.bc[d] = A.bc[d];
    const DBox& B = g.B;
    const int n[3] = {B.hi[0] - B.lo[0] + 1, B.hi[1] - B.lo[1] + 1, B.hi[2] - B.lo[2] + 1};
    double* o = G.MO.data + G.MO.off[b];
    bool ok = true;
    auto clipped = [&](const int p[3]) { const double c = g.c_in(p); return c < A.thr || c > 1.0 - A.thr; };
    double* kout = o + fab_index(B, G.MO.ng, G.MO.ncomp, kcomp, X[0], X[1], X[2]);
    if (CLIP && clipped(X)) { *kout = 0.0; continue; }
    // component d of the UNCLIPPED normal of cell p of this box (the sweep zeroed the clipped ones in the output)
    auto nrm = [&](const int p[3], int d) -> double {
      if (CLIP && GEN && clipped(p)) return comp_of(gen_normal(g, p, dxinv, ok), d);
      return o[fab_index(B, G.MO.ng, G.MO.ncomp, ncomp0 + d, p[0], p[1], p[2])];
    };
    double curv = 0.0;
    for (int d = 0; d < 3; ++d) {
      const double n0d = nrm(X, d);
      double nb[2];
      for (int s2 = 0; s2 < 2; ++s2) {
        const int sg = s2 ? 1 : -1;
        int q[3] = {X[0], X[1], X[2]};
        q[d] += sg;
        if (in_box(B, q)) { nb[s2] = nrm(q, d); continue; }
        int sb, qw[3];
        const int cls = classify(L, q[0], q[1], q[2], sb, qw);
        if (cls == 0) {
          // a valid cell of a neighbouring box: its FINAL normal from that box's output when the box is local (the sweeps of
          // the level are done), rebuilt from the progress variable as its owner sees it when it is another rank's
          if (sb >= 0) {
            const double v = G.MO.data[G.MO.off[sb] + fab_index(L.boxes[sb], G.MO.ng, G.MO.ncomp, ncomp0 + d, qw[0], qw[1], qw[2])];
            nb[s2] = (CLIP && GEN && v == 0.0 && clipped(q)) ? comp_of(gen_normal(g, q, dxinv, ok), d) : v;
          } else if (GEN) {
            nb[s2] = comp_of(gen_normal(g, q, dxinv, ok), d);
          } else {  // (cannot happen: the host compiles GEN in for sharded levels)
            ok = false; nb[s2] = 0.0;
          }
        } else if (cls == 2) {
          nb[s2] = (A.bc[d] == PA_BC_REFLECT_ODD) ? -n0d : n0d;
        } else {
          if (!A.has_crse) { ok = false; nb[s2] = 0.0; continue; }
          double coef[4];
          const int NX = cf_normal_coef(n[d], A.ratio, coef);
          // q is a ghost cell of face (d, s2) of this box, which is special: its masks are stored, its coarse patch holds component d
          double bv;
          const int e2 = L.sfindex[b * 6 + d * 2 + s2];
          const long long cpo = (G.use_cp && L.cp && e2 >= 0) ? L.cpoff[e2] : -1;
          if (e2 < 0 || ((PATCH || cpo >= 0) && (!L.cp || L.cpoff[e2] < 0))) {  // (cannot happen: a coarse-fine ghost cell makes its face special, with a patch)
            ok = false; bv = 0.0;
          } else if (PATCH || cpo >= 0) {
            const int u0 = (d == 0) ? 1 : 0, u1 = (d == 2) ? 1 : 2;
            const unsigned code = L.sfcode[L.sfoff[e2] + (q[u0] - B.lo[u0]) + (long long)n[u0] * (q[u1] - B.lo[u1])];
            const int xf[1] = {0};
            double bv1[1];
            cf_interp_patch<1>(code, L.cp + z * G.cp_stride + L.cpoff[e2], B, s2, G.MCn, q, d, xf, ok, bv1);
            bv = bv1[0];
          } else {
            bv = gen_crse_normal(L, G.LCn, G.MCn, cncomp0 + d, q, d, A.ratio, ok);
          }
          double tmp = 0.0;
          for (int m = 1; m < NX; ++m) {
            int pc[3] = {q[0], q[1], q[2]};
            pc[d] -= sg * m;  // into the box
            const double v = (m == 1) ? n0d : nrm(pc, d);
            tmp += v * coef[m];
          }
          double gv = tmp;
          gv += bv * coef[0];
          nb[s2] = gv;
        }
      }
      curv += cdiff(dxinv[d], nb[0], n0d, nb[1]);
    }
    curv = curv * 0.5;
    if (!ok) atomicAdd(nbad, 1);
    *kout = curv;
  }
}
template <bool CLIP, bool GEN = true, bool PATCH = false>
__global__ __launch_bounds__(256) void k_curv_general(GenLev G, int* nbad, SlotK sk) {
  curv_general_body<CLIP, GEN, PATCH>(G, nbad, sk, blockIdx.x * 256LL + threadIdx.x, gridDim.x * 256LL);
}
// the static lists of several levels in one launch: level l owns workgroups wg0[l] .. wg0[l+1]-1, 256 list items each
struct GenBatch { int n; unsigned wg0[PA_MAXB + 1]; GenLev a[PA_MAXB]; };
static_assert(sizeof(GenBatch) + sizeof(SlotK) + 16 <= 4000, "kernel arguments of k_curv_general_levels");
template <bool CLIP, bool GEN, bool PATCH>
__global__ __launch_bounds__(256) void k_curv_general_levels(GenBatch Bt, int* nbad, SlotK sk) {
  int l = 0;
  while (l + 1 < Bt.n && blockIdx.x >= Bt.wg0[l + 1]) ++l;
  const GenLev G = Bt.a[l];
  curv_general_body<CLIP, GEN, PATCH>(G, nbad, sk, (long long)(blockIdx.x - Bt.wg0[l]) * 256 + threadIdx.x, 1LL << 40);
}

// after the sweeps of ALL levels: curvature of the first layer behind every special face, several levels per launch pair.
// crse_n[l]: the coarser level's output (normal components from cncomp0) or this rank's coarse-source copy of them.
// nslots > 1: components pcomp .. pcomp + nslots - 1, slot z with outputs at ncomp0 + 8 z / kcomp + 8 z, coarse normals at
// cncomp0 + cn_z z, progress range prog[2 z], prog[2 z + 1] (device): one launch each (SlotK)
// crse_phi[l] (component cpcomp + slot): the coarse progress source behind level l's coarse-fine faces, as handed to
// pa_gradcurv_prep_levels -- the irregular cells of general BoxArrays rebuild ghost normals from it (k_curv_general)
int pa_gradcurv_fix_levels(pa_ctx* ctx, int nlev, pa_mf* const* phi, int pcomp, const pa_mf* const* crse_n, int cncomp0, const int32_t bc[3], double pmin, double pmax,
                           pa_mf* const* out, int ncomp0, int kcomp, double thr, int nslots, const double* prog, int cn_z, const pa_mf* const* crse_phi, int cpcomp) {
  SlotK sk;
  sk.prog = prog;
  sk.cn_z = cn_z;
  const bool use_cp = PA_USE_CPATCH;
  const bool clip = thr >= 0.0;
  auto gen_lev = [&](int l) {  // level l's arguments of k_curv_general
    const pa_level* L = phi[l]->lev;
    GenLev G;
    G.L = L->view; G.MP = phi[l]->view; G.pcomp = pcomp;
    const pa_mf* cp = crse_phi ? crse_phi[l] : nullptr;
    G.LCp = cp ? cp->lev->view : L->view; G.MCp = cp ? cp->view : phi[l]->view; G.cpcomp = cpcomp;
    G.LCn = crse_n[l] ? crse_n[l]->lev->view : L->view; G.MCn = crse_n[l] ? crse_n[l]->view : phi[l]->view; G.cncomp0 = cncomp0;
    G.MO = out[l]->view; G.ncomp0 = ncomp0; G.kcomp = kcomp;
    for (int d = 0; d < 3; ++d) G.A.bc[d] = bc[d];
    G.A.ratio = 2; G.A.has_crse = (crse_n[l] && cp) ? 1 : 0; G.A.thr = clip ? thr : -1.0; G.A.layers = 1; G.A.perim_only = 0; G.A.pmin = pmin; G.A.invd = 1.0 / (pmax - pmin);
    G.items = nullptr; G.n = 0;
    G.use_cp = (use_cp && crse_n[l] && L->cp_total > 0) ? 1 : 0;
    G.cp_stride = pa_cp_stride(L);
    return G;
  };
  for (int l0 = 0; l0 < nlev; l0 += PA_MAXB) {
    if (use_cp && pa_cpatch_launch(ctx, l0, std::min(nlev, l0 + PA_MAXB), phi, crse_n, cncomp0, 1, nslots, cn_z)) return 1;
    LevBatch<FixArgs> Bt;
    int blev[PA_MAXB];  // hierarchy level of every batch row
    for (int l = l0; l < nlev && l < l0 + PA_MAXB; ++l) {
      const pa_level* L = phi[l]->lev;
      if (L->boxes.empty() || L->sfaces.empty()) continue;
      blev[Bt.n] = l;
      FaceArgs A;
      for (int d = 0; d < 3; ++d) A.bc[d] = bc[d];
      A.ratio = 2; A.has_crse = crse_n[l] ? 1 : 0; A.thr = clip ? thr : -1.0; A.layers = 1; A.perim_only = 1; A.pmin = pmin; A.invd = 1.0 / (pmax - pmin);
      Bt.a[Bt.n] = FixArgs{L->view, phi[l]->view, pcomp, crse_n[l] ? crse_n[l]->lev->view : L->view, crse_n[l] ? crse_n[l]->view : phi[l]->view, cncomp0,
                           out[l]->view, ncomp0, kcomp, A, (use_cp && crse_n[l] && L->cp_total > 0) ? 1 : 0, pa_cg_stride(L), pa_cp_stride(L), (const int2*)L->d_sfwg, L->nsfwg, (const int2*)L->d_pfwg, L->npfwg};
      if (L->ncg_live) {  // this pass's sweep mirrored the first layer behind the special x faces
        if (!clip && nslots == 1) { Bt.a[Bt.n].ncg = L->d_ncg; Bt.a[Bt.n].ncgs = pa_cg_stride(L); Bt.a[Bt.n].ncg_minw = L->ncg_minw; }
        const_cast<pa_level*>(L)->ncg_live = false;
      }
      Bt.ycum[Bt.n + 1] = Bt.ycum[Bt.n] + (int)L->sfaces.size();
      ++Bt.n;
    }
    if (!Bt.n) continue;
    ProfScope prof(ctx, PA_TAG_GRADCURV_FACES);
    bool all_patch = true;  // every level of the batch that interpolates from a coarser level does so from patches
    for (int q = 0; q < Bt.n; ++q) all_patch = all_patch && (Bt.a[q].use_cp || !Bt.a[q].A.has_crse);
    if (Bt.ycum[Bt.n] >= (1 << 24)) return pa_fail(ctx, "pa_gradcurv_fix_levels: too many special faces in one batch");
    unsigned nwgf = 0;
    for (int q = 0; q < Bt.n; ++q) nwgf += (unsigned)Bt.a[q].nwg;
    const dim3 gfast(nwgf, 1, (unsigned)nslots);
    LevChunks Ck;  // the levels' chunk records (the face interiors without the clip: k_faces_fix_chunks)
    Ck.w0[0] = 0;
    unsigned npt = 0;  // the perimeters' work tables
    for (int q = 0; q < Bt.n; ++q) {
      const pa_level* Lq = phi[blev[q]]->lev;
      if (!Lq->d_sfchunk || Lq->nsfchunk <= 0 || !Bt.a[q].pwg || Bt.a[q].npwg <= 0) return pa_fail(ctx, "pa_gradcurv_fix_levels: a level without chunk records / perimeter tables");
      Ck.ck[q] = Lq->d_sfchunk;
      Ck.w0[q + 1] = Ck.w0[q] + (unsigned)Lq->nsfchunk;
      npt += (unsigned)Bt.a[q].npwg;
    }
    const dim3 gtab(npt, 1, (unsigned)nslots);
    if (clip) {
      SlowList sl;
      if (pa_slow_list(ctx, &sl)) return 1;
      PA_HIP(hipMemsetAsync(sl.count, 0, 2 * sizeof(int), ctx->stream));
      if (all_patch) hipLaunchKernelGGL((k_faces_curv_fast<1, true, true>), gfast, dim3(256), 0, ctx->stream, Bt, ctx->d_flags, sl, sk);
      else hipLaunchKernelGGL((k_faces_curv_fast<1, false, true>), gfast, dim3(256), 0, ctx->stream, Bt, ctx->d_flags, sl, sk);
      // the hand-over list is a few thousand cells through a long chain of dependent loads (~0.12 ms whatever its length): the
      // perimeter kernel (other cells, as latency bound) runs next to it on the side stream
      hipStream_t pst = ctx->stream;
      if (ctx->stream2 != ctx->stream) {
        if (!ctx->stream2) PA_HIP(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
        for (int e = 0; e < 2; ++e)
          if (!ctx->fix_evs[e]) PA_HIP(hipEventCreateWithFlags(&ctx->fix_evs[e], hipEventDisableTiming));
        pst = ctx->stream2;
        PA_HIP(hipEventRecord(ctx->fix_evs[0], ctx->stream));
        PA_HIP(hipStreamWaitEvent(pst, ctx->fix_evs[0], 0));
      }
      if (all_patch) hipLaunchKernelGGL((k_faces_curv_list<true>), dim3(1024), dim3(256), 0, ctx->stream, Bt, ctx->d_flags, sl, sk);
      else hipLaunchKernelGGL((k_faces_curv_list<false>), dim3(1024), dim3(256), 0, ctx->stream, Bt, ctx->d_flags, sl, sk);
      // general BoxArrays: cells with a valid ghost cell behind a special face whose neighbour's normal the sweep clipped
      for (int q = 0; q < Bt.n; ++q) {
        if (phi[blev[q]]->lev->pure_faces) continue;  // no such cells on this level
        GenLev G = gen_lev(blev[q]);
        G.items = sl.gitems; G.n = sl.gcap; G.ncount = sl.gcount; G.lev = q;
        hipLaunchKernelGGL(k_curv_general<true>, dim3(256), dim3(256), 0, ctx->stream, G, ctx->d_flags, sk);
      }
      if (all_patch) hipLaunchKernelGGL((k_faces_curv_tab<true, true, true>), gtab, dim3(256), 0, pst, Bt, ctx->d_flags, sk);
      else hipLaunchKernelGGL((k_faces_curv_tab<true, false, true>), gtab, dim3(256), 0, pst, Bt, ctx->d_flags, sk);
      if (pst != ctx->stream) {
        PA_HIP(hipEventRecord(ctx->fix_evs[1], pst));
        PA_HIP(hipStreamWaitEvent(ctx->stream, ctx->fix_evs[1], 0));
      }
    } else {
      // The face interiors from the chunk records, the perimeters' work tables IN FRONT of them in the same launch when they are few next
      // to the interiors (large faces: headline 5.906 -> 5.870 ms per pass) or on a rank's share of a sharded hierarchy (two short
      // chains, always together); the many short perimeters of small faces run better as their own launch with their own register
      // budget (irregular hierarchy: 6.50 against 6.60 ms merged).  (The perimeter kernel on a side stream next to the interiors was
      // measured twice and bought nothing: DESIGN_HISTORY.md R2, R4.)
      const bool sharded = nlev > 0 && phi[0]->lev->nranks > 1;
      const bool with_perim = sharded || npt * 8u <= Ck.w0[Bt.n];
      const unsigned np = with_perim ? npt : 0u;
      const dim3 gc(np + Ck.w0[Bt.n], 1, (unsigned)nslots);
      if (all_patch) hipLaunchKernelGGL((k_faces_fix_chunks<true>), gc, dim3(256), 0, ctx->stream, Bt, Ck, ctx->d_flags, sk, np);
      else hipLaunchKernelGGL((k_faces_fix_chunks<false>), gc, dim3(256), 0, ctx->stream, Bt, Ck, ctx->d_flags, sk, np);
      if (!with_perim) {
        if (all_patch) hipLaunchKernelGGL((k_faces_curv_tab<true, true>), gtab, dim3(256), 0, ctx->stream, Bt, ctx->d_flags, sk);
        else hipLaunchKernelGGL((k_faces_curv_tab<true, false>), gtab, dim3(256), 0, ctx->stream, Bt, ctx->d_flags, sk);
      }
    }
  }
  // general BoxArrays: the listed irregular cells, after (and over) whatever the kernels above wrote there; the lists of up to
  // PA_MAXB levels in one launch
  {
    const int phi_nranks = nlev > 0 ? phi[0]->lev->nranks : 1;
    GenBatch Gb;
    Gb.n = 0;
    Gb.wg0[0] = 0;
    auto flush = [&]() {
      if (!Gb.n) return;
      ProfScope prof(ctx, PA_TAG_GRADCURV_FACES);
      const dim3 gg(Gb.wg0[Gb.n], 1, (unsigned)nslots);
      bool light = !clip, patch = true;  // one rank, no clip, every coarse-fine face has its patch: the small variant
      for (int q = 0; q < Gb.n; ++q) {
        light = light && Gb.a[q].L.nboxes > 0 && phi_nranks == 1;
        patch = patch && (Gb.a[q].use_cp || !Gb.a[q].A.has_crse);
      }
      if (light && patch) hipLaunchKernelGGL((k_curv_general_levels<false, false, true>), gg, dim3(256), 0, ctx->stream, Gb, ctx->d_flags, sk);
      else if (clip) hipLaunchKernelGGL((k_curv_general_levels<true, true, false>), gg, dim3(256), 0, ctx->stream, Gb, ctx->d_flags, sk);
      else hipLaunchKernelGGL((k_curv_general_levels<false, true, false>), gg, dim3(256), 0, ctx->stream, Gb, ctx->d_flags, sk);
      Gb.n = 0;
    };
    for (int l = 0; l < nlev; ++l) {
      const pa_level* L = phi[l]->lev;
      if (L->boxes.empty()) continue;
      if (pa_level_irregular(ctx, L)) return 1;
      if (L->nirr == 0) continue;
      GenLev G = gen_lev(l);
      G.items = (const int4*)L->d_irr; G.n = L->nirr;
      Gb.a[Gb.n] = G;
      Gb.wg0[Gb.n + 1] = Gb.wg0[Gb.n] + (unsigned)((L->nirr + 255) / 256);
      if (++Gb.n == PA_MAXB) flush();
    }
    flush();
  }
  PA_HIP(hipGetLastError());
  return 0;
}
