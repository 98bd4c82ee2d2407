// pa_fused.h -- what the translation units of the fused grad -> curvature path share, and nothing else.
//
// Included only by pa_fused_sweep.hip (the sweep launchers), pa_fused_prep.hip (ghost preparation of the exact-normal pipeline),
// pa_fused_fix.hip (the curvature fix-up of both pipelines) and pa_fused_irreg.hip (irregular cells, Gaussian-curvature fix-up).
// The entry points the level loops call (pa_pipeline.hip) are declared in pa_internal.h; types and helpers that one unit alone
// uses stay in that unit.  Every type here is at global scope and appears in kernel signatures: a type local to one unit must not
// reuse one of these names, nor the name of a local type of another unit.
#pragma once
#include "pa_internal.h"
#include <algorithm>

// Component slots: the boundary kernels of the exact-normal pipeline run for several components in ONE launch, blockIdx.z =
// slot z: phi component + z, output components + 8 z, coarse-normal components + cn_z z, the slot's own set of compact ghost
// arrays and coarse patches, its own progress-variable range prog[2 z], prog[2 z + 1] = (pmin, 1 / (pmax - pmin)) (null: the
// one in the level arguments).  One launch over 16 components costs little more than over one: at the size of a level's
// special faces these kernels are latency bound (pa_gradcurv_run_comps2).
struct SlotK { const double* prog = nullptr; int cn_z = 8; };

struct LevChunks { const SfChunk* ck[PA_MAXB]; unsigned w0[PA_MAXB + 1]; };  // level l of the batch owns workgroups w0[l] .. w0[l + 1] - 1

// ---- round 6: the coarse-fine interpolation of the four ghost cells of a 2 x 2 block for ANY mix of codes, without branches.  The
// block's cells share the coarse parent qc; InterpBndryData reaches at most two coarse cells along each tangential axis and the
// four diagonal neighbours, so 13 values of the face's coarse patch are a superset of what the four cells read (always inside the
// patch: it covers coarsen(lo - 1) - 2 .. coarsen(hi + 1) + 2).  Per cell: the stencil extents come out of its code, the weights
// out of a copy of g_cf_coef.tan in LDS, the values out of the superset by selects, and a term outside the cell's stencil is
// SKIPPED by a select (not multiplied by zero) -- the additions that happen are cf_interp_core's, in its order.
struct CfBlock {
  double ax0[5], ax1[5], dg[4];  // coarse(qc + a e_t0), coarse(qc + a e_t1) for a = -2 .. 2; diagonals (+,+) (-,+) (-,-) (+,-)
  unsigned miss;                 // bit i: ax0[i]; bit 5 + i: ax1[i]; bit 10 + i: dg[i] has no coarse owner (zeroed here, as craw does)
};
__device__ __forceinline__ void cf_block_load(const double* cb, int pw, CfBlock& K) {
#pragma unroll
  for (int a = 0; a < 5; ++a) K.ax0[a] = cb[a - 2];
#pragma unroll
  for (int a = 0; a < 5; ++a) K.ax1[a] = (a == 2) ? 0.0 : cb[(long long)(a - 2) * pw];
  K.dg[0] = cb[pw + 1]; K.dg[1] = cb[pw - 1]; K.dg[2] = cb[-pw - 1]; K.dg[3] = cb[-pw + 1];
}
__device__ __forceinline__ void cf_block_finish(CfBlock& K) {  // after the loads have been issued with everything else
  K.ax1[2] = K.ax0[2];
  K.miss = 0;
#pragma unroll
  for (int a = 0; a < 5; ++a) {
    if (__double_as_longlong(K.ax0[a]) == PA_CP_MISSING) { K.miss |= 1u << a; K.ax0[a] = 0.0; }
    if (__double_as_longlong(K.ax1[a]) == PA_CP_MISSING) { K.miss |= 1u << (5 + a); K.ax1[a] = 0.0; }
  }
#pragma unroll
  for (int a = 0; a < 4; ++a)
    if (__double_as_longlong(K.dg[a]) == PA_CP_MISSING) { K.miss |= 1u << (10 + a); K.dg[a] = 0.0; }
}
__device__ __forceinline__ void cf_tab_to_lds(double* tabs) {  // g_cf_coef.tan, flat: ((rem * 3 + lo + 2) * 3 + hi) * 3 + m
  if (threadIdx.x < 54) tabs[threadIdx.x] = (&g_cf_coef.tan[0][0][0][0])[threadIdx.x];
  __syncthreads();
}
// child (du, dv) of the parent, masks `code` (class 1); field 0 sees the raw coarse values, field 1 (NF == 2) (v - xa) * xb.
// Returns true when the cell's stencil touches a coarse cell without an owner.
// one tangential direction of cf_block_interp: the (up to three) stencil points lo .. hi out of the five axis values e0 .. e4 = coarse(qc + a e_t),
// a = -2 .. 2 (by value: a pointer chosen by the direction would keep the block in memory and turn the selects into an indexed load)
template <int NF>
__device__ __forceinline__ unsigned cf_block_axis(unsigned fld, int rem, const double* tabs, double e0, double e1, double e2, double e3, double e4, double xa, double xb, double b[NF]) {
  const int lo2 = (int)(fld & 3u), hi = (int)((fld >> 2) & 3u);  // lo2 = lo + 2
  const int N = hi - (lo2 - 2) + 1;
  const double* ct = tabs + ((rem * 3 + lo2) * 3 + hi) * 3;
  const double c0 = ct[0], c1 = ct[1], c2 = ct[2];
  const double v0 = lo2 == 0 ? e0 : (lo2 == 1 ? e1 : e2), v1 = lo2 == 0 ? e1 : (lo2 == 1 ? e2 : e3), v2 = lo2 == 0 ? e2 : (lo2 == 1 ? e3 : e4);
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const double w0 = f ? (v0 - xa) * xb : v0, w1 = f ? (v1 - xa) * xb : v1, w2 = f ? (v2 - xa) * xb : v2;
    b[f] += c0 * w0;
    const double s1 = b[f] + c1 * w1;
    b[f] = N > 1 ? s1 : b[f];
    const double s2 = b[f] + c2 * w2;
    b[f] = N > 2 ? s2 : b[f];
  }
  return ((1u << (hi + 3)) - 1u) & ~((1u << lo2) - 1u);  // the axis values the stencil uses
}
// child (du, dv) of the parent, masks `code` (class 1); field 0 sees the raw coarse values, field 1 (NF == 2) (v - xa) * xb.
// Returns true when the cell's stencil touches a coarse cell without an owner.
template <int NF>
__device__ __forceinline__ bool cf_block_interp(const CfBlock& K, unsigned code, int du, int dv, const double* tabs, double xa, double xb, double b[NF]) {
#pragma unroll
  for (int f = 0; f < NF; ++f) b[f] = 0.0;
  unsigned used = cf_block_axis<NF>((code >> 2) & 15u, du, tabs, K.ax0[0], K.ax0[1], K.ax0[2], K.ax0[3], K.ax0[4], xa, xb, b);
  used |= cf_block_axis<NF>((code >> 6) & 15u, dv, tabs, K.ax1[0], K.ax1[1], K.ax1[2], K.ax1[3], K.ax1[4], xa, xb, b) << 5;
  const bool cross = (code & (1u << 10)) != 0;
  used |= cross ? (0xFu << 10) : 0u;
  const double xi0 = du ? 0.25 : -0.25, xi1 = dv ? 0.25 : -0.25;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const double ce = f ? (K.ax0[2] - xa) * xb : K.ax0[2];
    b[f] -= ce;
    const double vpp = f ? (K.dg[0] - xa) * xb : K.dg[0], vmp = f ? (K.dg[1] - xa) * xb : K.dg[1];
    const double vmm = f ? (K.dg[2] - xa) * xb : K.dg[2], vpm = f ? (K.dg[3] - xa) * xb : K.dg[3];
    const double sc = b[f] + ((xi0 * xi1) * 0.25) * (((vpp - vmp) + vmm) - vpm);
    b[f] = cross ? sc : b[f];
  }
  return (K.miss & used) != 0;
}

// ---- host helpers that cross the units
// every level of the fused path gathers coarse patches (the face kernels' owner-map interpolation is what levels without patches --
// none today -- would take)
constexpr bool PA_USE_CPATCH = true;
// the level's compact ghost arrays, allocated on first use (pa_fused_prep.hip); doubles between the component slots' sets
int pa_level_cg(pa_ctx* ctx, const pa_level* L, int nsets = 1);
inline long long pa_cg_stride(const pa_level* L) { return std::max<long long>(L->cg_total, 8); }
inline long long pa_cp_stride(const pa_level* L) { return std::max<long long>(L->cp_total, 8); }
// gather the coarse patches of levels [l0, l1) (those that have a coarse source): one launch (pa_fused_prep.hip)
int pa_cpatch_launch(pa_ctx* ctx, int l0, int l1, pa_mf* const* fine, const pa_mf* const* crse, int ccomp, int by_dir, int nslots = 1, int zstride = 1);
// the level's list of irregular cells, built on first use (pa_fused_irreg.hip)
int pa_level_irregular(pa_ctx* ctx, const pa_level* L);
