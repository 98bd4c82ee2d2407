// pa_celltiles.h -- the walk of the fixed-point scatter kernels (pa_stats.hip: jpdf, conditionalMean; pa_integral.hip: integral, rmsVel;
// DESIGN.md 3.7 / 3.8).  A level is cut into TILES: 256 cells of a plane (x, aax) of one box -- lane = x, coalesced loads -- times kt
// cells along the march axis.  Persistent workgroups take tiles t = blockIdx.x, + gridDim.x, ..; a thread marches m0 .. m1 and keeps
// private runs.  Here: the tile table and its decode (tests/test_celltiles_host.py: every valid cell exactly once), "covered by the
// finer level", the workgroup's LDS table into the global one, and the host checks of the family.  NOT here: the address of a tile's
// first cell.  Every helper tried for it (FabView::idx of mf_view, or the same arithmetic in a function) changed the register
// allocation of the kernels around it; the three kernels keep the arithmetic in place.
#pragma once
#include "pa_internal.h"
#include "pa_fixed192.h"
#include <cmath>
#include <string>
#include <vector>

struct CellTile {
  int b, i, a, m0, m1;  // box, x, index along aax, first and last index along march
  DBox B;
  bool ok;              // false: the thread has no cell in this piece of the plane (m0 .. m1 are those of the whole workgroup all the same)
};
// The tile table and the walk travel in the kernel arguments as two plain structs, so that a kernel can keep them where its
// arguments had them: k_integral's scalar registers are allocated by the order of its arguments, and moving these fields cost its
// 8-variable form 1.5 %.
struct CellTab {
  const int* cum;  // [nboxes + 1] tiles before box b
  int nboxes, ntiles;
};
struct CellWalk { int march, aax, kt; };
// the walk of a kernel that has one only: as runtime values the box and cell indexing of k_jpdf and k_condmean goes through scratch
// and LDS and costs them a wave per SIMD
template <int AAX, int MARCH, int KT>
struct CellWalkFixed { static constexpr int aax = AAX, march = MARCH, kt = KT; };
// tile t as thread tid of the workgroup sees it
template <class W>
__host__ __device__ __forceinline__ CellTile celltile_decode(const CellTab& T, const W& w, const DBox* boxes, int t, unsigned tid) {
  CellTile c;
  int lo = 0, hi = T.nboxes - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.cum[mid] <= t) lo = mid; else hi = mid - 1;
  }
  c.b = lo;
  c.B = boxes[lo];
  const unsigned local = (unsigned)(t - T.cum[lo]);
  const unsigned nx = c.B.hi[0] - c.B.lo[0] + 1, na = c.B.hi[w.aax] - c.B.lo[w.aax] + 1;
  const unsigned npl = (nx * na + 255u) / 256u;
  const unsigned mt = local / npl, pt = local - mt * npl;
  const unsigned p = pt * 256u + tid;
  c.ok = p < nx * na;
  const unsigned aa = p / nx;
  c.a = c.B.lo[w.aax] + (int)aa;
  c.i = c.B.lo[0] + (int)(p - aa * nx);
  c.m0 = c.B.lo[w.march] + (int)(mt * (unsigned)w.kt);
  c.m1 = c.m0 + w.kt - 1;
  if (c.m1 > c.B.hi[w.march]) c.m1 = c.B.hi[w.march];
  return c;
}
// the thread's cell at step m of the march
template <class W>
__host__ __device__ __forceinline__ void celltile_cell(const W& w, const CellTile& c, int m, int idx[3]) {
  idx[0] = c.i;
  idx[w.aax] = c.a;
  idx[w.march] = m;
}

// cum[b] = tiles before box b, cum[nb] = all of them.  0, or which limit a level breaks: 1 a plane of 2^31 - 256 cells, 2 2^31 tiles
inline int celltiles_count(const DBox* boxes, int nb, int aax, int march, int kt, std::vector<int>& cum) {
  cum.assign(nb + 1, 0);
  long long tot = 0;
  for (int b = 0; b < nb; ++b) {
    const DBox& B = boxes[b];
    const long long nx = B.hi[0] - B.lo[0] + 1, na = B.hi[aax] - B.lo[aax] + 1, nm = B.hi[march] - B.lo[march] + 1;
    if (nx * na >= (1LL << 31) - 256) return 1;
    cum[b] = (int)tot;
    tot += ((nx * na + 255) / 256) * ((nm + kt - 1) / kt);
    if (tot >= (1LL << 31)) return 2;
  }
  cum[nb] = (int)tot;
  return 0;
}

// the tile table of the level being added, on the device (grow-only) and its host staging
struct CellTileTable {
  int* d_cum = nullptr;
  size_t cap = 0;
  std::vector<int> h_cum;
  int build(pa_ctx* ctx, const pa_level* lev, int aax, int march, int kt, const char* who, CellTab& T) {
    const int nb = (int)lev->boxes.size();
    const int bad = celltiles_count(lev->boxes.data(), nb, aax, march, kt, h_cum);
    if (bad) return pa_fail(ctx, std::string(who) + (bad == 1 ? ": FAB too large" : ": level too large for one call"));
    if (cap < (size_t)nb + 1) {
      PA_HIP(hipStreamSynchronize(ctx->stream));  // the previous table may still be read by a launch in flight
      release();
      PA_HIP(hipMalloc((void**)&d_cum, ((size_t)nb + 1) * sizeof(int)));
      cap = (size_t)nb + 1;
    }
    PA_HIP(hipMemcpyAsync(d_cum, h_cum.data(), ((size_t)nb + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(hipStreamSynchronize(ctx->stream));  // h_cum is reused by the next call
    T = {d_cum, nb, h_cum[nb]};
    return 0;
  }
  void release() {
    if (d_cum) (void)hipFree(d_cum);
    d_cum = nullptr;
    cap = 0;
  }
};

// "the cell's refined image has an owner on the next finer level" (jpdf.cpp:373-387, conditionalMean.cpp:246-258, integral.cpp:425-436)
__device__ __forceinline__ bool covered_by(const DLevelView& F, int ratio, int i, int j, int k) {
  const int p[3] = {i * ratio, j * ratio, k * ratio};
  return owner_of(F, p) != -1;
}
// the kernel arguments of that test: F is the level itself where there is no finer one (never read then)
inline void fine_cover(const pa_level* lev, const pa_level* finer, int ratio, DLevelView& F, int& has_fine, int& aratio) {
  F = finer ? finer->view : lev->view;
  has_fine = finer ? 1 : 0;
  aratio = ratio;
}

// The workgroup's table in LDS into the global one of the same layout -- per slot `stride` words: the count, then 3 limbs per row
// 1 .. nrows - 1 -- with one add per touched slot and row.  also(e, g) runs once per touched slot (LDS entry e, global entry g), with
// the add of the count, for what a kernel keeps behind the rows (conditionalMean's minima and maxima).  Every thread of the
// workgroup calls this after its last run went to LDS.
template <class F>
__device__ __forceinline__ void celltab_merge(const u64* lds, u64* glob, int nslots, int nrows, int stride, F also) {
  __syncthreads();
  const int ne = nslots * nrows;
  for (int z = threadIdx.x; z < ne; z += 256) {
    const int sl = z / nrows, r = z - sl * nrows;
    const u64* e = lds + (long long)sl * stride;
    u64* g = glob + (long long)sl * stride;
    if (e[0] == 0) continue;  // no cell of this workgroup in the slot
    if (r == 0) {
      atomicAdd(g, e[0]);
      also(e, g);
    } else {
      const int o = 1 + 3 * (r - 1);
      const U192 v = {{e[o], e[o + 1], e[o + 2]}};
      if (!u192_zero(v)) u192_atomic_add(g + o, v);
    }
  }
}

// ---------------------------------------------------------------- host checks
// pa_*_begin: the declared magnitudes of the n `what`s
inline int check_magnitudes(pa_ctx* ctx, const char* who, const char* what, const double* vabs, int n) {
  for (int v = 0; v < n; ++v)
    if (!(vabs[v] >= 0.0) || !std::isfinite(vabs[v])) return pa_fail(ctx, std::string(who) + ": magnitude of " + what + " " + std::to_string(v) + " is not finite");
  return 0;
}
// pa_*_read: the sticky PA_ST_* flags of the accumulator (k_integral can only set PA_ST_OVERFLOW: int_term keeps what is not finite away
// from to_fixed, and it has no bins)
inline int check_sum_flags(pa_ctx* ctx, const int* d_flags, const char* who) {
  int fl = 0;
  PA_HIP(hipMemcpyAsync(&fl, d_flags, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipStreamSynchronize(ctx->stream));
  if (fl & PA_ST_BADBIN) return pa_fail(ctx, std::string(who) + ": Bad bin");
  if (fl & PA_ST_NONFINITE) return pa_fail(ctx, std::string(who) + ": a value that is not finite went into a sum");
  if (fl & PA_ST_OVERFLOW) return pa_fail(ctx, std::string(who) + ": a term exceeds the magnitude declared at begin (accumulator overflow)");
  return 0;
}
