// pa_flatten.hip -- one level of one file on ANY list of disjoint boxes of the level's domain, without a running sum
// (flattenAMRFile.cpp:77-89: geom, grid.maxSize, fillPatchFromPlt).  Every valid and ghost cell of `out` receives V(f, l) as
// pa_resample defines it: the file's own value where one of its boxes holds the (canonical) cell, else the interpolant of V(f, l-1)
// read from `crse`.  Two routes, chosen per box on the host:
//
// Wide route (k_prolong + k_overlay): boxes without ghost cells whose rows start on a parent's edge, are whole parents wide and are
// 16-byte aligned.  One thread per coarse parent, x fastest, so a wavefront covers 64 consecutive parents of a parent row (in a
// narrower box: several rows); the 27 coarse neighbours are plain loads at fixed offsets in one grown coarse FAB, straight from
// global memory (they are 1/8 of the written bytes at ratio 2 and neighbouring lanes and rows share them through L2; no LDS
// staging); slopes once per parent, ccl_child once per child (pa_cclin.h: the operands and order of every other
// user).  A child row of a parent is stored as 16-byte vectors -- one per lane at ratio 2, two at ratio 4 -- so a store instruction
// of a wavefront writes 1 KiB of one output row contiguously; the stores are non-temporal, nothing on the device reads the
// output again.  k_overlay then copies the file's own cells over the interpolant, 8 bytes per cell as integers (-0.0 and NaN
// payloads survive), through a host-built table of rectangles (file box) n (output box); a box that its rectangles cover skips
// k_prolong.  Both kernels are launched over (box, tile) / (rectangle, tile) tables: no block is empty.
//
// General route (k_flatten_general): every other box -- ghost cells, level 0 (ratio 1), boxes off the ratio's alignment, odd
// widths.  The per-parent code of k_resample (pa_resample.h: rs_parent) without the sum.
#include "pa_resample.h"
#define PA_FLATTEN_PLAN_ONLY
#include "../../tools/common/pa_flatten_plan.h"
#include <algorithm>
#include <limits>

typedef double pa_d2 __attribute__((ext_vector_type(2)));

static int64_t g_flat_last[4] = {0, 0, 0, 0};

FlPlan::~FlPlan() {
  if (d_ptile) (void)hipFree(d_ptile);
  if (d_rects) (void)hipFree(d_rects);
  if (d_otile) (void)hipFree(d_otile);
  if (d_glist) (void)hipFree(d_glist);
}

struct PrArgs {
  DLevelView U;   // the output boxes (a slab)
  DMFView O;
  DLevelView F;   // the file's level (has_f): only asked where the coarse data is missing, for the count
  DLevelView UC;  // the coarser level and its multifab
  DMFView TC;
  int has_f, interp, nvar;
};

template <int R>
__global__ __launch_bounds__(256) void k_prolong(const PrArgs A, const int2* __restrict__ tiles, unsigned long long* nosrc) {
  const int2 bt = tiles[blockIdx.x];
  const int b = bt.x;
  const DBox B = A.U.boxes[b];
  int clo[3], cn[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    clo[d] = coarsen_idx(B.lo[d], R);
    cn[d] = coarsen_idx(B.hi[d], R) - clo[d] + 1;
  }
  const unsigned t = (unsigned)bt.y * 256u + threadIdx.x;
  if (t >= (unsigned)cn[0] * (unsigned)cn[1] * (unsigned)cn[2]) return;  // (the last tile of a box)
  const unsigned row = t / (unsigned)cn[0];
  const int qc[3] = {clo[0] + (int)(t - row * (unsigned)cn[0]), clo[1] + (int)(row % (unsigned)cn[1]), clo[2] + (int)(row / (unsigned)cn[1])};

  // the parent is a valid cell of the coarse domain (the children are valid cells of the fine one): the coarse box that holds it,
  // grown by its ghost layers, has to hold the neighbours
  const double* p0 = nullptr;
  int sy = 0, sz = 0;
  long long cstride = 0;
  {
    const int cb = owner_of(A.UC, qc);
    if (cb >= 0) {
      const DBox CB = A.UC.boxes[cb];
      const int need = A.interp == 1 ? 1 : 0;
      bool ok = true;
#pragma unroll
      for (int d = 0; d < 3; ++d) ok = ok && qc[d] - need >= CB.lo[d] - A.TC.ng && qc[d] + need <= CB.hi[d] + A.TC.ng;
      if (ok) {
        sy = CB.hi[0] - CB.lo[0] + 1 + 2 * A.TC.ng;
        sz = sy * (CB.hi[1] - CB.lo[1] + 1 + 2 * A.TC.ng);  // a coarse FAB is far below 2^31 cells
        p0 = A.TC.data + A.TC.off[cb] + fab_index(CB, A.TC.ng, A.TC.ncomp, 0, qc[0], qc[1], qc[2]);
        cstride = fab_index(CB, A.TC.ng, A.TC.ncomp, 1, qc[0], qc[1], qc[2]) - fab_index(CB, A.TC.ng, A.TC.ncomp, 0, qc[0], qc[1], qc[2]);
      }
    }
  }
  if (!p0) {  // no coarse data: the children the file does not hold are counted (they keep the NaN stored below)
    unsigned n = 0;
    for (int c = 0; c < R * R * R; ++c) {
      const int q[3] = {R * qc[0] + c % R, R * qc[1] + (c / R) % R, R * qc[2] + c / (R * R)};
      if (q[1] < B.lo[1] || q[1] > B.hi[1] || q[2] < B.lo[2] || q[2] > B.hi[2]) continue;
      if (!(A.has_f && owner_of(A.F, q) >= 0)) ++n;
    }
    if (n) atomicAdd(nosrc, (unsigned long long)n);
  }

  const long long nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const long long ocs = pa_cstride(nx * ny * nz, A.O.ncomp);
  double* const ob = A.O.data + A.O.off[b] + (R * qc[0] - B.lo[0]);
  for (int v = 0; v < A.nvar; ++v) {
    double u0 = std::numeric_limits<double>::quiet_NaN(), sl[3] = {0.0, 0.0, 0.0}, alpha = 1.0;
    if (p0) {
      const double* pv = p0 + (long long)v * cstride;
      u0 = pv[0];
      if (A.interp == 1) {
        double w[27];  // index (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
#pragma unroll
        for (int n = 0; n < 27; ++n) w[n] = pv[(n / 9 - 1) * sz + ((n / 3) % 3 - 1) * sy + (n % 3 - 1)];
        ccl_slopes<true>([&](int n) { return w[n]; }, u0, R, sl, alpha);
      }
    }
    const bool lin = p0 && A.interp == 1;
#pragma unroll
    for (int cz = 0; cz < R; ++cz) {
      const int k = R * qc[2] + cz;
      if (k < B.lo[2] || k > B.hi[2]) continue;
#pragma unroll
      for (int cy = 0; cy < R; ++cy) {
        const int j = R * qc[1] + cy;
        if (j < B.lo[1] || j > B.hi[1]) continue;
        double* const orow = ob + (long long)v * ocs + ((long long)(k - B.lo[2]) * ny + (j - B.lo[1])) * nx;
#pragma unroll
        for (int cx = 0; cx < R; cx += 2) {
          const int r0[3] = {cx, cy, cz}, r1[3] = {cx + 1, cy, cz};
          pa_d2 val;
          val.x = lin ? ccl_child(u0, sl, alpha, r0, R) : u0;
          val.y = lin ? ccl_child(u0, sl, alpha, r1, R) : u0;
          __builtin_nontemporal_store(val, (pa_d2*)(orow + cx));
        }
      }
    }
  }
}

struct OvArgs {
  DMFView O, FM;
  const DBox* oboxes;
  const DBox* fboxes;
  int nvar;
  int comp[PA_RS_MAXV];
};

// the file's own cells over the interpolant: rectangle tiles[].x, its cells tiles[].y * 256 .. + 255 in x-fastest order
__global__ __launch_bounds__(256) void k_overlay(const OvArgs A, const pa::FlatRect* __restrict__ rects, const int2* __restrict__ tiles) {
  const int2 rt = tiles[blockIdx.x];
  const pa::FlatRect r = rects[rt.x];
  const unsigned nx = r.hi[0] - r.lo[0] + 1, ny = r.hi[1] - r.lo[1] + 1, nz = r.hi[2] - r.lo[2] + 1;
  const unsigned t = (unsigned)rt.y * 256u + threadIdx.x;
  if (t >= nx * ny * nz) return;
  const unsigned row = t / nx;
  const int i = r.lo[0] + (int)(t - row * nx), j = r.lo[1] + (int)(row % ny), k = r.lo[2] + (int)(row / ny);
  const DBox FB = A.fboxes[r.fbox], OB = A.oboxes[r.obox];
  const unsigned long long* src = (const unsigned long long*)(A.FM.data + A.FM.off[r.fbox]);
  unsigned long long* dst = (unsigned long long*)(A.O.data + A.O.off[r.obox]);
  for (int v = 0; v < A.nvar; ++v)
    dst[fab_index(OB, A.O.ng, A.O.ncomp, v, i, j, k)] = src[fab_index(FB, A.FM.ng, A.FM.ncomp, A.comp[v], i, j, k)];
}

template <int R>
__global__ __launch_bounds__(256) void k_flatten_general(const RsArgs A, const int* __restrict__ glist, unsigned long long* nosrc) {
  rs_parent<R, false>(A, glist[blockIdx.x], blockIdx.y * 256u + threadIdx.x, nosrc);
}

// the launch tables of (out, file) at ratio R, built on first use and kept with the output level
static const FlPlan* flatten_plan(pa_ctx* ctx, const pa_mf* out, const pa_mf* file, int R) {
  const pa_level* U = out->lev;
  const bool aligned = ((uintptr_t)out->data & 15u) == 0;
  const std::array<long long, 5> key = {file ? file->lev->serial : 0, R, out->ng, out->ncomp, aligned ? 1 : 0};
  auto it = U->fl_plans.find(key);
  if (it != U->fl_plans.end()) return it->second.get();
  if (U->fl_plans.size() >= 8) {  // (a level that is flattened from ever new file levels)
    (void)hipStreamSynchronize(ctx->stream);
    U->fl_plans.clear();
  }
  const size_t nb = U->boxes.size();
  std::vector<char> wide(nb, 0);
  std::vector<int> glist;
  long long gmax = 1;
  for (size_t b = 0; b < nb; ++b) {
    const DBox& B = U->boxes[b];
    const long long nx = B.hi[0] - B.lo[0] + 1, n = nx * (B.hi[1] - B.lo[1] + 1) * (B.hi[2] - B.lo[2] + 1);
    // rows 16-byte aligned: the base, the FAB's offset, the component stride (pa_mf_layout pads it; checked, not assumed), the row
    // length and the row's first cell are all even numbers of doubles
    const bool ok = R > 1 && out->ng == 0 && aligned && ((B.lo[0] % R) + R) % R == 0 && nx % R == 0 && out->off[b] % 2 == 0 && pa_cstride(n, out->ncomp) % 2 == 0;
    wide[b] = ok ? 1 : 0;
    if (!ok) {
      glist.push_back((int)b);
      long long np = 1;
      for (int d = 0; d < 3; ++d) np *= coarsen_idx(B.hi[d] + out->ng, R) - coarsen_idx(B.lo[d] - out->ng, R) + 1;
      gmax = std::max(gmax, np);
    }
  }
  std::vector<long long> covered;
  std::vector<pa::FlatRect> rects;
  if (file) rects = pa::flat_rects(file->lev->boxes, U->boxes, &wide, &covered);
  else covered.assign(nb, 0);
  std::unique_ptr<FlPlan> P(new FlPlan);
  std::vector<int2> ptile, otile;
  for (size_t b = 0; b < nb; ++b) {
    if (!wide[b]) continue;
    const DBox& B = U->boxes[b];
    long long n = 1, np = 1;
    for (int d = 0; d < 3; ++d) {
      n *= B.hi[d] - B.lo[d] + 1;
      np *= coarsen_idx(B.hi[d], R) - coarsen_idx(B.lo[d], R) + 1;
    }
    if (covered[b] == n) { ++P->nskipped; continue; }
    ++P->nwide;
    for (long long t = 0; t < (np + 255) / 256; ++t) ptile.push_back(make_int2((int)b, (int)t));
  }
  for (size_t r = 0; r < rects.size(); ++r)
    for (long long t = 0; t < (rects[r].numPts() + 255) / 256; ++t) otile.push_back(make_int2((int)r, (int)t));
  P->ngeneral = (int)glist.size();
  P->nrect = (int)rects.size();
  P->nptile = (int)ptile.size();
  P->notile = (int)otile.size();
  P->ngtile = (int)((gmax + 255) / 256);
  if (P->ngtile > 65535) { pa_fail(ctx, "pa_flatten_level: a box of the output is too large (chop it)"); return nullptr; }
  auto up = [&](void** d, const void* h, size_t bytes) {
    if (bytes == 0) return true;
    return hipMalloc(d, bytes) == hipSuccess && hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(&P->d_ptile, ptile.data(), ptile.size() * sizeof(int2)) || !up(&P->d_rects, rects.data(), rects.size() * sizeof(pa::FlatRect)) ||
      !up(&P->d_otile, otile.data(), otile.size() * sizeof(int2)) || !up((void**)&P->d_glist, glist.data(), glist.size() * sizeof(int))) {
    pa_fail(ctx, "pa_flatten_level: out of device memory");
    return nullptr;
  }
  return (U->fl_plans[key] = std::move(P)).get();
}

extern "C" int pa_flatten_level(pa_ctx* ctx, const pa_mf* file, const int32_t* comp_map, const pa_mf* crse, int ratio, int interp_type, pa_mf* out,
                                int nvar, int64_t* nosrc) {
  PaBind bind_(ctx);
  if (!ctx || !out) return pa_fail(ctx, "pa_flatten_level: null argument");
  if (nvar < 1 || nvar > PA_RS_MAXV) return pa_fail(ctx, "pa_flatten_level: 1 to " + std::to_string(PA_RS_MAXV) + " variables per call");
  if (interp_type != 0 && interp_type != 1) return pa_fail(ctx, "pa_flatten_level: interp_type must be 0 or 1");
  if (out->ncomp < nvar) return pa_fail(ctx, "pa_flatten_level: the output multifab has fewer components than variables");
  const pa_level* U = out->lev;
  if (U->nranks > 1) return pa_fail(ctx, "pa_flatten_level: sharded levels are not supported");
  if (!file && !crse) return pa_fail(ctx, "pa_flatten_level: neither the file's level nor a coarser multifab");
  if (file && !comp_map) return pa_fail(ctx, "pa_flatten_level: null component map");
  RsArgs A;
  A.U = U->view;
  A.S = out->view;  // (not touched: there is no running sum)
  A.T = out->view;
  A.has_t = 1;
  A.gt = out->ng;
  A.has_f = file != nullptr;
  A.F = U->view;
  A.FM = out->view;
  if (file) {
    const pa_level* F = file->lev;
    if (F->nranks > 1) return pa_fail(ctx, "pa_flatten_level: sharded levels are not supported");
    for (int d = 0; d < 3; ++d)
      if (F->domlo[d] != U->domlo[d] || F->domhi[d] != U->domhi[d]) return pa_fail(ctx, "pa_flatten_level: the file's level has another domain");
    for (int v = 0; v < nvar; ++v)
      if (comp_map[v] < 0 || comp_map[v] >= file->ncomp) return pa_fail(ctx, "pa_flatten_level: component map out of range");
    A.F = F->view;
    A.FM = file->view;
  }
  A.has_c = crse != nullptr;
  A.UC = U->view;
  A.TC = out->view;
  if (crse) {
    const pa_level* C = crse->lev;
    if (ratio != 2 && ratio != 4) return pa_fail(ctx, "pa_flatten_level: the refinement ratio must be 2 or 4");
    if (C->nranks > 1) return pa_fail(ctx, "pa_flatten_level: sharded levels are not supported");
    if (crse->ncomp < nvar) return pa_fail(ctx, "pa_flatten_level: the coarser multifab has fewer components than variables");
    for (int d = 0; d < 3; ++d)
      if (U->domlo[d] != C->domlo[d] * ratio || U->domhi[d] + 1 != (C->domhi[d] + 1) * ratio || U->is_per[d] != C->is_per[d])
        return pa_fail(ctx, "pa_flatten_level: the level's domain is not the coarser one refined by the ratio");
    const int need = (out->ng + ratio - 1) / ratio + (interp_type == 1 ? 1 : 0);
    if (crse->ng < need) return pa_fail(ctx, "pa_flatten_level: the coarser multifab needs " + std::to_string(need) + " ghost layers");
    A.UC = C->view;
    A.TC = crse->view;
  }
  A.interp = interp_type;
  A.nvar = nvar;
  for (int v = 0; v < PA_RS_MAXV; ++v) A.comp[v] = file && v < nvar ? comp_map[v] : 0;
  if (!ctx->d_flat_nosrc) PA_HIP(hipMalloc(&ctx->d_flat_nosrc, sizeof(unsigned long long)));
  PA_HIP(hipMemsetAsync(ctx->d_flat_nosrc, 0, sizeof(unsigned long long), ctx->stream));
  for (int q = 0; q < 4; ++q) g_flat_last[q] = 0;
  if (!U->boxes.empty()) {
    const int R = crse ? ratio : 1;
    const FlPlan* P = flatten_plan(ctx, out, file, R);
    if (!P) return 1;
    if (P->ngeneral > 0) {
      const dim3 grid((unsigned)P->ngeneral, (unsigned)P->ngtile);
      if (R == 1) hipLaunchKernelGGL(k_flatten_general<1>, grid, dim3(256), 0, ctx->stream, A, P->d_glist, ctx->d_flat_nosrc);
      else if (R == 2) hipLaunchKernelGGL(k_flatten_general<2>, grid, dim3(256), 0, ctx->stream, A, P->d_glist, ctx->d_flat_nosrc);
      else hipLaunchKernelGGL(k_flatten_general<4>, grid, dim3(256), 0, ctx->stream, A, P->d_glist, ctx->d_flat_nosrc);
      PA_HIP(hipGetLastError());
    }
    if (P->nptile > 0) {
      PrArgs W;
      W.U = A.U; W.O = out->view; W.F = A.F; W.UC = A.UC; W.TC = A.TC;
      W.has_f = A.has_f; W.interp = interp_type; W.nvar = nvar;
      if (R == 2) hipLaunchKernelGGL(k_prolong<2>, dim3((unsigned)P->nptile), dim3(256), 0, ctx->stream, W, (const int2*)P->d_ptile, ctx->d_flat_nosrc);
      else hipLaunchKernelGGL(k_prolong<4>, dim3((unsigned)P->nptile), dim3(256), 0, ctx->stream, W, (const int2*)P->d_ptile, ctx->d_flat_nosrc);
      PA_HIP(hipGetLastError());
    }
    if (P->notile > 0) {
      OvArgs V;
      V.O = out->view; V.FM = file->view; V.oboxes = U->view.boxes; V.fboxes = file->lev->view.boxes; V.nvar = nvar;
      for (int v = 0; v < PA_RS_MAXV; ++v) V.comp[v] = A.comp[v];
      hipLaunchKernelGGL(k_overlay, dim3((unsigned)P->notile), dim3(256), 0, ctx->stream, V, (const pa::FlatRect*)P->d_rects, (const int2*)P->d_otile);
      PA_HIP(hipGetLastError());
    }
    g_flat_last[0] = P->nwide; g_flat_last[1] = P->ngeneral; g_flat_last[2] = P->nskipped; g_flat_last[3] = P->nrect;
  }
  if (nosrc) PA_HIP(hipMemcpyAsync(nosrc, ctx->d_flat_nosrc, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

extern "C" void pa_flatten_last_launch(int64_t counts[4]) {
  if (!counts) return;
  for (int q = 0; q < 4; ++q) counts[q] = g_flat_last[q];
}
