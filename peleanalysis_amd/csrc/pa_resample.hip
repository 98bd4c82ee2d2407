// pa_resample.hip -- a hierarchy's data on a BoxArray that is not its own, and the running sum of avgPlotfiles.cpp (:156-195).
//
// For one file and one level l the kernel fills the cells of the TARGET level's boxes -- valid cells and, in the work multifab
// T_l, gt ghost layers -- with V(f, l): the file's own level-l value where one of its boxes holds the cell (owner map of the
// file's level), else the interpolant of V(f, l-1), read from the work multifab T_{l-1} of the coarser target level
// (interp_type 0: the parent; 1: pa_cclin.h, the arithmetic of FillPatchTwoLevels).  Every cell of T_l holds the value of its
// CANONICAL cell -- clamped into the domain across a wall, wrapped across a periodic face -- so the 27 coarse neighbours of
// a parent are plain loads at fixed offsets around it in ONE grown coarse FAB: no owner-map walk, no clamping in the gather.
// The valid cells are added to the running sum by the thread that computed them (one thread per cell, files in call order:
// the sum is reproducible by bits and does not depend on the tiling); there are no atomics on data.
//
// Thread per coarse PARENT of the grown box (ratio R: R^3 children share slopes and alpha; level 0: R = 1, a parent is the
// cell), x fastest over the parent grid of the box, so a wavefront covers 64 R consecutive fine cells of a row -- 512 R bytes
// -- or, in a box narrower than that, several rows.  Parents whose children are all in the file skip the gather.
#include "pa_resample.h"
#include <cmath>

struct pa_resample {
  pa_ctx* ctx = nullptr;
  unsigned long long* d_nosrc = nullptr;
  std::vector<pa_mf*> sum;
  int nvar = 0;
  bool begun = false;
};

template <int R>
__global__ __launch_bounds__(256) void k_resample(const RsArgs A, unsigned long long* nosrc) {
  rs_parent<R, true>(A, (int)blockIdx.x, blockIdx.y * 256u + threadIdx.x, nosrc);
}

// running_data[lev].mult(factor), avgPlotfiles.cpp:192-195: valid cells of the first nvar components
__global__ __launch_bounds__(256) void k_rs_scale(DLevelView L, DMFView S, int nvar, double factor) {
  const int b = blockIdx.x;
  const DBox B = L.boxes[b];
  const unsigned nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const unsigned n = nx * ny * nz;
  double* s = S.data + S.off[b];
  for (unsigned t = blockIdx.y * 256u + threadIdx.x; t < n; t += gridDim.y * 256u) {
    const unsigned row = t / nx;
    const int i = B.lo[0] + (int)(t - row * nx), j = B.lo[1] + (int)(row % ny), k = B.lo[2] + (int)(row / ny);
    for (int v = 0; v < nvar; ++v) {
      double* p = s + fab_index(B, S.ng, S.ncomp, v, i, j, k);
      *p = *p * factor;
    }
  }
}

extern "C" pa_resample* pa_resample_create(pa_ctx* ctx) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  pa_resample* h = new pa_resample;
  h->ctx = ctx;
  if (hipMalloc(&h->d_nosrc, sizeof(unsigned long long)) != hipSuccess || hipMemset(h->d_nosrc, 0, sizeof(unsigned long long)) != hipSuccess) {
    pa_fail(ctx, "pa_resample_create: out of device memory");
    if (h->d_nosrc) (void)hipFree(h->d_nosrc);
    delete h;
    return nullptr;
  }
  return h;
}

extern "C" void pa_resample_destroy(pa_resample* h) {
  if (!h) return;
  PaBind bind_(h->ctx);
  if (h->ctx && h->ctx->stream) (void)hipStreamSynchronize(h->ctx->stream);
  if (h->d_nosrc) (void)hipFree(h->d_nosrc);
  delete h;
}

extern "C" int pa_resample_begin(pa_ctx* ctx, pa_resample* h, int nlev, pa_mf* const* sum, int nvar) {
  PaBind bind_(ctx);
  if (!ctx || !h || !sum) return pa_fail(ctx, "pa_resample_begin: null argument");
  if (nlev < 1) return pa_fail(ctx, "pa_resample_begin: no level");
  if (nvar < 1 || nvar > PA_RS_MAXV) return pa_fail(ctx, "pa_resample_begin: 1 to " + std::to_string(PA_RS_MAXV) + " variables per pass");
  for (int l = 0; l < nlev; ++l) {
    if (!sum[l]) return pa_fail(ctx, "pa_resample_begin: null running multifab");
    if (sum[l]->ncomp < nvar) return pa_fail(ctx, "pa_resample_begin: the running multifab has fewer components than variables");
    if (sum[l]->lev->nranks > 1) return pa_fail(ctx, "pa_resample_begin: sharded levels are not supported");
  }
  h->sum.assign(sum, sum + nlev);
  h->nvar = nvar;
  for (int l = 0; l < nlev; ++l)
    if (pa_mf_setval(ctx, sum[l], 0, nvar, 0.0)) return 1;  // running_data[lev].setVal(0.0), :167
  PA_HIP(hipMemsetAsync(h->d_nosrc, 0, sizeof(unsigned long long), ctx->stream));
  h->begun = true;
  return 0;
}

extern "C" int pa_resample_add_file_level(pa_ctx* ctx, pa_resample* h, int lev, const pa_mf* file, const int32_t* comp_map, const pa_mf* crse_work,
                                          int ratio, int interp_type, pa_mf* work) {
  PaBind bind_(ctx);
  if (!ctx || !h) return pa_fail(ctx, "pa_resample_add_file_level: null argument");
  if (!h->begun) return pa_fail(ctx, "pa_resample_add_file_level: pa_resample_begin has not been called");
  if (lev < 0 || lev >= (int)h->sum.size()) return pa_fail(ctx, "pa_resample_add_file_level: level out of range");
  if (interp_type != 0 && interp_type != 1) return pa_fail(ctx, "pa_resample_add_file_level: interp_type must be 0 or 1");
  pa_mf* S = h->sum[lev];
  const pa_level* U = S->lev;
  if (U->boxes.empty()) return 0;
  if (lev == 0 && (!file || crse_work)) return pa_fail(ctx, "pa_resample_add_file_level: level 0 is read from the file alone");
  if (lev > 0 && !crse_work) return pa_fail(ctx, "pa_resample_add_file_level: a finer level needs the coarser work multifab");
  if (file && !comp_map) return pa_fail(ctx, "pa_resample_add_file_level: null component map");
  RsArgs A;
  A.U = U->view;
  A.S = S->view;
  A.has_t = work != nullptr;
  A.gt = 0;
  A.T = S->view;
  if (work) {
    if (work->lev != U) return pa_fail(ctx, "pa_resample_add_file_level: the work multifab is not on the running multifab's level");
    if (work->ncomp < h->nvar) return pa_fail(ctx, "pa_resample_add_file_level: the work multifab has fewer components than variables");
    A.T = work->view;
    A.gt = work->ng;
  }
  A.has_f = file != nullptr;
  A.F = U->view;
  A.FM = S->view;
  if (file) {
    const pa_level* F = file->lev;
    if (F->nranks > 1) return pa_fail(ctx, "pa_resample_add_file_level: sharded levels are not supported");
    for (int d = 0; d < 3; ++d)
      if (F->domlo[d] != U->domlo[d] || F->domhi[d] != U->domhi[d]) return pa_fail(ctx, "pa_resample_add_file_level: the file's level has another domain");  // :135-138
    for (int v = 0; v < h->nvar; ++v)
      if (comp_map[v] < 0 || comp_map[v] >= file->ncomp) return pa_fail(ctx, "pa_resample_add_file_level: component map out of range");
    A.F = F->view;
    A.FM = file->view;
  }
  A.has_c = crse_work != nullptr;
  A.UC = U->view;
  A.TC = S->view;
  if (crse_work) {
    const pa_level* C = crse_work->lev;
    if (ratio != 2 && ratio != 4) return pa_fail(ctx, "pa_resample_add_file_level: the refinement ratio must be 2 or 4");
    if (C != h->sum[lev - 1]->lev) return pa_fail(ctx, "pa_resample_add_file_level: the coarser work multifab is not on the coarser running multifab's level");
    if (crse_work->ncomp < h->nvar) return pa_fail(ctx, "pa_resample_add_file_level: the coarser work multifab has fewer components than variables");
    for (int d = 0; d < 3; ++d)
      if (U->domlo[d] != C->domlo[d] * ratio || U->domhi[d] + 1 != (C->domhi[d] + 1) * ratio || U->is_per[d] != C->is_per[d])
        return pa_fail(ctx, "pa_resample_add_file_level: the level's domain is not the coarser one refined by the ratio");
    // coarsen(grow(U_l, g)) + 1 lies inside grow(U_{l-1}, g + 1): one more layer per level down
    const int need = (A.gt + ratio - 1) / ratio + (interp_type == 1 ? 1 : 0);
    if (crse_work->ng < need) return pa_fail(ctx, "pa_resample_add_file_level: the coarser work multifab needs " + std::to_string(need) + " ghost layers");
    A.UC = C->view;
    A.TC = crse_work->view;
  }
  A.interp = interp_type;
  A.nvar = h->nvar;
  for (int v = 0; v < PA_RS_MAXV; ++v) A.comp[v] = file && v < h->nvar ? comp_map[v] : 0;
  const int R = crse_work ? ratio : 1;
  long long maxp = 1;
  for (const DBox& B : U->boxes) {
    long long n = 1;
    for (int d = 0; d < 3; ++d) n *= coarsen_idx(B.hi[d] + A.gt, R) - coarsen_idx(B.lo[d] - A.gt, R) + 1;
    maxp = std::max(maxp, n);
  }
  const long long ny = (maxp + 255) / 256;
  if (ny > 65535) return pa_fail(ctx, "pa_resample_add_file_level: a box of the target level is too large (chop it)");
  const dim3 grid((unsigned)U->boxes.size(), (unsigned)ny);
  if (R == 1) hipLaunchKernelGGL(k_resample<1>, grid, dim3(256), 0, ctx->stream, A, h->d_nosrc);
  else if (R == 2) hipLaunchKernelGGL(k_resample<2>, grid, dim3(256), 0, ctx->stream, A, h->d_nosrc);
  else hipLaunchKernelGGL(k_resample<4>, grid, dim3(256), 0, ctx->stream, A, h->d_nosrc);
  PA_HIP(hipGetLastError());
  return 0;
}

extern "C" int pa_resample_finish(pa_ctx* ctx, pa_resample* h, int nfiles, int64_t* nosrc) {
  PaBind bind_(ctx);
  if (!ctx || !h) return pa_fail(ctx, "pa_resample_finish: null argument");
  if (!h->begun) return pa_fail(ctx, "pa_resample_finish: pa_resample_begin has not been called");
  if (nfiles < 1) return pa_fail(ctx, "pa_resample_finish: no file");
  const double factor = 1.0 / (double)nfiles;  // :192
  for (pa_mf* S : h->sum) {
    if (S->lev->boxes.empty()) continue;
    hipLaunchKernelGGL(k_rs_scale, dim3((unsigned)S->lev->boxes.size(), 16), dim3(256), 0, ctx->stream, S->lev->view, S->view, h->nvar, factor);
    PA_HIP(hipGetLastError());
  }
  unsigned long long n = 0;
  PA_HIP(hipStreamSynchronize(ctx->stream));
  PA_HIP(hipMemcpy(&n, h->d_nosrc, sizeof n, hipMemcpyDeviceToHost));
  if (nosrc) *nosrc = (int64_t)n;
  h->begun = false;
  return 0;
}
