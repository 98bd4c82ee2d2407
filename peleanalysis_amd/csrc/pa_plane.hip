// pa_plane.hip -- avgToPlane.cpp (:121-201) and slicePlot.cpp (:51-55) on gfx950 (the avgToPlane3d / slicePlot3d tools): a whole hierarchy
// reduced to ONE plane at the finest level's resolution -- the sum along `dir` of the composite field over a sub-box, or one slice of
// it -- then the plane's non-NaN min / max and pixelizeData's 256 levels.
//   Composite value F(i,j,k) of a cell of the finest level (FillVar, recalled: DESIGN.md 1): the value of the finest level <= finestLevel
//   whose grids hold the cell's coarsened image, no interpolation (pl_resolve: the rule of ss_cell in pa_streamsample.hip without the
//   periodic images).  A cell no level holds is counted (nosrc) and reads as NaN.
//   k_plane_sum<NC>: a thread per pixel walks its column through the hierarchy IN PLACE: the sub-box's volume is never staged.  The
//     owner is resolved once per RUN and reused for the NC <= 4 components of the launch.  A run inside a box of the finest level goes
//     to the box's end: plain loads at a fixed stride.  A run under a coarse cell is the R fine positions the cell spans: one load, R
//     additions; while the NEXT cell of that level lies in the same box only the finer levels' owner maps are asked (lookups that do
//     not depend on each other) and the cell's values, whose address is known, are loaded beside them -- one memory round trip per
//     coarse cell instead of owner -> box -> offset -> value.  The order is the reference's: s_c = (((0.0 + F(a_c)) + ...) + F(b_c))
//     over the cells of chunk c of pa::max_size along dir (the MFIter loop, :164-199), S = (((0.0 + s_0) + s_1) + ...) (ParallelAdd, :201).
//     Neighbouring threads are neighbours in the plane's first direction: i for dir 1 and 2 (a wavefront's loads on the finest level
//     are 512 contiguous bytes), j for dir 0, where a lane takes 8 bytes of a line per step and the 15 steps that follow find the line
//     in cache.  A variant that staged 64 rows x 16 cells through LDS (whole 128-byte lines, summed per row from LDS, stride 17) was
//     built and measured 5 to 14 times SLOWER than this walk on the headline hierarchy and is not kept.
//   k_plane_slice: F on the plane index[dir] == sliceloc, every component, bits kept (-0.0 stays -0.0).
//   k_plane_minmax: per-workgroup min / max of the non-NaN values (order-free); the host folds the partial results.
//   k_plane_pixelize: t = (v - min) / (max - min); level 0 if !(t > 0) (NaN t included: the reference's cast is undefined there), else
//     (int)(255 * (t < 1 ? t : 1)).
// No atomics on data (the nosrc counter is one), no fixed-point sums: the image bytes depend on the sum's bits.
// PRECONDITION of the run logic: every level's grids are whole refined cells of the next coarser level (a finer level never holds PART
// of the fine positions under a coarser cell that owns one of them): true of every AMR plotfile (blocking factor >= ratio, proper nesting).
#include "pa_internal.h"
#include <climits>
#include <cmath>
#include <limits>

#define PA_PL_MAXLEV 8
#define PA_PL_SC 16     // components per launch of the slice kernel (the component map travels in the kernel arguments)
#define PA_PL_NC 4      // components per launch of the sum kernels (their partial sums live in registers)
#define PA_PL_MMB 256   // workgroups of the min / max kernel

struct pa_plane {
  pa_ctx* ctx = nullptr;
  int ncomp = 0, dir = 0, slice = 0;
  int lo[3], hi[3];
  int W = 0, H = 0;
  std::vector<int> chunk_end;  // last index along dir of every chunk (sum)
  int* d_chunk_end = nullptr;
  double* d_out = nullptr;     // [ncomp][H][W]
  double* d_part = nullptr;    // [2][PA_PL_MMB]
  unsigned char* d_pix = nullptr;
  unsigned long long* d_nosrc = nullptr;
  bool ran = false;
};

struct PlArgs {
  int nlev, dir, nchunk, ncomp, W, H;
  int lo[3], hi[3];
  int ratio[PA_PL_MAXLEV];  // ratio[l]: level l to level l - 1 (l >= 1)
  DLevelView L[PA_PL_MAXLEV];
  DMFView M[PA_PL_MAXLEV];
  const int* chunk_end;
  int c0, nc;               // this launch: components c0 .. c0 + nc - 1 of the plane ...
  int comp[PA_PL_SC];       // ... are these components of the levels' multifabs
  double* out;
  unsigned long long* nosrc;
};

// the source of cell q of the finest level: pointer to component 0 and the component stride (null: no level holds it); lev = the
// owning level, B its box, span = fine cells per cell of that level
struct PlSrc {
  const double* p;
  long long cs;
  int lev, span, ng;
  DBox B;
};

__device__ __forceinline__ PlSrc pl_resolve(const PlArgs& A, const int q[3]) {
  PlSrc s;
  s.p = nullptr;
  s.cs = 0;
  s.span = 1;
  s.lev = -1;
  s.ng = 0;
  // every level's owner-map entry first -- the loads do not depend on each other --, then the finest hit: one round trip, not one per level
  int p[3] = {q[0], q[1], q[2]}, span = 1;
  int hit = -1, ho = -1, hp[3] = {0, 0, 0}, hng = 0, hnc = 1;
  const DBox* hboxes = nullptr;
  double* hdata = nullptr;
  const long long* hoff = nullptr;
#pragma unroll
  for (int u = 0; u < PA_PL_MAXLEV; ++u) {
    const int l = A.nlev - 1 - u;
    if (l < 0) break;
    const int o = owner_of(A.L[l], p);
    if (o >= 0 && hit < 0) {
      hit = l;
      ho = o;
      s.span = span;
      hboxes = A.L[l].boxes;
      hdata = A.M[l].data;
      hoff = A.M[l].off;
      hng = A.M[l].ng;
      hnc = A.M[l].ncomp;
#pragma unroll
      for (int d = 0; d < 3; ++d) hp[d] = p[d];
    }
    if (l > 0) {
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] = coarsen_idx(p[d], A.ratio[l]);
      span *= A.ratio[l];
    }
  }
  if (hit < 0) {
    s.span = span;
    return s;
  }
  s.B = hboxes[ho];
  s.cs = pa_cstride((long long)(s.B.hi[0] - s.B.lo[0] + 1 + 2 * hng) * (s.B.hi[1] - s.B.lo[1] + 1 + 2 * hng) * (s.B.hi[2] - s.B.lo[2] + 1 + 2 * hng), hnc);
  s.p = hdata + hoff[ho] + fab_index(s.B, hng, hnc, 0, hp[0], hp[1], hp[2]);
  s.lev = hit;
  s.ng = hng;
  return s;
}

// does a level finer than l0 hold cell q of the finest level?  (the lookups do not depend on each other)
__device__ __forceinline__ bool pl_finer_hit(const PlArgs& A, const int q[3], int l0) {
  int p[3] = {q[0], q[1], q[2]};
  bool hit = false;
#pragma unroll
  for (int u = 0; u < PA_PL_MAXLEV; ++u) {
    const int l = A.nlev - 1 - u;
    if (l <= l0) break;
    hit = hit || owner_of(A.L[l], p) >= 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) p[d] = coarsen_idx(p[d], A.ratio[l]);
  }
  return hit;
}

// pixel (x, y) of the plane -> the two indices other than dir
__device__ __forceinline__ void pl_pixel_cell(const PlArgs& A, int x, int y, int q[3]) {
  const int d0 = A.dir == 0 ? 1 : 0, d1 = A.dir == 2 ? 1 : 2;
  q[d0] = A.lo[d0] + x;
  q[d1] = A.lo[d1] + y;
}

template <int NC>
__global__ __launch_bounds__(256) void k_plane_sum(const PlArgs A) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= A.W || y >= A.H) return;
  const int dir = A.dir, F = A.nlev - 1, last = A.hi[dir];
  int q[3];
  pl_pixel_cell(A, x, y, q);
  int comp[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) comp[c] = A.comp[c];
  double s[NC], S[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) s[c] = S[c] = 0.0;
  int ci = 0, cend = A.chunk_end[0];
  unsigned long long miss = 0;
  int p = A.lo[dir];
  // the last coarse run: its level, box, cell pointer and the stride along dir in that FAB.  The next position starts the next cell of
  // that level; while it lies in the same box only the finer levels are asked (one round of lookups), and the cell's values -- whose
  // address is known -- are loaded beside them instead of behind a new owner -> box -> offset -> value chain
  bool chave = false;
  int clev = -1, cspan = 1, chi = 0;
  const double* cptr = nullptr;
  long long ccs = 0, cstr = 0;
  while (p <= last) {
    q[dir] = p;
    PlSrc src;
    double v[NC];
    bool fast = false;
    if (chave && coarsen_idx(p, cspan) <= chi) {
      const double* nptr = cptr + cstr;
#pragma unroll
      for (int c = 0; c < NC; ++c) v[c] = nptr[(long long)comp[c] * ccs];
      if (!pl_finer_hit(A, q, clev)) {
        fast = true;
        cptr = nptr;
        src.p = nptr;
        src.cs = ccs;
        src.lev = clev;
        src.span = cspan;
      }
    }
    if (!fast) {
      src = pl_resolve(A, q);
      chave = src.lev >= 0 && src.lev != F;
      if (chave) {
        clev = src.lev;
        cspan = src.span;
        chi = src.B.hi[dir];
        cptr = src.p;
        ccs = src.cs;
        const long long nx = src.B.hi[0] - src.B.lo[0] + 1 + 2 * src.ng, ny = src.B.hi[1] - src.B.lo[1] + 1 + 2 * src.ng;
        cstr = dir == 0 ? 1 : (dir == 1 ? nx : nx * ny);
      }
      if (src.lev != F) {
#pragma unroll
        for (int c = 0; c < NC; ++c) v[c] = src.p ? src.p[(long long)comp[c] * src.cs] : std::numeric_limits<double>::quiet_NaN();
      }
    }
    int e;  // last position of the run
    long long sd = 0;
    if (src.lev == F) {
      e = src.B.hi[dir];
      const long long nx = src.B.hi[0] - src.B.lo[0] + 1 + 2 * src.ng, ny = src.B.hi[1] - src.B.lo[1] + 1 + 2 * src.ng;
      sd = dir == 0 ? 1 : (dir == 1 ? nx : nx * ny);
    } else {
      e = (coarsen_idx(p, src.span) + 1) * src.span - 1;
    }
    e = min(e, last);
    if (!src.p) miss += (unsigned long long)(e - p + 1);
    const double* ptr = src.p;
    while (p <= e) {
      const int e2 = min(e, cend);
      if (src.lev == F) {
        for (; p <= e2; ++p, ptr += sd) {
#pragma unroll
          for (int c = 0; c < NC; ++c) s[c] = s[c] + ptr[(long long)comp[c] * src.cs];
        }
      } else {
        for (; p <= e2; ++p) {
#pragma unroll
          for (int c = 0; c < NC; ++c) s[c] = s[c] + v[c];
        }
      }
      if (e2 == cend) {  // the chunk is complete: ParallelAdd in box order
#pragma unroll
        for (int c = 0; c < NC; ++c) { S[c] = S[c] + s[c]; s[c] = 0.0; }
        ++ci;
        cend = ci < A.nchunk ? A.chunk_end[ci] : INT_MAX;
      }
    }
  }
  if (miss && A.c0 == 0) atomicAdd(A.nosrc, miss);  // counted once, not once per group of components
  const long long np = (long long)A.W * A.H, px = (long long)y * A.W + x;
#pragma unroll
  for (int c = 0; c < NC; ++c) A.out[(long long)(A.c0 + c) * np + px] = S[c];
}

__global__ __launch_bounds__(256) void k_plane_slice(const PlArgs A) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= A.W || y >= A.H) return;
  int q[3];
  pl_pixel_cell(A, x, y, q);
  q[A.dir] = A.lo[A.dir];
  const PlSrc src = pl_resolve(A, q);
  if (!src.p && A.c0 == 0) atomicAdd(A.nosrc, 1ull);
  const long long np = (long long)A.W * A.H, px = (long long)y * A.W + x;
  for (int c = 0; c < A.nc; ++c) A.out[(long long)(A.c0 + c) * np + px] = src.p ? src.p[(long long)A.comp[c] * src.cs] : std::numeric_limits<double>::quiet_NaN();
}

// part[b] / part[PA_PL_MMB + b]: min / max of the non-NaN values workgroup b saw (+inf / -inf: none)
__global__ __launch_bounds__(256) void k_plane_minmax(const double* __restrict__ v, long long n, double* __restrict__ part) {
  __shared__ double smn[256], smx[256];
  double mn = std::numeric_limits<double>::infinity(), mx = -std::numeric_limits<double>::infinity();
  bool any = false;
  for (long long q = blockIdx.x * 256ll + threadIdx.x; q < n; q += (long long)gridDim.x * 256) {
    const double a = v[q];
    if (a == a) {
      mn = a < mn ? a : mn;
      mx = a > mx ? a : mx;
      any = true;
    }
  }
  if (!any) { mn = std::numeric_limits<double>::quiet_NaN(); mx = mn; }  // NaN: this thread saw no value
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      const double a = smn[threadIdx.x + w], b = smx[threadIdx.x + w];
      if (a == a) {
        const double c = smn[threadIdx.x], d = smx[threadIdx.x];
        smn[threadIdx.x] = (c == c && c < a) ? c : a;
        smx[threadIdx.x] = (d == d && d > b) ? d : b;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[blockIdx.x] = smn[0];
    part[PA_PL_MMB + blockIdx.x] = smx[0];
  }
}

// pixelizeData (avgToPlane.cpp:233-270, slicePlot.cpp:95-132)
__global__ __launch_bounds__(256) void k_plane_pixelize(const double* __restrict__ v, long long n, double mn, double mx, unsigned char* __restrict__ pix) {
  const long long q = blockIdx.x * 256ll + threadIdx.x;
  if (q >= n) return;
  const double del = mx - mn;
  const double t = (v[q] - mn) / del;
  int level = 0;
  if (t > 0.0) level = (int)(255.0 * (t < 1.0 ? t : 1.0));
  pix[q] = (unsigned char)level;
}

static void pl_free(pa_plane* h) {
  if (h->d_chunk_end) (void)hipFree(h->d_chunk_end);
  if (h->d_out) (void)hipFree(h->d_out);
  if (h->d_part) (void)hipFree(h->d_part);
  if (h->d_pix) (void)hipFree(h->d_pix);
  if (h->d_nosrc) (void)hipFree(h->d_nosrc);
}

extern "C" pa_plane* pa_plane_create(pa_ctx* ctx, int ncomp, int dir, const pa_box* subbox, int max_grid_size) {
  PaBind bind_(ctx);
  auto fail = [&](const char* m) -> pa_plane* { pa_fail(ctx, m); return nullptr; };
  if (!ctx || !subbox) return fail("pa_plane_create: null argument");
  if (ncomp < 1) return fail("pa_plane_create: no component");
  if (dir < 0 || dir > 2) return fail("pa_plane_create: dir must be 0, 1 or 2");
  if (max_grid_size < 0) return fail("pa_plane_create: negative max_grid_size");
  for (int d = 0; d < 3; ++d)
    if (subbox->hi[d] < subbox->lo[d]) return fail("pa_plane_create: empty sub-box");
  if (max_grid_size == 0 && subbox->hi[dir] != subbox->lo[dir]) return fail("pa_plane_create: a slice's box is one cell thick along dir");
  const int d0 = dir == 0 ? 1 : 0, d1 = dir == 2 ? 1 : 2;
  const long long W = (long long)subbox->hi[d0] - subbox->lo[d0] + 1, H = (long long)subbox->hi[d1] - subbox->lo[d1] + 1;
  if (W > 65535ll * 64 || H > 65535 || W * H > (1ll << 31) - 1) return fail("pa_plane_create: the plane is too large");
  pa_plane* h = new pa_plane;
  h->ctx = ctx;
  h->ncomp = ncomp;
  h->dir = dir;
  h->slice = max_grid_size == 0;
  for (int d = 0; d < 3; ++d) { h->lo[d] = subbox->lo[d]; h->hi[d] = subbox->hi[d]; }
  h->W = (int)W;
  h->H = (int)H;
  if (h->slice) {
    h->chunk_end.push_back(h->hi[dir]);
  } else {  // pa::max_size along dir (BoxArray::maxSize: even split)
    const int len = h->hi[dir] - h->lo[dir] + 1, parts = (len + max_grid_size - 1) / max_grid_size, base = len / parts, rem = len % parts;
    int s = h->lo[dir];
    for (int p = 0; p < parts; ++p) {
      s += base + (p < rem ? 1 : 0);
      h->chunk_end.push_back(s - 1);
    }
  }
  const size_t np = (size_t)W * (size_t)H;
  if (hipMalloc(&h->d_chunk_end, sizeof(int) * h->chunk_end.size()) != hipSuccess ||
      hipMalloc(&h->d_out, sizeof(double) * np * (size_t)ncomp) != hipSuccess || hipMalloc(&h->d_part, sizeof(double) * 2 * PA_PL_MMB) != hipSuccess ||
      hipMalloc(&h->d_pix, np) != hipSuccess || hipMalloc(&h->d_nosrc, sizeof(unsigned long long)) != hipSuccess ||
      hipMemcpy(h->d_chunk_end, h->chunk_end.data(), sizeof(int) * h->chunk_end.size(), hipMemcpyHostToDevice) != hipSuccess) {
    pl_free(h);
    delete h;
    return fail("pa_plane_create: out of device memory");
  }
  return h;
}

extern "C" void pa_plane_destroy(pa_plane* h) {
  if (!h) return;
  PaBind bind_(h->ctx);
  if (h->ctx && h->ctx->stream) (void)hipStreamSynchronize(h->ctx->stream);
  pl_free(h);
  delete h;
}

extern "C" int pa_plane_run(pa_ctx* ctx, pa_plane* h, int nlev, const pa_mf* const* levels, const int32_t* ratios, const int32_t* comps) {
  PaBind bind_(ctx);
  if (!ctx || !h || !levels || !comps) return pa_fail(ctx, "pa_plane_run: null argument");
  h->ran = false;
  if (nlev < 1 || nlev > PA_PL_MAXLEV) return pa_fail(ctx, "pa_plane_run: 1 to " + std::to_string(PA_PL_MAXLEV) + " levels");
  if (nlev > 1 && !ratios) return pa_fail(ctx, "pa_plane_run: null refinement ratios");
  PlArgs A{};
  A.nlev = nlev;
  for (int l = 0; l < nlev; ++l) {
    const pa_mf* m = levels[l];
    if (!m) return pa_fail(ctx, "pa_plane_run: null level");
    if (m->lev->nranks > 1 || m->lev->nremote > 0) return pa_fail(ctx, "pa_plane_run: sharded levels are not supported");
    for (int c = 0; c < h->ncomp; ++c)
      if (comps[c] < 0 || comps[c] >= m->ncomp) return pa_fail(ctx, "pa_plane_run: component out of range");
    A.L[l] = m->lev->view;
    A.M[l] = m->view;
    A.ratio[l] = 1;
    if (l > 0) {
      const pa_level *Fl = m->lev, *C = levels[l - 1]->lev;
      const int r = ratios[l - 1];
      if (r < 2) return pa_fail(ctx, "pa_plane_run: a refinement ratio must be at least 2");
      for (int d = 0; d < 3; ++d)
        if ((long long)Fl->domlo[d] != (long long)C->domlo[d] * r || (long long)Fl->domhi[d] + 1 != ((long long)C->domhi[d] + 1) * r)
          return pa_fail(ctx, "pa_plane_run: the domain of level " + std::to_string(l) + " is not the coarser one refined by the ratio");
      A.ratio[l] = r;
    }
  }
  const pa_level* Fine = levels[nlev - 1]->lev;
  for (int d = 0; d < 3; ++d)
    if (h->lo[d] < Fine->domlo[d] || h->hi[d] > Fine->domhi[d]) return pa_fail(ctx, "pa_plane_run: the sub-box is not inside the finest level's domain");
  A.dir = h->dir;
  A.nchunk = (int)h->chunk_end.size();
  A.ncomp = h->ncomp;
  A.W = h->W;
  A.H = h->H;
  for (int d = 0; d < 3; ++d) { A.lo[d] = h->lo[d]; A.hi[d] = h->hi[d]; }
  A.chunk_end = h->d_chunk_end;
  A.out = h->d_out;
  A.nosrc = h->d_nosrc;
  PA_HIP(hipMemsetAsync(h->d_nosrc, 0, sizeof(unsigned long long), ctx->stream));
  const dim3 grid((unsigned)((h->W + 63) / 64), (unsigned)((h->H + 3) / 4));
  const int per = h->slice ? PA_PL_SC : PA_PL_NC;
  for (int c0 = 0; c0 < h->ncomp; c0 += per) {
    const int nc = std::min(per, h->ncomp - c0);
    A.c0 = c0;
    A.nc = nc;
    for (int c = 0; c < PA_PL_SC; ++c) A.comp[c] = c < nc ? comps[c0 + c] : 0;
    if (h->slice) {
      hipLaunchKernelGGL(k_plane_slice, grid, dim3(64, 4), 0, ctx->stream, A);
    } else {
      if (nc == 1) hipLaunchKernelGGL(k_plane_sum<1>, grid, dim3(64, 4), 0, ctx->stream, A);
      else if (nc == 2) hipLaunchKernelGGL(k_plane_sum<2>, grid, dim3(64, 4), 0, ctx->stream, A);
      else if (nc == 3) hipLaunchKernelGGL(k_plane_sum<3>, grid, dim3(64, 4), 0, ctx->stream, A);
      else hipLaunchKernelGGL(k_plane_sum<4>, grid, dim3(64, 4), 0, ctx->stream, A);
    }
  }
  PA_HIP(hipGetLastError());
  h->ran = true;
  return 0;
}

extern "C" int pa_plane_read(pa_ctx* ctx, const pa_plane* h, double* out, int64_t* nosrc) {
  PaBind bind_(ctx);
  if (!ctx || !h || !out) return pa_fail(ctx, "pa_plane_read: null argument");
  if (!h->ran) return pa_fail(ctx, "pa_plane_read: no completed pa_plane_run");
  unsigned long long n = 0;
  PA_HIP(hipStreamSynchronize(ctx->stream));
  PA_HIP(hipMemcpy(out, h->d_out, sizeof(double) * (size_t)h->W * (size_t)h->H * (size_t)h->ncomp, hipMemcpyDeviceToHost));
  PA_HIP(hipMemcpy(&n, h->d_nosrc, sizeof n, hipMemcpyDeviceToHost));
  if (nosrc) *nosrc = (int64_t)n;
  return 0;
}

extern "C" int pa_plane_minmax(pa_ctx* ctx, const pa_plane* h, int comp, double* mn, double* mx) {
  PaBind bind_(ctx);
  if (!ctx || !h || !mn || !mx) return pa_fail(ctx, "pa_plane_minmax: null argument");
  if (!h->ran) return pa_fail(ctx, "pa_plane_minmax: no completed pa_plane_run");
  if (comp < 0 || comp >= h->ncomp) return pa_fail(ctx, "pa_plane_minmax: component out of range");
  const long long np = (long long)h->W * h->H;
  const unsigned nb = (unsigned)std::min<long long>(PA_PL_MMB, (np + 255) / 256);
  hipLaunchKernelGGL(k_plane_minmax, dim3(nb), dim3(256), 0, ctx->stream, h->d_out + (size_t)comp * (size_t)np, np, h->d_part);
  PA_HIP(hipGetLastError());
  double part[2 * PA_PL_MMB];
  PA_HIP(hipMemcpyAsync(part, h->d_part, sizeof part, hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipStreamSynchronize(ctx->stream));
  bool any = false;
  double a = 0.0, b = 0.0;
  for (unsigned q = 0; q < nb; ++q) {
    const double pm = part[q], px = part[PA_PL_MMB + q];
    if (pm != pm) continue;
    a = (any && a < pm) ? a : pm;
    b = (any && b > px) ? b : px;
    any = true;
  }
  if (!any) return pa_fail(ctx, "pa_plane_minmax: the plane holds no value that is not a NaN");
  *mn = a;
  *mx = b;
  return 0;
}

extern "C" int pa_plane_pixelize(pa_ctx* ctx, const pa_plane* h, int comp, double mn, double mx, uint8_t* levels) {
  PaBind bind_(ctx);
  if (!ctx || !h || !levels) return pa_fail(ctx, "pa_plane_pixelize: null argument");
  if (!h->ran) return pa_fail(ctx, "pa_plane_pixelize: no completed pa_plane_run");
  if (comp < 0 || comp >= h->ncomp) return pa_fail(ctx, "pa_plane_pixelize: component out of range");
  const long long np = (long long)h->W * h->H;
  hipLaunchKernelGGL(k_plane_pixelize, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, ctx->stream, h->d_out + (size_t)comp * (size_t)np, np, mn, mx, h->d_pix);
  PA_HIP(hipGetLastError());
  PA_HIP(hipMemcpyAsync(levels, h->d_pix, (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}
