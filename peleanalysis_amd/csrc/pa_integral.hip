// pa_integral.hip -- line, plane and volume integrals of plotfile components over the composite AMR hierarchy (integral.cpp) and the
// moments of rmsVel.cpp: the kernel family that projects a level onto a point (kind 3), a line (kind 2) or a plane (kind 1).
//
// NUMERICS: the contract of pa_stats.hip, through the same limb arithmetic (pa_fixed192.h).  Every sum is a 192-bit
// fixed-point integer scaled from the magnitudes declared at begin, added with 64-bit integer atomics and rounded once at read.  Row 0
// (the measure) is an integer COUNT of cells per level; read multiplies it by the level's weight in fixed point, so it is exact.
// A term that is not finite cannot be held in fixed point: it sets one of three sticky flags of its slot and row (NaN, +inf, -inf), and
// read returns what IEEE addition returns in any order.
//
// LAYOUT: every level is accumulated in ITS OWN index space -- ldir / R_l slots (kind 2), (ldir1 / R_l) x (ldir2 / R_l) pixels (kind 1) --
// in a table of its own: per slot one count and 3 limbs per row.  read adds the tables of all levels in fixed point, a coarse slot
// into the R_l (or R_l x R_l) fine slots under it, and only then rounds.
//
// FEW ATOMICS: a thread keeps one private run (slot, count, sums in registers) and marches 16 cells under a 256-cell piece of a plane
// whose fast axis is x (coalesced loads).  The march direction is chosen so that the slot does not change along it where such a
// direction exists (kind 2, dir = z marches in y; kind 1 marches along dir unless dir = x).  Where the lanes of a wavefront share the
// slot -- kind 3; kind 2 with dir != x; kind 1 with dir = x -- the runs are summed over the wavefront in integers first (at the end
// of the kernel, of the tile, or of the step) and one lane adds.  Runs go to a table of the level in LDS (kind 3; kind 2 while the
// table is small and the wavefront sum does not already leave one add per tile), which is added to the global one once per workgroup
// and touched slot; otherwise to the global table.  `uncombined` selects one set of
// global atomics per cell, with identical bits (tools/integral_bench.py).
#include "pa_celltiles.h"
#include <cmath>
#include <cstring>

#define PA_INT_MAXV 8
#define PA_INT_LDS_MAX (32 * 1024)
enum { PA_IF_NAN = 1, PA_IF_PINF = 2, PA_IF_NINF = 4 };
enum { PA_WR_NONE = 0, PA_WR_END = 1, PA_WR_TILE = 2, PA_WR_STEP = 3 };  // when the wavefront's runs are summed before they are added

struct IntLevelTab {
  int R = 1;
  double w = 0.0;
  int n1 = 1, n2 = 1;  // slots of the level along dir1 (kind 2: along dir) and dir2
  size_t nslots = 0;
  u64* d_tab = nullptr;       // [nslots][stride]: count, then 3 limbs per row 1 ..
  unsigned* d_flg = nullptr;  // [nslots][nrows - 1]: sticky PA_IF_* of the terms that were not finite
};

struct pa_integral {
  pa_ctx* ctx = nullptr;
  int nvars = 0, kind = 0, dir = 0, dir1 = 0, dir2 = 0, squares = 0, nrows = 0, stride = 0;
  DBox dom;  // the domain box of the finest level that is integrated
  bool begun = false;
  double w_max = 0.0;
  int s_w = 0;
  int s_row[2 * PA_INT_MAXV] = {};
  std::vector<IntLevelTab> tabs;
  int* d_flags = nullptr;
  CellTileTable tiles;  // of the level being added
};

struct IntArgs {
  DLevelView L, F;
  DMFView M;
  CellTab T;
  int has_fine, ratio;
  int kind, dir, dir1, dir2;
  CellWalk W;
  int wr, mode;  // mode 0: every cell -> global table; 1: runs -> global table; 2: runs -> LDS table
  int lo[3], n2, nslots;
  int nvars, nrows, stride;
  int ccomp;
  double cmin, cmax, w;
  int srow[2 * PA_INT_MAXV];
  u64* tab;
  unsigned* flg;
  int* flags;
};

// one run of a thread (or of a wavefront, or one cell) into a table of the level's layout, in LDS or in HBM
// the table row (after the measure) of register row r, or -1: the squares sit behind the NV rows of the template in registers and
// behind the nvars rows in the table
template <int NV, int NR>
__device__ __forceinline__ int int_trow(const IntArgs& A, int r) {
  if (r < NV) return r < A.nvars ? r : -1;
  return r - NV < A.nvars ? A.nvars + (r - NV) : -1;
}
template <int NV, int NR>
__device__ __forceinline__ void int_flush(u64* tab, const IntArgs& A, int key, u64& cnt, U192 (&s)[NR]) {
  u64* e = tab + (long long)key * A.stride;
  atomicAdd(e, cnt);
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int tr = int_trow<NV, NR>(A, r);
    if (tr < 0) continue;
    if (!u192_zero(s[r])) u192_atomic_add(e + 1 + 3 * tr, s[r]);
    s[r] = {{0, 0, 0}};
  }
  cnt = 0;
}

// the runs of the wavefront: summed in integers and added by one lane when the lanes that hold a run share its slot, else lane by lane.
// Every lane of the wavefront calls this.
template <int NV, int NR>
__device__ __forceinline__ void int_wave_flush(u64* tab, const IntArgs& A, int& key, u64& cnt, U192 (&s)[NR]) {
  const bool has = cnt > 0;
  const u64 m = __ballot(has);
  if (m == 0) return;
  const int first = __ffsll((long long)m) - 1;
  const int k0 = __shfl(key, first);
  const bool uni = __ballot(has && key != k0) == 0;
  if (uni) {
    cnt = wave_sum_u64(cnt);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      if (int_trow<NV, NR>(A, r) < 0) continue;
      s[r] = wave_sum_u192(s[r]);
    }
    if ((int)(threadIdx.x & 63) == first) {
      int_flush<NV, NR>(tab, A, k0, cnt, s);
    } else {
      cnt = 0;
#pragma unroll
      for (int r = 0; r < NR; ++r) s[r] = {{0, 0, 0}};
    }
  } else if (has) {
    int_flush<NV, NR>(tab, A, key, cnt, s);
  }
}

// the term t of row r (0-based after the measure) of slot `slot`: into the run, or -- not finite -- into the slot's sticky flags
__device__ __forceinline__ void int_term(U192& acc, double t, int s, int& flag, const IntArgs& A, int slot, int r) {
  const long long bits = __double_as_longlong(t);
  if (((bits >> 52) & 0x7ff) == 0x7ff) {
    const unsigned f = (bits & ((1ll << 52) - 1)) ? PA_IF_NAN : (bits < 0 ? PA_IF_NINF : PA_IF_PINF);
    atomicOr(A.flg + (long long)slot * (A.nrows - 1) + r, f);
    return;
  }
  u192_add(acc, to_fixed(t, s, flag));
}

template <int NV, bool SQ>
__global__ __launch_bounds__(256) void k_integral(IntArgs A) {
  extern __shared__ u64 lds[];
  constexpr int NR = SQ ? 2 * NV : NV;
  u64* tab = A.tab;
  if (A.mode == 2) {
    const int nw = A.nslots * A.stride;
    for (int z = threadIdx.x; z < nw; z += 256) lds[z] = 0;
    __syncthreads();
    tab = lds;
  }
  int key = -1, flag = 0;
  u64 cnt = 0;
  U192 s[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) s[r] = {{0, 0, 0}};
  for (int t = blockIdx.x; t < A.T.ntiles; t += gridDim.x) {
    const CellTile c = celltile_decode(A.T, A.W, A.L.boxes, t, threadIdx.x);  // a thread without a cell (!c.ok) marches along: the wavefront sums need every lane
    const long long nxg = c.B.hi[0] - c.B.lo[0] + 1 + 2 * A.M.ng, nyg = c.B.hi[1] - c.B.lo[1] + 1 + 2 * A.M.ng,
                    nzg = c.B.hi[2] - c.B.lo[2] + 1 + 2 * A.M.ng;
    const long long cs = pa_cstride(nxg * nyg * nzg, A.M.ncomp);
    int idx[3];
    celltile_cell(A.W, c, c.m0, idx);
    const long long ms = A.W.march == 2 ? nxg * nyg : nxg;
    const double* f = A.M.data + A.M.off[c.b] + ((long long)(idx[2] - c.B.lo[2] + A.M.ng) * nyg + (idx[1] - c.B.lo[1] + A.M.ng)) * nxg +
                      (idx[0] - c.B.lo[0] + A.M.ng);
    for (int m = c.m0; m <= c.m1; ++m, f += ms) {  // the bounds are the same for every thread of the workgroup
      idx[A.W.march] = m;
      // integral.cpp:425-436: the cell's refined image has an owner on the next finer level
      bool take = c.ok;
      if (take && A.has_fine) take = !covered_by(A.F, A.ratio, idx[0], idx[1], idx[2]);
      if (take && A.ccomp >= 0) {  // :28, :89, :133 -- a NaN fails both comparisons
        const double vc = f[A.ccomp * cs];
        take = vc >= A.cmin && vc < A.cmax;
      }
      if (take) {
        int slot = 0;
        if (A.kind == 2) slot = idx[A.dir] - A.lo[A.dir];
        else if (A.kind == 1) slot = (idx[A.dir1] - A.lo[A.dir1]) * A.n2 + (idx[A.dir2] - A.lo[A.dir2]);
        if (A.mode != 0 && slot != key && cnt) int_flush<NV, NR>(tab, A, key, cnt, s);
        key = slot;
        cnt += 1;
#pragma unroll
        for (int n = 0; n < NV; ++n) {
          if (n >= A.nvars) continue;
          const double v = f[n * cs];
          int_term(s[n], A.w * v, A.srow[n], flag, A, slot, n);  // :36, :96, :136: one rounded product
          if (SQ) int_term(s[SQ ? NV + n : 0], (v * v) * A.w, A.srow[A.nvars + n], flag, A, slot, A.nvars + n);  // rmsVel.cpp:109-111
        }
        if (A.mode == 0) int_flush<NV, NR>(tab, A, key, cnt, s);
      }
      if (A.wr == PA_WR_STEP) int_wave_flush<NV, NR>(tab, A, key, cnt, s);
    }
    if (A.wr == PA_WR_TILE) int_wave_flush<NV, NR>(tab, A, key, cnt, s);
  }
  if (A.wr != PA_WR_NONE) int_wave_flush<NV, NR>(tab, A, key, cnt, s);
  else if (cnt) int_flush<NV, NR>(tab, A, key, cnt, s);
  if (A.mode == 2) celltab_merge(lds, A.tab, A.nslots, A.nrows, A.stride, [](const u64*, u64*) {});  // one add per touched slot and row
  if (flag) atomicOr(A.flags, flag);
}

template <int NV, bool SQ>
static void integral_launch(pa_ctx* ctx, const IntArgs& A, unsigned grid, size_t lds_bytes) {
  hipLaunchKernelGGL((k_integral<NV, SQ>), dim3(grid), dim3(256), lds_bytes, ctx->stream, A);
}

static void integral_free_tabs(pa_integral* I) {
  for (IntLevelTab& T : I->tabs) {
    if (T.d_tab) (void)hipFree(T.d_tab);
    if (T.d_flg) (void)hipFree(T.d_flg);
  }
  I->tabs.clear();
}

extern "C" void pa_integral_destroy(pa_integral* I) {
  if (!I) return;
  PaBind bind_(I->ctx);
  if (I->ctx && I->ctx->stream) (void)hipStreamSynchronize(I->ctx->stream);
  integral_free_tabs(I);
  if (I->d_flags) (void)hipFree(I->d_flags);
  I->tiles.release();
  delete I;
}

// integral.cpp:442-449, :497-501, :520 (the output arrays) and rmsVel.cpp:82 (the seven sums)
extern "C" pa_integral* pa_integral_create(pa_ctx* ctx, int nvars, int kind, int dir, const pa_box* domain, int squares) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  if (!domain) { pa_fail(ctx, "pa_integral_create: null domain"); return nullptr; }
  if (nvars < 1 || nvars > PA_INT_MAXV) { pa_fail(ctx, "pa_integral_create: 1 to " + std::to_string(PA_INT_MAXV) + " variables per accumulator"); return nullptr; }
  if (kind < 1 || kind > 3) { pa_fail(ctx, "pa_integral_create: kind must be 1 (line), 2 (plane) or 3 (volume)"); return nullptr; }
  if (dir < 0 || dir > 2) { pa_fail(ctx, "pa_integral_create: dir must be 0, 1 or 2"); return nullptr; }
  for (int d = 0; d < 3; ++d)
    if (domain->hi[d] < domain->lo[d]) { pa_fail(ctx, "pa_integral_create: empty domain"); return nullptr; }
  pa_integral* I = new pa_integral;
  I->ctx = ctx;
  I->nvars = nvars;
  I->kind = kind;
  I->dir = dir;
  I->dir1 = (dir + 1) % 3;
  I->dir2 = (dir + 2) % 3;
  I->squares = squares ? 1 : 0;
  I->nrows = 1 + nvars * (squares ? 2 : 1);
  I->stride = 1 + 3 * (I->nrows - 1);
  for (int d = 0; d < 3; ++d) { I->dom.lo[d] = domain->lo[d]; I->dom.hi[d] = domain->hi[d]; }
  if (hipMalloc((void**)&I->d_flags, sizeof(int)) != hipSuccess) {
    pa_fail(ctx, "pa_integral_create: out of device memory");
    pa_integral_destroy(I);
    return nullptr;
  }
  return I;
}

static long long integral_slots(const pa_integral* I) {
  const long long l0 = I->dom.hi[I->dir] - I->dom.lo[I->dir] + 1, l1 = I->dom.hi[I->dir1] - I->dom.lo[I->dir1] + 1,
                  l2 = I->dom.hi[I->dir2] - I->dom.lo[I->dir2] + 1;
  return I->kind == 3 ? 1 : (I->kind == 2 ? l0 : l1 * l2);
}

extern "C" int64_t pa_integral_slots(const pa_integral* I) { return I ? integral_slots(I) : 0; }

extern "C" int pa_integral_begin(pa_ctx* ctx, pa_integral* I, double w_max, const double* vabs) {
  PaBind bind_(ctx);
  if (!ctx || !I || !vabs) return pa_fail(ctx, "pa_integral_begin: bad argument");
  if (!(w_max > 0.0) || !std::isfinite(w_max)) return pa_fail(ctx, "pa_integral_begin: w_max must be positive and finite");
  if (check_magnitudes(ctx, "pa_integral_begin", "variable", vabs, I->nvars)) return 1;
  for (int n = 0; n < I->nvars; ++n) {
    I->s_row[n] = scale_of(w_max * vabs[n]);
    if (I->squares) I->s_row[I->nvars + n] = scale_of(w_max * vabs[n] * vabs[n]);
  }
  I->w_max = w_max;
  I->s_w = scale_of(w_max);
  PA_HIP(hipStreamSynchronize(ctx->stream));
  integral_free_tabs(I);
  PA_HIP(hipMemsetAsync(I->d_flags, 0, sizeof(int), ctx->stream));
  I->begun = true;
  return 0;
}

// integrate1d / integrate2d / integrate3d for ONE level (integral.cpp:24-44, :85-101, :129-140) and the cell loop of rmsVel.cpp:83-115
extern "C" int pa_integral_add_level(pa_ctx* ctx, pa_integral* I, const pa_mf* vars, const pa_level* finer, int ratio, int R, double w, int ccomp,
                                     double cmin, double cmax, int uncombined) {
  PaBind bind_(ctx);
  if (!ctx || !I || !vars) return pa_fail(ctx, "pa_integral_add_level: bad argument");
  if (!I->begun) return pa_fail(ctx, "pa_integral_add_level: pa_integral_begin has not been called");
  if (vars->ncomp < I->nvars) return pa_fail(ctx, "pa_integral_add_level: the multifab must hold " + std::to_string(I->nvars) + " components");
  if (finer && ratio < 1) return pa_fail(ctx, "pa_integral_add_level: bad refinement ratio");
  if (R < 1) return pa_fail(ctx, "pa_integral_add_level: R_l must be at least 1");
  if (!(w > 0.0) || !(w <= I->w_max)) return pa_fail(ctx, "pa_integral_add_level: the weight must be positive and at most the w_max given to pa_integral_begin");
  if (ccomp >= I->nvars) return pa_fail(ctx, "pa_integral_add_level: the condition component must be one of the " + std::to_string(I->nvars) + " variables");
  if (ccomp >= 0 && (cmin != cmin || cmax != cmax)) return pa_fail(ctx, "pa_integral_add_level: cMin or cMax is NaN");
  const pa_level* lev = vars->lev;
  if (lev->nranks > 1) return pa_fail(ctx, "pa_integral_add_level: sharded levels are not supported");
  for (int d = 0; d < 3; ++d)
    if ((long long)lev->domlo[d] * R != I->dom.lo[d] || ((long long)lev->domhi[d] + 1) * R - 1 != I->dom.hi[d])
      return pa_fail(ctx, "pa_integral_add_level: the level's domain times R_l is not the domain the accumulator was created for");
  for (const DBox& B : lev->boxes)
    for (int d = 0; d < 3; ++d)
      if (B.lo[d] < lev->domlo[d] || B.hi[d] > lev->domhi[d]) return pa_fail(ctx, "pa_integral_add_level: a box lies outside the level's domain");
  if (lev->boxes.empty()) return 0;
  // the level's table
  IntLevelTab* T = nullptr;
  for (IntLevelTab& t : I->tabs)
    if (t.R == R && t.w == w) T = &t;
  if (!T) {
    if (I->tabs.size() >= 64) return pa_fail(ctx, "pa_integral_add_level: more than 64 distinct levels");
    IntLevelTab t;
    t.R = R;
    t.w = w;
    if (I->kind == 2) t.n1 = lev->domhi[I->dir] - lev->domlo[I->dir] + 1;
    if (I->kind == 1) { t.n1 = lev->domhi[I->dir1] - lev->domlo[I->dir1] + 1; t.n2 = lev->domhi[I->dir2] - lev->domlo[I->dir2] + 1; }
    t.nslots = (size_t)t.n1 * (size_t)t.n2;
    if (t.nslots * (size_t)I->stride >= (1ull << 31)) return pa_fail(ctx, "pa_integral_add_level: the output is too large");
    PA_HIP(hipMalloc((void**)&t.d_tab, t.nslots * I->stride * sizeof(u64)));
    if (hipMalloc((void**)&t.d_flg, t.nslots * (I->nrows - 1) * sizeof(unsigned)) != hipSuccess) {
      (void)hipFree(t.d_tab);
      return pa_fail(ctx, "pa_integral_add_level: out of device memory");
    }
    I->tabs.push_back(t);
    T = &I->tabs.back();
    PA_HIP(hipMemsetAsync(T->d_tab, 0, T->nslots * I->stride * sizeof(u64), ctx->stream));
    PA_HIP(hipMemsetAsync(T->d_flg, 0, T->nslots * (I->nrows - 1) * sizeof(unsigned), ctx->stream));
  }
  IntArgs A;
  A.L = lev->view;
  A.M = vars->view;
  fine_cover(lev, finer, ratio, A.F, A.has_fine, A.ratio);
  A.kind = I->kind; A.dir = I->dir; A.dir1 = I->dir1; A.dir2 = I->dir2;
  // the march direction: one along which the slot does not change, where there is one (x stays the lane direction)
  int march = 2, aax = 1, kt = 16;
  A.wr = PA_WR_NONE;
  if (I->kind == 3) A.wr = PA_WR_END;
  else if (I->kind == 2) {
    if (I->dir == 2) { march = 1; aax = 2; }
    if (I->dir != 0) A.wr = PA_WR_TILE; else kt = 128;  // dir = x: the lane is the slot; long runs, few adds
  } else {
    if (I->dir == 1) { march = 1; aax = 2; }
    if (I->dir == 0) A.wr = PA_WR_STEP; else kt = 64;
  }
  // Where the table goes: kind 3 is one slot in LDS.  Kind 2 with dir != x and rows of whole wavefronts (every box a multiple of 64
  // cells wide) leaves one add per wavefront and tile: straight to HBM, no LDS that would cost occupancy.  Otherwise the level's
  // table lives in LDS while it is small enough to keep five workgroups on a CU; kind 1 (a plane) never fits.
  bool rows_of_waves = true;
  for (const DBox& B : lev->boxes) rows_of_waves = rows_of_waves && ((B.hi[0] - B.lo[0] + 1) % 64 == 0);
  const size_t lds_bytes = T->nslots * I->stride * sizeof(u64);
  A.mode = 1;
  if (I->kind == 3) A.mode = 2;
  else if (I->kind == 2 && !(I->dir != 0 && rows_of_waves) && lds_bytes <= PA_INT_LDS_MAX) A.mode = 2;
  if (uncombined) A.mode = 0;
  if (uncombined) A.wr = PA_WR_NONE;
  for (int d = 0; d < 3; ++d) A.lo[d] = lev->domlo[d];
  A.n2 = T->n2;
  A.nslots = (int)T->nslots;
  A.nvars = I->nvars; A.nrows = I->nrows; A.stride = I->stride;
  A.ccomp = ccomp < 0 ? -1 : ccomp;
  A.cmin = cmin; A.cmax = cmax; A.w = w;
  for (int r = 0; r < 2 * PA_INT_MAXV; ++r) A.srow[r] = I->s_row[r];
  A.tab = T->d_tab; A.flg = T->d_flg; A.flags = I->d_flags;
  A.W = {march, aax, kt};
  if (I->tiles.build(ctx, lev, aax, march, kt, "pa_integral", A.T)) return 1;
  const unsigned grid = (unsigned)std::min<long long>(A.T.ntiles, 1024);
  const size_t lb = A.mode == 2 ? lds_bytes : 0;
  const int nv = I->nvars;
  if (I->squares) {
    if (nv <= 1) integral_launch<1, true>(ctx, A, grid, lb);
    else if (nv <= 4) integral_launch<4, true>(ctx, A, grid, lb);
    else integral_launch<PA_INT_MAXV, true>(ctx, A, grid, lb);
  } else {
    if (nv <= 1) integral_launch<1, false>(ctx, A, grid, lb);
    else if (nv <= 4) integral_launch<4, false>(ctx, A, grid, lb);
    else integral_launch<PA_INT_MAXV, false>(ctx, A, grid, lb);
  }
  PA_HIP(hipGetLastError());
  return 0;
}

// the raw sums before the avg division (integral.cpp:51-58, :107-112, :143-147; rmsVel.cpp:116-122): out[row][slot], rows = the measure,
// w * v of every variable and, with squares, (v * v) * w of every variable
extern "C" int pa_integral_read(pa_ctx* ctx, const pa_integral* I, double* out) {
  PaBind bind_(ctx);
  if (!ctx || !I || !out) return pa_fail(ctx, "pa_integral_read: bad argument");
  if (!I->begun) return pa_fail(ctx, "pa_integral_read: pa_integral_begin has not been called");
  if (check_sum_flags(ctx, I->d_flags, "pa_integral_read")) return 1;
  const size_t nt = I->tabs.size();
  std::vector<std::vector<u64>> ht(nt);
  std::vector<std::vector<unsigned>> hf(nt);
  std::vector<U192> wfx(nt);
  for (size_t q = 0; q < nt; ++q) {
    const IntLevelTab& T = I->tabs[q];
    ht[q].resize(T.nslots * I->stride);
    hf[q].resize(T.nslots * (I->nrows - 1));
    PA_HIP(hipMemcpyAsync(ht[q].data(), T.d_tab, ht[q].size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    PA_HIP(hipMemcpyAsync(hf[q].data(), T.d_flg, hf[q].size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    int f2 = 0;
    wfx[q] = to_fixed(T.w, I->s_w, f2);
  }
  PA_HIP(hipStreamSynchronize(ctx->stream));
  const long long nslots = integral_slots(I);
  const long long l2 = I->dom.hi[I->dir2] - I->dom.lo[I->dir2] + 1;
  for (long long f = 0; f < nslots; ++f) {
    // the slot of every level above the fine slot f
    size_t ls[64];
    for (size_t q = 0; q < nt && q < 64; ++q) {
      const IntLevelTab& T = I->tabs[q];
      ls[q] = I->kind == 3 ? 0 : (I->kind == 2 ? (size_t)(f / T.R) : (size_t)((f / l2) / T.R) * T.n2 + (size_t)((f % l2) / T.R));
    }
    for (int r = 0; r < I->nrows; ++r) {
      U192 tot = {{0, 0, 0}};
      unsigned flg = 0;
      for (size_t q = 0; q < nt; ++q) {
        const u64* e = ht[q].data() + ls[q] * I->stride;
        if (r == 0) {
          u192_add(tot, u192_mul(wfx[q], e[0]));
        } else {
          const U192 v = {{e[1 + 3 * (r - 1)], e[2 + 3 * (r - 1)], e[3 + 3 * (r - 1)]}};
          u192_add(tot, v);
          flg |= hf[q][ls[q] * (I->nrows - 1) + (r - 1)];
        }
      }
      double v;
      if ((flg & PA_IF_NAN) || ((flg & PA_IF_PINF) && (flg & PA_IF_NINF))) v = std::nan("");
      else if (flg & PA_IF_PINF) v = HUGE_VAL;
      else if (flg & PA_IF_NINF) v = -HUGE_VAL;
      else v = from_fixed(tot.w, r == 0 ? I->s_w : I->s_row[r - 1]);
      out[(long long)r * nslots + f] = v;
    }
  }
  return 0;
}
