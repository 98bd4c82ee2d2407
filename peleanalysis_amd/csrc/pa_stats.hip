// pa_stats.hip -- binned statistics of a plotfile: the joint PDFs of jpdf.cpp and the conditional means of conditionalMean.cpp.
//
// A scatter with heavy contention (in a flame most cells are burnt or unburnt and fall into a handful of bins), and the first
// kernels of the library whose sums cannot keep the reference's order of additions.  Two requirements shape the design:
//
//  * REPRODUCIBLE sums.  Every sum is kept in FIXED POINT: a 192-bit two's-complement integer (three 64-bit limbs) in units of
//    2^-s, s chosen per accumulator from the declared magnitude M of its terms (pa_*_begin): M < 2^k  ->  s = 157 - k, so that
//    2^33 terms cannot overflow and a term down to 2^-105 M keeps all of its 53 bits.  Integer addition is associative: the order
//    of the adds -- run order, the tiling of the level, the order of the boxes -- drops out, bit for bit.  Limbs are added with
//    64-bit integer atomics; the carry out of a limb (old + x < old) is added to the next limb by whoever caused it.  The one
//    rounding of a sum happens on the host when it is read (pa_*_read: round to nearest even of the exact integer).
//  * Few atomics.  Neighbouring cells of a smooth field share a bin, so every thread keeps ONE private run per accumulator row:
//    the bin of its last cell, the number of cells and the fixed-point sums of the run, all in registers.  A thread marches in z
//    under a 256-cell piece of an x-y plane (lane = x: coalesced loads) and keeps its run across all tiles it visits (persistent
//    workgroups); it goes to memory only when the bin changes.  conditionalMean's whole table then lives in LDS (ds atomics) and
//    is added to the global table once per workgroup and touched entry; jpdf's table does not fit (128^2 bins x 3 sums x 24 B per pair),
//    so its runs go to a 512-slot cache of hot bins in LDS (claimed by compare-and-swap, never evicted; a run that meets a slot of
//    another bin goes to the global table) that is added to the global table once per workgroup and used slot.
//    `uncombined` selects the plain kernel -- one set of global atomics per cell -- with identical bits (tools/stats_bench.py).
// The walk itself -- tile table, decode, coverage by the finer level, LDS-table merge -- is pa_celltiles.h's, shared with pa_integral.hip.
#include "pa_celltiles.h"
#include <cfloat>
#include <cmath>
#include <cstring>

#define PA_STATS_KT 16  // cells a thread marches in z per tile
typedef CellWalkFixed<1, 2, PA_STATS_KT> StatWalk;  // planes (x, y), march in z
#define PA_STATS_NP 6   // jpdf: pairs per pass over the cells (4 variables: all of them)
#define PA_STATS_NA 8   // conditionalMean: averaged components per object
// doubles as unsigned integers of the same order (per-bin minimum / maximum with integer atomics)
__host__ __device__ __forceinline__ u64 dbl_sortable(double v) {
  u64 b;
#ifdef __HIP_DEVICE_COMPILE__
  b = (u64)__double_as_longlong(v);
#else
  memcpy(&b, &v, 8);
#endif
  return (b >> 63) ? ~b : (b | (1ull << 63));
}
static double dbl_unsortable(u64 u) {
  const u64 b = (u >> 63) ? (u & ~(1ull << 63)) : ~u;
  double v;
  memcpy(&v, &b, 8);
  return v;
}

// one lane of the active ones adds their number to *p
__device__ __forceinline__ void wave_count_add(long long* p) {
  const u64 m = __ballot(1);
  if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd((u64*)p, (u64)__popcll(m));
}

// ================================================================ min / max of several components in one launch
// jpdf.cpp:297-306 (AmrData::MinMax of every variable): every valid cell of the level, cells under a finer level included
struct MinMaxComps { int n; int comp[16]; };
__global__ __launch_bounds__(256) void k_minmax_comps(DLevelView L, DMFView M, MinMaxComps C, double* part) {
  const int b = blockIdx.y;
  const DBox B = L.boxes[b];
  const unsigned nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const unsigned n = nx * ny * nz;
  const long long nxg = nx + 2 * M.ng, nyg = ny + 2 * M.ng, nzg = nz + 2 * M.ng;
  const long long cs = pa_cstride(nxg * nyg * nzg, M.ncomp);
  const double* f = M.data + M.off[b];
  __shared__ double slo[4], shi[4];
  for (int q = 0; q < C.n; ++q) {
    const double* fc = f + (long long)C.comp[q] * cs;
    double lo = DBL_MAX, hi = -DBL_MAX;
    for (unsigned t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x) {
      const unsigned k = t / (nx * ny), r = t - k * nx * ny, j = r / nx, i = r - j * nx;
      const double v = fc[((long long)(k + M.ng) * nyg + (j + M.ng)) * nxg + (i + M.ng)];
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { slo[w] = lo; shi[w] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int z = 1; z < 4; ++z) { lo = slo[z] < lo ? slo[z] : lo; hi = shi[z] > hi ? shi[z] : hi; }
      const long long slot = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * C.n + q;
      part[2 * slot] = lo;
      part[2 * slot + 1] = hi;
    }
  }
}

extern "C" int pa_minmax_comps_level(pa_ctx* ctx, const pa_mf* s, int ncomps, const int32_t* comps, double* mn, double* mx) {
  PaBind bind_(ctx);
  if (!ctx || !s || !comps || !mn || !mx) return pa_fail(ctx, "pa_minmax_comps_level: null argument");
  if (ncomps < 1 || ncomps > 16) return pa_fail(ctx, "pa_minmax_comps_level: 1 to 16 components per call");
  MinMaxComps C;
  C.n = ncomps;
  for (int q = 0; q < ncomps; ++q) {
    if (comps[q] < 0 || comps[q] >= s->ncomp) return pa_fail(ctx, "pa_minmax_comps_level: component range");
    C.comp[q] = comps[q];
    mn[q] = DBL_MAX;
    mx[q] = -DBL_MAX;
  }
  const unsigned nb = (unsigned)s->lev->boxes.size();
  if (nb == 0) return 0;
  for (const DBox& B : s->lev->boxes)
    if ((long long)(B.hi[0] - B.lo[0] + 1) * (B.hi[1] - B.lo[1] + 1) * (B.hi[2] - B.lo[2] + 1) >= (1LL << 31))
      return pa_fail(ctx, "pa_minmax_comps_level: FAB too large");
  const unsigned gx = 32;
  const size_t np = (size_t)gx * nb * ncomps;
  if (pa_ensure_red(ctx, 2 * np)) return 1;
  hipLaunchKernelGGL(k_minmax_comps, dim3(gx, nb), dim3(256), 0, ctx->stream, s->lev->view, s->view, C, ctx->d_red);
  PA_HIP(hipGetLastError());
  std::vector<double> h(2 * np);
  PA_HIP(hipMemcpyAsync(h.data(), ctx->d_red, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t z = 0; z < np; ++z) {
    const int q = (int)(z % ncomps);
    mn[q] = std::min(mn[q], h[2 * z]);
    mx[q] = std::max(mx[q], h[2 * z + 1]);
  }
  return 0;
}

// ================================================================ the accumulator object
struct pa_hist {
  pa_ctx* ctx = nullptr;
  int kind = 0;  // 1 jpdf, 2 conditionalMean
  int nvars = 0, npairs = 0, nbins = 0, navg = 0, with_minmax = 0;
  bool begun = false;
  // jpdf: acc[((pair * 3 + which) * nbins^2 + bin) * 3 + limb], which = 0 bin, 1 binX1, 2 binX2
  // conditionalMean: acc[bin * stride + ...]: hits, sums [navg][2][3 limbs], then (with_minmax) min [navg], max [navg]
  u64* d_acc = nullptr;
  size_t acc_words = 0;
  long long* d_cnt = nullptr;  // jpdf: [npairs][5] = v1l v1g v2l v2g nan of the CURRENT add_level call
  int* d_flags = nullptr;
  CellTileTable tiles;         // of the level being added
  int s_vol = 0;               // scale exponents
  int s_x[PA_STATS_MAXV] = {};
  int s_sum[PA_STATS_NA] = {}, s_sq[PA_STATS_NA] = {};
  int stride = 0;
};

static int hist_reset(pa_ctx* ctx, pa_hist* H) {
  PA_HIP(hipMemsetAsync(H->d_acc, 0, H->acc_words * sizeof(u64), ctx->stream));
  PA_HIP(hipMemsetAsync(H->d_flags, 0, sizeof(int), ctx->stream));
  if (H->kind == 2 && H->with_minmax) {  // minima start at the largest key
    std::vector<u64> init(H->acc_words, 0);
    for (int b = 0; b < H->nbins; ++b)
      for (int a = 0; a < H->navg; ++a) init[(size_t)b * H->stride + 1 + 6 * H->navg + a] = ~0ull;
    PA_HIP(hipMemcpyAsync(H->d_acc, init.data(), init.size() * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
    PA_HIP(hipStreamSynchronize(ctx->stream));
  }
  return 0;
}

extern "C" void pa_hist_destroy(pa_hist* H) {
  if (!H) return;
  PaBind bind_(H->ctx);
  if (H->ctx && H->ctx->stream) (void)hipStreamSynchronize(H->ctx->stream);
  if (H->d_acc) (void)hipFree(H->d_acc);
  if (H->d_cnt) (void)hipFree(H->d_cnt);
  if (H->d_flags) (void)hipFree(H->d_flags);
  H->tiles.release();
  delete H;
}

static pa_hist* hist_alloc(pa_ctx* ctx, pa_hist* H, size_t words, size_t ncnt) {
  H->ctx = ctx;
  H->acc_words = words;
  if (hipMalloc((void**)&H->d_acc, words * sizeof(u64)) != hipSuccess || hipMalloc((void**)&H->d_flags, sizeof(int)) != hipSuccess ||
      (ncnt && hipMalloc((void**)&H->d_cnt, ncnt * sizeof(long long)) != hipSuccess)) {
    pa_fail(ctx, "pa_hist: out of device memory");
    pa_hist_destroy(H);
    return nullptr;
  }
  return H;
}

// ================================================================ jpdf
struct JpdfArgs {
  DLevelView L, F;
  DMFView M;
  CellTab T;
  int has_fine, ratio;
  int nbins, nload, stoich, cond, cvar, normc;
  double cnmin, cnmax, cmin, cmax;
  double h[PA_STATS_MAXV], o[PA_STATS_MAXV], vmin[PA_STATS_MAXV], vmax[PA_STATS_MAXV];
  double vol;
  U192 volfx;
  int sx[PA_STATS_MAXV];
  int pair0, np;  // this pass bins pairs pair0 .. pair0 + np - 1
  unsigned char p1[PA_STATS_NP], p2[PA_STATS_NP];
  u64* acc;
  long long* cnt;
  int* flags;
};

// jpdf.cpp:490-495: the bin of v, the casts' undefined cases defined: 0 in range, 1 clamped low, 2 clamped high, 3 NaN
__device__ __forceinline__ int jpdf_bin(double v, double vmin, double vmax, int nbins, int& idx) {
  const double q = (double)nbins * (v - vmin) / (vmax - vmin);
  if (q != q) { idx = 0; return 3; }
  if (q >= (double)nbins) { idx = nbins - 1; return 2; }
  if (q <= -1.0) { idx = 0; return 1; }
  idx = (int)q;
  return 0;
}

// The workgroup's cache of hot bins: PA_JL_SLOTS entries {pair and bin + 1 (0: free), cells, binX1 [3 limbs], binX2 [3 limbs]} in LDS,
// claimed with a compare-and-swap on the key and never evicted; a run whose slot belongs to another bin goes to the global table.
#define PA_JL_SLOTS 512
template <bool COMB>
__global__ __launch_bounds__(256) void k_jpdf(JpdfArgs A) {
  __shared__ u64 jl[COMB ? PA_JL_SLOTS * 8 : 8];
  if (COMB) {
    for (int z = threadIdx.x; z < PA_JL_SLOTS * 8; z += 256) jl[z] = 0;
    __syncthreads();
  }
  int key[PA_STATS_NP];
  u64 cnt[PA_STATS_NP];
  U192 s1[PA_STATS_NP], s2[PA_STATS_NP];
#pragma unroll
  for (int q = 0; q < PA_STATS_NP; ++q) { key[q] = -1; cnt[q] = 0; s1[q] = {{0, 0, 0}}; s2[q] = {{0, 0, 0}}; }
  int flag = 0;
  const long long nb2 = (long long)A.nbins * A.nbins;
  auto to_global = [&](int pair, long long bin, u64 n, const U192& a1, const U192& a2) {
    u64* base = A.acc + ((long long)pair * 3 * nb2 + bin) * 3;
    u192_atomic_add(base, u192_mul(A.volfx, n));
    u192_atomic_add(base + nb2 * 3, a1);
    u192_atomic_add(base + 2 * nb2 * 3, a2);
  };
  auto flush = [&](int q) {
    bool cached = false;
    if (COMB) {
      const u64 kk = (((u64)(A.pair0 + q) << 32) | (u64)(unsigned)key[q]) + 1;
      u64* e = jl + (size_t)((kk * 0x9E3779B97F4A7C15ull) >> 55) * 8;  // 9 bits: PA_JL_SLOTS = 512
      const u64 old = atomicCAS(e, 0ull, kk);
      if (old == 0 || old == kk) {
        atomicAdd(e + 1, cnt[q]);
        u192_atomic_add(e + 2, s1[q]);
        u192_atomic_add(e + 5, s2[q]);
        cached = true;
      }
    }
    if (!cached) to_global(A.pair0 + q, key[q], cnt[q], s1[q], s2[q]);
    cnt[q] = 0; s1[q] = {{0, 0, 0}}; s2[q] = {{0, 0, 0}};
  };
  for (int t = blockIdx.x; t < A.T.ntiles; t += gridDim.x) {
    const CellTile c = celltile_decode(A.T, StatWalk(), A.L.boxes, t, threadIdx.x);
    if (!c.ok) continue;
    const long long nxg = c.B.hi[0] - c.B.lo[0] + 1 + 2 * A.M.ng, nyg = c.B.hi[1] - c.B.lo[1] + 1 + 2 * A.M.ng,
                    nzg = c.B.hi[2] - c.B.lo[2] + 1 + 2 * A.M.ng;
    const long long cs = pa_cstride(nxg * nyg * nzg, A.M.ncomp);
    const double* f = A.M.data + A.M.off[c.b] + ((long long)(c.m0 - c.B.lo[2] + A.M.ng) * nyg + (c.a - c.B.lo[1] + A.M.ng)) * nxg +
                      (c.i - c.B.lo[0] + A.M.ng);
    for (int k = c.m0; k <= c.m1; ++k, f += nxg * nyg) {
      if (A.has_fine && covered_by(A.F, A.ratio, c.i, c.a, k)) continue;  // jpdf.cpp:373-387, :472
      double st = 0.0;
      if (A.stoich) {  // jpdf.cpp:410-418
        double sumH = 0.0, sumO = 0.0;
        for (int v = 0; v < A.nload; ++v) {
          const double X = f[v * cs];
          sumH += X * A.h[v];
          sumO += X * A.o[v];
        }
        st = 0.5 * sumH / sumO;
      }
      if (A.cond > 0) {  // jpdf.cpp:476-487
        double cVal = A.cvar < A.nload ? f[A.cvar * cs] : st;
        if (A.normc == 1) cVal = (cVal - A.cnmin) / (A.cnmax - A.cnmin);
        if (A.cond == 2) cVal = cVal * (1. - cVal);
        if (cVal < A.cmin || cVal > A.cmax) continue;
      }
#pragma unroll
      for (int q = 0; q < PA_STATS_NP; ++q) {
        if (q >= A.np) continue;
        const int a = A.p1[q], b = A.p2[q];
        const double v1 = a < A.nload ? f[a * cs] : st, v2 = b < A.nload ? f[b * cs] : st;
        int i1, i2;
        const int r1 = jpdf_bin(v1, A.vmin[a], A.vmax[a], A.nbins, i1), r2 = jpdf_bin(v2, A.vmin[b], A.vmax[b], A.nbins, i2);
        long long* cn = A.cnt + (A.pair0 + q) * 5;
        if (r1 == 3 || r2 == 3) { wave_count_add(cn + 4); continue; }
        if (r1 == 1) wave_count_add(cn + 0);
        if (r1 == 2) wave_count_add(cn + 1);
        if (r2 == 1) wave_count_add(cn + 2);
        if (r2 == 2) wave_count_add(cn + 3);
        const int kk = i1 * A.nbins + i2;
        if (COMB && kk != key[q] && cnt[q]) flush(q);
        key[q] = kk;
        cnt[q] += 1;
        const double t1 = A.vol * v1, t2 = A.vol * v2;  // one rounded product each (jpdf.cpp:497-498)
        u192_add(s1[q], to_fixed(t1, A.sx[a], flag));
        u192_add(s2[q], to_fixed(t2, A.sx[b], flag));
        if (!COMB) flush(q);
      }
    }
  }
  if (COMB) {  // the runs still open go to the cache; then the cache to the global table, one add per used slot
#pragma unroll
    for (int q = 0; q < PA_STATS_NP; ++q)
      if (q < A.np && cnt[q]) flush(q);
    __syncthreads();
    for (int z = threadIdx.x; z < PA_JL_SLOTS; z += 256) {
      const u64* e = jl + (size_t)z * 8;
      if (e[0] == 0) continue;
      const u64 kk = e[0] - 1;
      const U192 a1 = {{e[2], e[3], e[4]}}, a2 = {{e[5], e[6], e[7]}};
      to_global((int)(kk >> 32), (long long)(kk & 0xffffffffull), e[1], a1, a2);
    }
  }
  if (flag) atomicOr(A.flags, flag);
}

extern "C" pa_hist* pa_jpdf_create(pa_ctx* ctx, int nvars, int nbins) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  if (nvars < 2 || nvars > PA_STATS_MAXV) { pa_fail(ctx, "pa_jpdf_create: 2 to " + std::to_string(PA_STATS_MAXV) + " variables"); return nullptr; }
  if (nbins < 1 || nbins > 4096) { pa_fail(ctx, "pa_jpdf_create: nbins must be 1 .. 4096"); return nullptr; }
  pa_hist* H = new pa_hist;
  H->kind = 1;
  H->nvars = nvars;
  H->npairs = nvars * (nvars - 1) / 2;
  H->nbins = nbins;
  return hist_alloc(ctx, H, (size_t)H->npairs * 3 * nbins * nbins * 3, (size_t)H->npairs * 5);
}

extern "C" int pa_jpdf_begin(pa_ctx* ctx, pa_hist* H, double vol_max, const double* vabs) {
  PaBind bind_(ctx);
  if (!ctx || !H || !vabs || H->kind != 1) return pa_fail(ctx, "pa_jpdf_begin: bad argument");
  if (!(vol_max > 0.0) || !std::isfinite(vol_max)) return pa_fail(ctx, "pa_jpdf_begin: vol_max must be positive and finite");
  if (check_magnitudes(ctx, "pa_jpdf_begin", "variable", vabs, H->nvars)) return 1;
  H->s_vol = scale_of(vol_max);
  for (int v = 0; v < H->nvars; ++v) H->s_x[v] = scale_of(vol_max * vabs[v]);
  if (hist_reset(ctx, H)) return 1;
  H->begun = true;
  return 0;
}

extern "C" int pa_jpdf_add_level(pa_ctx* ctx, pa_hist* H, const pa_mf* vars, const pa_level* finer, int ratio, double vol,
                                 const pa_jpdf_params* P, int64_t* outside, int64_t* nan_cells) {
  PaBind bind_(ctx);
  if (!ctx || !H || !vars || !P || H->kind != 1) return pa_fail(ctx, "pa_jpdf_add_level: bad argument");
  if (!H->begun) return pa_fail(ctx, "pa_jpdf_add_level: pa_jpdf_begin has not been called");
  const int nload = P->nload, nvars = nload + (P->do_stoichiometry ? 1 : 0);
  if (nload < 1 || nvars != H->nvars) return pa_fail(ctx, "pa_jpdf_add_level: " + std::to_string(nvars) + " variables, the accumulator was created for " + std::to_string(H->nvars));
  if (vars->ncomp < nload) return pa_fail(ctx, "pa_jpdf_add_level: the multifab holds fewer components than nload");
  if (finer && ratio < 1) return pa_fail(ctx, "pa_jpdf_add_level: bad refinement ratio");
  if (!(vol > 0.0)) return pa_fail(ctx, "pa_jpdf_add_level: cell volume must be positive");
  if (P->do_conditioning < 0 || P->do_conditioning > 2) return pa_fail(ctx, "pa_jpdf_add_level: do_conditioning must be 0, 1 or 2");
  if (P->do_conditioning && (P->cvar < 0 || P->cvar >= nvars)) return pa_fail(ctx, "pa_jpdf_add_level: cVar out of range");
  for (int v = 0; v < nvars; ++v)
    if (!(P->vmax[v] != P->vmin[v])) return pa_fail(ctx, "pa_jpdf_add_level: vMax == vMin for variable " + std::to_string(v));
  if (vars->lev->nranks > 1) return pa_fail(ctx, "pa_jpdf_add_level: sharded levels are not supported");
  JpdfArgs A;
  A.L = vars->lev->view;
  A.M = vars->view;
  fine_cover(vars->lev, finer, ratio, A.F, A.has_fine, A.ratio);
  if (outside) memset(outside, 0, sizeof(int64_t) * 4 * H->npairs);
  if (nan_cells) memset(nan_cells, 0, sizeof(int64_t) * H->npairs);
  if (vars->lev->boxes.empty()) return 0;
  if (H->tiles.build(ctx, vars->lev, StatWalk::aax, StatWalk::march, StatWalk::kt, "pa_stats", A.T)) return 1;
  A.nbins = H->nbins; A.nload = nload; A.stoich = P->do_stoichiometry ? 1 : 0;
  A.cond = P->do_conditioning; A.cvar = P->cvar; A.normc = P->norm_cval;
  A.cnmin = P->cnorm_min; A.cnmax = P->cnorm_max; A.cmin = P->cmin; A.cmax = P->cmax;
  for (int v = 0; v < PA_STATS_MAXV; ++v) { A.h[v] = P->hlist[v]; A.o[v] = P->olist[v]; A.vmin[v] = P->vmin[v]; A.vmax[v] = P->vmax[v]; A.sx[v] = H->s_x[v]; }
  A.vol = vol;
  int fl = 0;
  A.volfx = to_fixed(vol, H->s_vol, fl);
  if (fl) return pa_fail(ctx, "pa_jpdf_add_level: the cell volume exceeds the vol_max given to pa_jpdf_begin");
  A.acc = H->d_acc; A.cnt = H->d_cnt; A.flags = H->d_flags;
  PA_HIP(hipMemsetAsync(H->d_cnt, 0, (size_t)H->npairs * 5 * sizeof(long long), ctx->stream));
  std::vector<std::pair<int, int>> pairs;
  for (int a = 0; a < nvars; ++a)
    for (int b = a + 1; b < nvars; ++b) pairs.push_back({a, b});
  const unsigned grid = (unsigned)std::min<long long>(A.T.ntiles, 2048);
  for (int p0 = 0; p0 < H->npairs; p0 += PA_STATS_NP) {
    A.pair0 = p0;
    A.np = std::min(PA_STATS_NP, H->npairs - p0);
    for (int q = 0; q < A.np; ++q) { A.p1[q] = (unsigned char)pairs[p0 + q].first; A.p2[q] = (unsigned char)pairs[p0 + q].second; }
    if (P->uncombined) hipLaunchKernelGGL(k_jpdf<false>, dim3(grid), dim3(256), 0, ctx->stream, A);
    else hipLaunchKernelGGL(k_jpdf<true>, dim3(grid), dim3(256), 0, ctx->stream, A);
    PA_HIP(hipGetLastError());
  }
  if (outside || nan_cells) {
    std::vector<long long> h((size_t)H->npairs * 5);
    PA_HIP(hipMemcpyAsync(h.data(), H->d_cnt, h.size() * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    PA_HIP(hipStreamSynchronize(ctx->stream));
    for (int p = 0; p < H->npairs; ++p) {
      if (outside) for (int z = 0; z < 4; ++z) outside[4 * p + z] = h[5 * p + z];
      if (nan_cells) nan_cells[p] = h[5 * p + 4];
    }
  }
  return 0;
}

extern "C" int pa_jpdf_read(pa_ctx* ctx, const pa_hist* H, double* bin, double* binx1, double* binx2) {
  PaBind bind_(ctx);
  if (!ctx || !H || !bin || !binx1 || !binx2 || H->kind != 1) return pa_fail(ctx, "pa_jpdf_read: bad argument");
  if (!H->begun) return pa_fail(ctx, "pa_jpdf_read: pa_jpdf_begin has not been called");
  if (check_sum_flags(ctx, H->d_flags, "pa_jpdf_read")) return 1;
  std::vector<u64> h(H->acc_words);
  PA_HIP(hipMemcpyAsync(h.data(), H->d_acc, h.size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipStreamSynchronize(ctx->stream));
  const size_t nb2 = (size_t)H->nbins * H->nbins;
  int p = 0;
  for (int a = 0; a < H->nvars; ++a)
    for (int b = a + 1; b < H->nvars; ++b, ++p)
      for (size_t i = 0; i < nb2; ++i) {
        const u64* w = h.data() + ((size_t)p * 3 * nb2 + i) * 3;
        bin[p * nb2 + i] = from_fixed(w, H->s_vol);
        binx1[p * nb2 + i] = from_fixed(w + nb2 * 3, H->s_x[a]);
        binx2[p * nb2 + i] = from_fixed(w + 2 * nb2 * 3, H->s_x[b]);
      }
  return 0;
}

// ================================================================ conditionalMean
struct CondArgs {
  DLevelView L, F;
  DMFView M;
  CellTab T;
  int has_fine, ratio;
  DBox dom;
  int nbins, navg, with_minmax, stride;
  double bmin, bmax;
  long long weight;
  int ssum[PA_STATS_NA], ssq[PA_STATS_NA];
  u64* acc;
  int* flags;
};

// one run of a thread (or one cell) into a table of the accumulator's layout, in LDS or in HBM
template <int NA>
__device__ __forceinline__ void cond_flush(u64* tab, const CondArgs& A, int key, u64& cnt, U192 (&sm)[NA], U192 (&sq)[NA], u64 (&mn)[NA], u64 (&mx)[NA]) {
  u64* e = tab + (long long)key * A.stride;
  atomicAdd(e, cnt * (u64)A.weight);
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    if (a >= A.navg) continue;
    u192_atomic_add(e + 1 + 6 * a, sm[a]);
    u192_atomic_add(e + 1 + 6 * a + 3, sq[a]);
    if (A.with_minmax) {
      atomicMin(e + 1 + 6 * A.navg + a, mn[a]);
      atomicMax(e + 1 + 7 * A.navg + a, mx[a]);
    }
    sm[a] = {{0, 0, 0}}; sq[a] = {{0, 0, 0}}; mn[a] = ~0ull; mx[a] = 0ull;
  }
  cnt = 0;
}

// MODE 0: one set of global atomics per cell; 1: private runs -> global table; 2: private runs -> LDS table -> global table
template <int NA, int MODE>
__global__ __launch_bounds__(256) void k_condmean(CondArgs A) {
  extern __shared__ u64 lds[];
  u64* tab = A.acc;
  if (MODE == 2) {
    const int nw = A.nbins * A.stride;
    for (int z = threadIdx.x; z < nw; z += 256) {
      const int r = z % A.stride;
      lds[z] = (A.with_minmax && r >= 1 + 6 * A.navg && r < 1 + 7 * A.navg) ? ~0ull : 0ull;
    }
    __syncthreads();
    tab = lds;
  }
  int key = -1, flag = 0;
  u64 cnt = 0;
  U192 sm[NA], sq[NA];
  u64 mn[NA], mx[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) { sm[a] = {{0, 0, 0}}; sq[a] = {{0, 0, 0}}; mn[a] = ~0ull; mx[a] = 0ull; }
  for (int t = blockIdx.x; t < A.T.ntiles; t += gridDim.x) {
    const CellTile c = celltile_decode(A.T, StatWalk(), A.L.boxes, t, threadIdx.x);
    if (!c.ok) continue;
    if (c.i < A.dom.lo[0] || c.i > A.dom.hi[0] || c.a < A.dom.lo[1] || c.a > A.dom.hi[1]) continue;  // conditionalMean.cpp:215
    const long long nxg = c.B.hi[0] - c.B.lo[0] + 1 + 2 * A.M.ng, nyg = c.B.hi[1] - c.B.lo[1] + 1 + 2 * A.M.ng,
                    nzg = c.B.hi[2] - c.B.lo[2] + 1 + 2 * A.M.ng;
    const long long cs = pa_cstride(nxg * nyg * nzg, A.M.ncomp);
    const double* f = A.M.data + A.M.off[c.b] + ((long long)(c.m0 - c.B.lo[2] + A.M.ng) * nyg + (c.a - c.B.lo[1] + A.M.ng)) * nxg +
                      (c.i - c.B.lo[0] + A.M.ng);
    for (int k = c.m0; k <= c.m1; ++k, f += nxg * nyg) {
      if (k < A.dom.lo[2] || k > A.dom.hi[2]) continue;
      if (A.has_fine && covered_by(A.F, A.ratio, c.i, c.a, k)) continue;  // conditionalMean.cpp:246-258, :267
      const double binVal = f[0];
      if (!(binVal >= A.bmin && binVal < A.bmax)) continue;  // :270
      const int myBin = (int)((double)A.nbins * (binVal - A.bmin) / (A.bmax - A.bmin));  // :272
      if (myBin < 0 || myBin >= A.nbins) { flag |= PA_ST_BADBIN; continue; }  // :273-274 "Bad bin"
      if (MODE != 0 && myBin != key && cnt) cond_flush<NA>(tab, A, key, cnt, sm, sq, mn, mx);
      key = myBin;
      cnt += 1;
#pragma unroll
      for (int a = 0; a < NA; ++a) {
        if (a >= A.navg) continue;
        const double val = f[(1 + a) * cs];
        const double wv = (double)A.weight * val;  // :280-281: myWeight * val, then (myWeight * val) * val
        const double wvv = wv * val;
        u192_add(sm[a], to_fixed(wv, A.ssum[a], flag));
        u192_add(sq[a], to_fixed(wvv, A.ssq[a], flag));
        if (A.with_minmax) {
          const u64 u = dbl_sortable(val);
          mn[a] = u < mn[a] ? u : mn[a];
          mx[a] = u > mx[a] ? u : mx[a];
        }
      }
      if (MODE == 0) cond_flush<NA>(tab, A, key, cnt, sm, sq, mn, mx);
    }
  }
  if (MODE != 0 && cnt) cond_flush<NA>(tab, A, key, cnt, sm, sq, mn, mx);
  if (MODE == 2)  // the workgroup's table -> the global one: one add per touched entry; per bin: hits, navg x (sum, sumsq), then min / max
    celltab_merge(lds, A.acc, A.nbins, 1 + 2 * A.navg, A.stride, [&](const u64* e, u64* g) {
      if (A.with_minmax)
        for (int a = 0; a < A.navg; ++a) {
          atomicMin(g + 1 + 6 * A.navg + a, e[1 + 6 * A.navg + a]);
          atomicMax(g + 1 + 7 * A.navg + a, e[1 + 7 * A.navg + a]);
        }
    });
  if (flag) atomicOr(A.flags, flag);
}

extern "C" pa_hist* pa_condmean_create(pa_ctx* ctx, int navg, int nbins, int with_minmax) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  if (navg < 1 || navg > PA_STATS_NA) { pa_fail(ctx, "pa_condmean_create: 1 to " + std::to_string(PA_STATS_NA) + " averaged components per accumulator"); return nullptr; }
  if (nbins < 1 || nbins > (1 << 20)) { pa_fail(ctx, "pa_condmean_create: nbins must be 1 .. 2^20"); return nullptr; }
  pa_hist* H = new pa_hist;
  H->kind = 2;
  H->navg = navg;
  H->nbins = nbins;
  H->with_minmax = with_minmax ? 1 : 0;
  H->stride = 1 + 6 * navg + (with_minmax ? 2 * navg : 0);
  return hist_alloc(ctx, H, (size_t)nbins * H->stride, 0);
}

extern "C" int pa_condmean_begin(pa_ctx* ctx, pa_hist* H, int64_t weight_max, const double* vabs) {
  PaBind bind_(ctx);
  if (!ctx || !H || !vabs || H->kind != 2) return pa_fail(ctx, "pa_condmean_begin: bad argument");
  if (weight_max < 1) return pa_fail(ctx, "pa_condmean_begin: weight_max must be at least 1");
  if (check_magnitudes(ctx, "pa_condmean_begin", "component", vabs, H->navg)) return 1;
  for (int a = 0; a < H->navg; ++a) {
    H->s_sum[a] = scale_of((double)weight_max * vabs[a]);
    H->s_sq[a] = scale_of((double)weight_max * vabs[a] * vabs[a]);
  }
  if (hist_reset(ctx, H)) return 1;
  H->begun = true;
  return 0;
}

template <int NA>
static void condmean_launch(pa_ctx* ctx, const CondArgs& A, int mode, unsigned grid, size_t lds_bytes) {
  if (mode == 0) hipLaunchKernelGGL((k_condmean<NA, 0>), dim3(grid), dim3(256), 0, ctx->stream, A);
  else if (mode == 1) hipLaunchKernelGGL((k_condmean<NA, 1>), dim3(grid), dim3(256), 0, ctx->stream, A);
  else hipLaunchKernelGGL((k_condmean<NA, 2>), dim3(grid), dim3(256), lds_bytes, ctx->stream, A);
}

extern "C" int pa_condmean_add_level(pa_ctx* ctx, pa_hist* H, const pa_mf* comps, const pa_level* finer, int ratio, const pa_box* domain,
                                     int64_t weight, double bin_min, double bin_max, int uncombined) {
  PaBind bind_(ctx);
  if (!ctx || !H || !comps || !domain || H->kind != 2) return pa_fail(ctx, "pa_condmean_add_level: bad argument");
  if (!H->begun) return pa_fail(ctx, "pa_condmean_add_level: pa_condmean_begin has not been called");
  if (comps->ncomp < 1 + H->navg) return pa_fail(ctx, "pa_condmean_add_level: the multifab must hold the bin component and " + std::to_string(H->navg) + " averaged ones");
  if (finer && ratio < 1) return pa_fail(ctx, "pa_condmean_add_level: bad refinement ratio");
  if (weight < 1) return pa_fail(ctx, "pa_condmean_add_level: weight must be at least 1");
  if (!(bin_max > bin_min)) return pa_fail(ctx, "pa_condmean_add_level: binMax must be greater than binMin");
  if (comps->lev->nranks > 1) return pa_fail(ctx, "pa_condmean_add_level: sharded levels are not supported");
  if (comps->lev->boxes.empty()) return 0;
  CondArgs A;
  A.L = comps->lev->view;
  A.M = comps->view;
  fine_cover(comps->lev, finer, ratio, A.F, A.has_fine, A.ratio);
  for (int d = 0; d < 3; ++d) { A.dom.lo[d] = domain->lo[d]; A.dom.hi[d] = domain->hi[d]; }
  if (H->tiles.build(ctx, comps->lev, StatWalk::aax, StatWalk::march, StatWalk::kt, "pa_stats", A.T)) return 1;
  A.nbins = H->nbins; A.navg = H->navg; A.with_minmax = H->with_minmax; A.stride = H->stride;
  A.bmin = bin_min; A.bmax = bin_max; A.weight = weight;
  for (int a = 0; a < PA_STATS_NA; ++a) { A.ssum[a] = H->s_sum[a]; A.ssq[a] = H->s_sq[a]; }
  A.acc = H->d_acc; A.flags = H->d_flags;
  const size_t lds_bytes = (size_t)H->nbins * H->stride * sizeof(u64);
  const int mode = uncombined ? 0 : (lds_bytes <= 48 * 1024 ? 2 : 1);
  const unsigned grid = (unsigned)std::min<long long>(A.T.ntiles, 1024);
  if (H->navg <= 2) condmean_launch<2>(ctx, A, mode, grid, lds_bytes);
  else if (H->navg <= 4) condmean_launch<4>(ctx, A, mode, grid, lds_bytes);
  else condmean_launch<PA_STATS_NA>(ctx, A, mode, grid, lds_bytes);
  PA_HIP(hipGetLastError());
  return 0;
}

extern "C" int pa_condmean_read(pa_ctx* ctx, const pa_hist* H, int64_t* hits, double* sum, double* sumsq, double* mn, double* mx) {
  PaBind bind_(ctx);
  if (!ctx || !H || !hits || !sum || !sumsq || H->kind != 2) return pa_fail(ctx, "pa_condmean_read: bad argument");
  if (!H->begun) return pa_fail(ctx, "pa_condmean_read: pa_condmean_begin has not been called");
  if (H->with_minmax && (!mn || !mx)) return pa_fail(ctx, "pa_condmean_read: the accumulator keeps minima and maxima: mn and mx are needed");
  if (check_sum_flags(ctx, H->d_flags, "pa_condmean_read")) return 1;
  std::vector<u64> h(H->acc_words);
  PA_HIP(hipMemcpyAsync(h.data(), H->d_acc, h.size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipStreamSynchronize(ctx->stream));
  for (int b = 0; b < H->nbins; ++b) {
    const u64* e = h.data() + (size_t)b * H->stride;
    hits[b] = (int64_t)e[0];
    for (int a = 0; a < H->navg; ++a) {
      sum[b * H->navg + a] = from_fixed(e + 1 + 6 * a, H->s_sum[a]);
      sumsq[b * H->navg + a] = from_fixed(e + 1 + 6 * a + 3, H->s_sq[a]);
      if (H->with_minmax) {  // an empty bin keeps the reference's initial 0 (conditionalMean.cpp:105-106)
        mn[b * H->navg + a] = e[0] ? dbl_unsortable(e[1 + 6 * H->navg + a]) : 0.0;
        mx[b * H->navg + a] = e[0] ? dbl_unsortable(e[1 + 7 * H->navg + a]) : 0.0;
      }
    }
  }
  return 0;
}
