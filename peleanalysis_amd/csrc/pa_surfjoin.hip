// pa_surfjoin.hip -- joining surfaces and editing their node fields on the handle of pa_surf.h (mergeMEF.cpp, scaleMEF.cpp, multMEF.cpp,
// combineMEF.cpp).
//   merge   merge_iso (mergeMEF.cpp:138-244): node i of S becomes the SMALLEST j < nN_M with ((dx0*dx0) + dx1*dx1) + dx2*dx2 <= eps*eps
//           (dx = S minus M, eps*eps formed once on the host), or the next new id in order of i.  Nodes of S are never compared with each
//           other, so every node is decided on its own:
//           brute   one wavefront per node of S walks j upward in chunks of 256 and stops at the first chunk with a hit, taking the
//                   minimum j of that chunk: the reference's loop, and the fallback
//           grid    1. bounds   the smallest / largest finite coordinate of M and of S (integer minima of order-preserving bit patterns)
//                   2. keys     node j of M -> cell c(x) = floor((x - lo) / h) per axis -> 64-bit hash; non-finite nodes get the key ~0,
//                               which no cell has (a cell that hashes to ~0 is moved to ~0 - 1), and sort behind the table
//                   3. sort     STABLE radix sort of (hash, j): j ascends inside every run; the coordinates follow in sorted order
//                   4. probe    node i of S looks up every cell that the box [s - r, s + r] touches, finds each hash's run by binary
//                               search, tests the candidates with the exact predicate above, stops a run at its first hit (or at the
//                               first j that is not below the best so far) and keeps the minimum j over the runs
//           then    flags, an exclusive scan of the not-found flags, and order-preserving copies into a NEW allocation (M stays
//                   component-major, so appending re-lays out its columns).  No atomics place anything.
//   WHY THE GRID FINDS EVERY j THE LOOP FINDS.  Let e2 = fl(eps * eps) and let the predicate hold for (i, j).  Sums of non-negative terms
//   do not round below a term, so fl(dx*dx) <= e2 for each axis.  If |dx| >= 2^-499 the square is a normal number, hence
//   dx*dx <= e2 / (1 - 2^-53) and |dx| <= sqrt(e2) * (1 + 2^-52); otherwise |dx| < 2^-499.  dx is the ROUNDED difference; the true one is
//   within a factor 1 + 2^-52 of it (exact where it is subnormal).  With r = max(sqrt(e2), 2^-499) * (1 + 2^-40) -- the host's sqrt is
//   correctly rounded -- the true |s - m| <= r holds on every axis.  m is a double, and rounding is monotone: s - r <= m <= s + r gives
//   fl(s - r) <= m <= fl(s + r).  c(x) is a composition of monotone steps (a rounded subtraction of one lo, a rounded division by one
//   h > 0, floor), so c(fl(s - r)) <= c(m) <= c(fl(s + r)): the cell of m is among those probed, whatever h is, and whatever the hash
//   does -- collisions and the choice of h only add candidates, which the exact predicate rejects.  The answer is the minimum over all
//   candidates of a set that contains every j the loop could find, so it is the loop's j.
//   HOW MANY CELLS.  h = max(2 r (1 + 2^-30), extent of M * 2^-40), so the box spans less than 2 cells in exact arithmetic plus the
//   rounding of s -+ r (at most one more cell: where ulp(s) > 2 r both ends round to s itself) plus the rounding of the two quotients
//   (below 1/2 each while every cell coordinate is below 2^51): at most 4 cells per axis, usually 2.  The probe loops run to 4; a box
//   that still spans more raises a flag and the call takes brute force.  The host refuses the grid (auto: brute force) where the
//   largest cell coordinate of M or S reaches 2^51 or is not finite, where M has no finite node, and where fewer than 2 cells span M
//   (eps at or above the extent: the table would be one run, i.e. brute force with a sort in front).
//   small   scale (scaleMEF.cpp:101-108) col = col * v per entry, in list order; product (multMEF.cpp:139-148) ((1.0 * d[c0]) * d[c1]) ...;
//           select (combineMEF.cpp:165-181) copies of chosen columns of two handles.
// Every floating-point value is computed by ONE thread in a written order (the file is built with -ffp-contract=off); atomics combine
// only integer counts and minima / maxima.  The same input gives the same bytes: those of tests/surfjoin_ref.py.
#include <cfloat>
#include <cmath>
#include <cstring>
#include "pa_surf.h"

namespace {
constexpr int SJ_BLOCKS = 2048;  // the bounds kernel strides with a grid of at most this many blocks
struct SjGrid { double lo[3]; double h; double r; };

__device__ __forceinline__ bool sj_finite(double x, double y, double z) { return fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX && fabs(z) <= DBL_MAX; }
__device__ __forceinline__ long long sj_cell(double x, double lo, double h) { return (long long)floor((x - lo) / h); }
// the mixing of pa_isomerge.hip; ~0 is kept for "not in the table"
__device__ __forceinline__ u64 sj_hash(long long x, long long y, long long z) {
  u64 h = (u64)x * 0x9E3779B97F4A7C15ull;
  h ^= (u64)y * 0xC2B2AE3D27D4EB4Full + (h << 6) + (h >> 2);
  h ^= (u64)z * 0x165667B19E3779F9ull + (h << 6) + (h >> 2);
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  return h == ~0ull ? ~0ull - 1 : h;
}
// order-preserving bit pattern of a finite double
__host__ __device__ __forceinline__ u64 sj_okey(double x) {
  u64 b;
  memcpy(&b, &x, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
inline double sj_unkey(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double x;
  memcpy(&x, &b, 8);
  return x;
}
__device__ __forceinline__ u64 sj_wave_min(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o); v = w < v ? w : v; } return v; }
__device__ __forceinline__ u64 sj_wave_max(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o); v = w > v ? w : v; } return v; }

// out[0..2] smallest, out[3..5] largest key per axis over the nodes whose three coordinates are finite, out[6] their number
__global__ __launch_bounds__(256) void k_sj_bounds(int n, const double* V, u64* out) {
  u64 lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0, 0, 0}, cnt = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double p[3] = {V[i], V[(long long)n + i], V[2LL * n + i]};
    if (!sj_finite(p[0], p[1], p[2])) continue;
    cnt += 1;
    for (int d = 0; d < 3; ++d) { const u64 k = sj_okey(p[d]); lo[d] = k < lo[d] ? k : lo[d]; hi[d] = k > hi[d] ? k : hi[d]; }
  }
  for (int d = 0; d < 3; ++d) { lo[d] = sj_wave_min(lo[d]); hi[d] = sj_wave_max(hi[d]); }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if ((threadIdx.x & 63) == 0 && cnt) {
    for (int d = 0; d < 3; ++d) { atomicMin(&out[d], lo[d]); atomicMax(&out[3 + d], hi[d]); }
    atomicAdd(&out[6], cnt);
  }
}
__global__ __launch_bounds__(256) void k_sj_keys(int nM, const double* MV, SjGrid G, u64* hash, int* idx) {
  const int j = sc_item();
  if (j >= nM) return;
  const double x = MV[j], y = MV[(long long)nM + j], z = MV[2LL * nM + j];
  hash[j] = sj_finite(x, y, z) ? sj_hash(sj_cell(x, G.lo[0], G.h), sj_cell(y, G.lo[1], G.h), sj_cell(z, G.lo[2], G.h)) : ~0ull;
  idx[j] = j;
}
__global__ __launch_bounds__(256) void k_sj_sorted(int nM, const int* sidx, const double* MV, double* P) {  // P[d * nM + a] = coordinate d of the a-th entry
  const int a = sc_item();
  if (a >= nM) return;
  const long long j = sidx[a];
  P[a] = MV[j]; P[(long long)nM + a] = MV[(long long)nM + j]; P[2LL * nM + a] = MV[2LL * nM + j];
}
// nT: the entries of the table (the finite nodes of M lead the sorted arrays)
__global__ __launch_bounds__(256) void k_sj_probe(int nS, const double* SV, int nM, int nT, const u64* shash, const int* sidx, const double* P, SjGrid G, double e2,
                                                  int* dup, int* wide) {
  const int i = sc_item();
  if (i >= nS) return;
  const double s[3] = {SV[i], SV[(long long)nS + i], SV[2LL * nS + i]};
  int best = 0x7fffffff;
  if (sj_finite(s[0], s[1], s[2])) {
    long long clo[3], chi[3];
    for (int d = 0; d < 3; ++d) {
      clo[d] = sj_cell(s[d] - G.r, G.lo[d], G.h);
      chi[d] = sj_cell(s[d] + G.r, G.lo[d], G.h);
    }
    if (chi[0] - clo[0] > 3 || chi[1] - clo[1] > 3 || chi[2] - clo[2] > 3) *wide = 1;  // never, by the header's bound: the host then takes brute force
    for (int az = 0; az < 4; ++az) {
      if (clo[2] + az > chi[2]) break;
      for (int ay = 0; ay < 4; ++ay) {
        if (clo[1] + ay > chi[1]) break;
        for (int ax = 0; ax < 4; ++ax) {
          if (clo[0] + ax > chi[0]) break;
          const u64 h = sj_hash(clo[0] + ax, clo[1] + ay, clo[2] + az);
          int a = 0, b = nT;  // lower bound of h
          while (a < b) {
            const int m = (int)(((long long)a + b) >> 1);
            if (shash[m] < h) a = m + 1; else b = m;
          }
          for (; a < nT; ++a) {
            if (shash[a] != h) break;
            const int j = sidx[a];
            if (j >= best) break;  // equal hashes keep the order of j (stable sort): nothing smaller follows
            const double dx0 = s[0] - P[a], dx1 = s[1] - P[(long long)nM + a], dx2 = s[2] - P[2LL * nM + a];
            if (((dx0 * dx0) + dx1 * dx1) + dx2 * dx2 <= e2) { best = j; break; }
          }
        }
      }
    }
  }
  dup[i] = best == 0x7fffffff ? -1 : best;
}
// one wavefront per node of S; chunk = 4 values of j per lane
__global__ __launch_bounds__(256) void k_sj_brute(int nS, const double* SV, int nM, const double* MV, double e2, int* dup) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nS) return;
  const int lane = threadIdx.x & 63;
  const double s0 = SV[w], s1 = SV[(long long)nS + w], s2 = SV[2LL * nS + w];
  int best = -1;
  for (long long j0 = 0; j0 < nM; j0 += 256) {
    int hit = 0x7fffffff;
    for (int q = 3; q >= 0; --q) {
      const long long j = j0 + 64 * q + lane;
      if (j < nM) {
        const double dx0 = s0 - MV[j], dx1 = s1 - MV[(long long)nM + j], dx2 = s2 - MV[2LL * nM + j];
        if (((dx0 * dx0) + dx1 * dx1) + dx2 * dx2 <= e2) hit = (int)j;
      }
    }
    for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(hit, o); hit = v < hit ? v : hit; }
    if (hit != 0x7fffffff) { best = hit; break; }  // the same in every lane
  }
  if (lane == 0) dup[w] = best;
}
__global__ __launch_bounds__(256) void k_sj_nodup(int nS, int* dup) {
  const int i = sc_item();
  if (i < nS) dup[i] = -1;
}
__global__ __launch_bounds__(256) void k_sj_flags(int nS, const int* dup, int* isnew) {
  const int i = sc_item();
  if (i < nS) isnew[i] = dup[i] < 0 ? 1 : 0;
}
// W has nW nodes per column: M's nM first
__global__ __launch_bounds__(256) void k_sj_copy_cols(long long n, long long nM, long long nW, const double* MV, double* W) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const long long c = t / nM, i = t - c * nM;
  W[c * nW + i] = MV[t];
}
__global__ __launch_bounds__(256) void k_sj_new_cols(long long n, long long nS, long long nM, long long nW, const double* SV, const int* isnew, const int* newid, double* W) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const long long c = t / nS, i = t - c * nS;
  if (isnew[i]) W[c * nW + nM + newid[i]] = SV[t];
}
__global__ __launch_bounds__(256) void k_sj_copy_int(long long n, const int* in, int* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < n) out[t] = in[t];
}
__global__ __launch_bounds__(256) void k_sj_new_elts(long long n, const int* SF, const int* dup, const int* newid, int nM, int* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int i = SF[t];
  out[t] = dup[i] >= 0 ? dup[i] : nM + newid[i];
}
__global__ __launch_bounds__(256) void k_sj_scale(long long n, double* col, double v) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < n) col[t] = col[t] * v;
}
struct SjComps { int n; int c[32]; };
__global__ __launch_bounds__(256) void k_sj_product(long long n, const double* V, SjComps C, double* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  double p = 1.0;
  for (int k = 0; k < C.n; ++k) p = p * V[(long long)C.c[k] * n + t];
  out[t] = p;
}
__global__ __launch_bounds__(256) void k_sj_copy_col(long long n, const double* in, double* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < n) out[t] = in[t];
}

#define SJ_TRY(call)           \
  do {                         \
    const int rc_ = (call);    \
    if (rc_ != 0) return rc_;  \
  } while (0)
void sj_rec(pa_surf* S, int op) {
  for (int64_t& r : S->rec) r = 0;
  S->rec[0] = op;
}
// a handle with room for nN nodes of nc components and nE elements; its contents are the caller's to write
pa_surf* sj_new(pa_ctx* ctx, long long nN, long long nE, int nc) {
  pa_surf* S = new pa_surf;
  S->ctx = ctx; S->nN = nN; S->nE = nE; S->nc = nc;
  if (hipMalloc((void**)&S->V, std::max<size_t>((size_t)nN * (size_t)nc, 1) * sizeof(double)) != hipSuccess ||
      hipMalloc((void**)&S->F, std::max<size_t>(3 * (size_t)nE, 1) * sizeof(int)) != hipSuccess) {
    pa_surf_destroy(S);
    ctx->err = "pa_surf: out of device memory";
    return nullptr;
  }
  return S;
}
// the grid of a merge, or why there is none
bool sj_plan(const u64 bm[7], const u64 bs[7], double e2, SjGrid& G, std::string& why) {
  if (bm[6] == 0) { why = "M has no finite node"; return false; }
  const double root = std::sqrt(e2);
  const double r = std::max(root, std::ldexp(1.0, -499)) * (1.0 + std::ldexp(1.0, -40));
  double ext = 0.0;
  for (int d = 0; d < 3; ++d) ext = std::max(ext, sj_unkey(bm[3 + d]) - sj_unkey(bm[d]));
  const double h = std::max(2.0 * r * (1.0 + std::ldexp(1.0, -30)), ext * std::ldexp(1.0, -40));
  if (!(h > 0.0) || !(h <= DBL_MAX) || !(r <= DBL_MAX)) { why = "the cell width is not finite"; return false; }
  double cmax = 0.0, cm = 0.0;
  for (int d = 0; d < 3; ++d) {
    const double lo = sj_unkey(bm[d]);
    double a = lo, b = sj_unkey(bm[3 + d]);
    cm = std::max(cm, std::floor((b - lo) / h));
    if (bs[6] != 0) { a = std::min(a, sj_unkey(bs[d])); b = std::max(b, sj_unkey(bs[3 + d])); }
    const double ta = std::floor(((a - r) - lo) / h), tb = std::floor(((b + r) - lo) / h);
    if (!(std::fabs(ta) <= DBL_MAX) || !(std::fabs(tb) <= DBL_MAX)) { why = "a cell coordinate is not finite"; return false; }
    cmax = std::max(cmax, std::max(std::fabs(ta), std::fabs(tb)));
    G.lo[d] = lo;
  }
  if (cmax >= std::ldexp(1.0, 51)) { why = "the largest cell coordinate reaches 2^51"; return false; }
  if (cm < 1.0) { why = "fewer than 2 cells span M (eps is at or above its extent)"; return false; }
  G.h = h; G.r = r;
  return true;
}
}  // namespace

extern "C" int pa_surfjoin_merge(pa_ctx* ctx, pa_surf* S_M, const pa_surf* S_S, double eps, int rem_dup_nodes, int method, int* appended) {
  PaBind bind_(ctx);
  pa_surf* S = S_M;  // SF_HIP reports through the handle named S
  const pa_surf* T = S_S;
  if (!sf_own(ctx, S) || !sf_own(ctx, T)) return pa_fail(ctx, "pa_surfjoin_merge: null argument, or an object belongs to another context");
  if (S == T) return pa_fail(ctx, "pa_surfjoin_merge: a surface cannot be merged into itself");
  if (S->nc != T->nc) return pa_fail(ctx, "pa_surfjoin_merge: the surfaces have " + std::to_string(S->nc) + " and " + std::to_string(T->nc) + " node components");
  if (method < 0 || method > 2) return pa_fail(ctx, "pa_surfjoin_merge: method is 0 (auto), 1 (grid) or 2 (brute force)");
  const double e2 = eps * eps;
  if (!(std::fabs(e2) <= DBL_MAX)) return pa_fail(ctx, "pa_surfjoin_merge: eps * eps is not finite");
  if (rem_dup_nodes && S->nc < 3) return pa_fail(ctx, "pa_surfjoin_merge: remDupNodes needs the node coordinates x, y, z as the first three components, the surfaces have " + std::to_string(S->nc));
  hipStream_t st = ctx->stream;
  int launches = 0;
  const int nM = (int)S->nN, nS = (int)T->nN, nc = S->nc;
  const long long nEM = S->nE, nES = T->nE;
  // A call that fails leaves the handle as it was, its slice and its launch record included: the scratch used below holds nothing that
  // pa_surf_slice_read reads, and `done` runs only where the call succeeds.
  int64_t rec[8] = {4, nS, 0, 0, 0, 0, 0, 0};
  auto done = [&](int app) {
    S->sliced = false; S->nsegs = 0; S->nverts = 0;  // a merge drops the slice M held
    rec[7] = launches;
    for (int k = 0; k < 8; ++k) S->rec[k] = rec[k];
    if (appended) *appended = app;
    return 0;
  };
  if (nS == 0) return done(0);  // cnt == nNodesM (:210): nothing is new
  int *dup, *isnew, *newid;
  SJ_TRY(sf_need(S, pa_surf::B_FLAG, (size_t)nS, dup));
  SJ_TRY(sf_need(S, pa_surf::B_POS, (size_t)nS, isnew));
  SJ_TRY(sf_need(S, pa_surf::B_HEAD, (size_t)nS, newid));
  int path = 0;
  long long ntab = 0;
  if (!rem_dup_nodes) {
    SF_LAUNCH(k_sj_nodup, nS, nS, dup);
  } else {
    SjGrid G = {{0, 0, 0}, 0, 0};
    std::string why;
    bool grid = false;
    u64* aux = nullptr;  // [0..6] bounds of M, [8..14] of S, [16] the probe's flag
    SJ_TRY(sf_need(S, pa_surf::B_AUX, 24, aux));
    if (method != 2) {
      u64 init[24], hb[24];
      for (int k = 0; k < 24; ++k) init[k] = 0;
      for (int k = 0; k < 3; ++k) init[k] = init[8 + k] = ~0ull;
      SF_HIP(hipMemcpyAsync(aux, init, sizeof init, hipMemcpyHostToDevice, st));
      // threads of the striding grid: 16 nodes each, or more -- one node per thread put 13 atomics per 64 nodes onto the same 13 words
      const long long spanM = std::min<long long>((nM + 15LL) / 16, (long long)SJ_BLOCKS * 256), spanS = std::min<long long>((nS + 15LL) / 16, (long long)SJ_BLOCKS * 256);
      SF_LAUNCH(k_sj_bounds, spanM, nM, S->V, aux);
      SF_LAUNCH(k_sj_bounds, spanS, nS, T->V, aux + 8);
      SF_HIP(hipMemcpyAsync(hb, aux, sizeof hb, hipMemcpyDeviceToHost, st));
      SF_HIP(hipStreamSynchronize(st));
      grid = sj_plan(hb, hb + 8, e2, G, why);
      ntab = (long long)hb[6];
      if (!grid && method == 1) return pa_fail(ctx, "pa_surfjoin_merge: the grid path cannot be taken: " + why);
    }
    if (grid) {
      u64 *hash, *shash;
      int *idx, *sidx;
      double* P;
      SJ_TRY(sf_need(S, pa_surf::B_UKEY, (size_t)nM, hash));
      SJ_TRY(sf_need(S, pa_surf::B_UKS, (size_t)nM, shash));
      SJ_TRY(sf_need(S, pa_surf::B_RIDX, (size_t)nM, idx));
      SJ_TRY(sf_need(S, pa_surf::B_RS, (size_t)nM, sidx));
      SJ_TRY(sf_need(S, pa_surf::B_DKEY, 3 * (size_t)nM, P));
      SF_LAUNCH(k_sj_keys, nM, nM, S->V, G, hash, idx);
      SJ_TRY(sf_sort_pairs(S, hash, shash, idx, sidx, (size_t)nM, 64));  // stable: equal hashes stay in the order of j
      SF_LAUNCH(k_sj_sorted, nM, nM, sidx, S->V, P);
      SF_LAUNCH(k_sj_probe, nS, nS, T->V, nM, (int)ntab, shash, sidx, P, G, e2, dup, (int*)(aux + 16));
      int wide = 0;
      SF_HIP(hipMemcpyAsync(&wide, aux + 16, sizeof(int), hipMemcpyDeviceToHost, st));
      SF_HIP(hipStreamSynchronize(st));
      if (wide) {
        if (method == 1) return pa_fail(ctx, "pa_surfjoin_merge: the grid path cannot be taken: a probe spans more than 4 cells");
        grid = false; ntab = 0;
      }
    } else {
      ntab = 0;
    }
    if (grid) {
      path = 1;
    } else {
      path = 2;
      SF_LAUNCH(k_sj_brute, 64LL * nS, nS, T->V, nM, S->V, e2, dup);
    }
  }
  SF_LAUNCH(k_sj_flags, nS, nS, dup, isnew);
  SJ_TRY(sf_scan(S, isnew, newid, (size_t)nS));
  long long nnew = 0;
  SJ_TRY(sf_total(S, isnew, newid, nS, &nnew));
  rec[2] = ntab; rec[3] = path; rec[4] = nS - nnew;
  if (nnew == 0) {  // cnt == nNodesM (:210): nothing is appended, the elements of S included
    SF_HIP(hipGetLastError());
    return done(0);
  }
  const long long nW = (long long)nM + nnew, nEW = nEM + nES;
  if (nW > 0x7fffffffLL || 3 * nEW > 0x7fffffffLL) return pa_fail(ctx, "pa_surfjoin_merge: the result would have more than 2^31 - 1 nodes or 3 * nelts");
  double* W = nullptr;
  int* Gf = nullptr;
  SF_HIP(hipMalloc((void**)&W, std::max<size_t>((size_t)nW * (size_t)nc, 1) * sizeof(double)));
  if (hipMalloc((void**)&Gf, std::max<size_t>(3 * (size_t)nEW, 1) * sizeof(int)) != hipSuccess) { (void)hipFree(W); return pa_fail(ctx, "pa_surfjoin_merge: out of memory"); }
  const long long nvM = (long long)nM * nc, nvS = (long long)nS * nc;
  SF_LAUNCH(k_sj_copy_cols, nvM, nvM, (long long)nM, nW, S->V, W);
  SF_LAUNCH(k_sj_new_cols, nvS, nvS, (long long)nS, (long long)nM, nW, T->V, isnew, newid, W);
  SF_LAUNCH(k_sj_copy_int, 3 * nEM, 3 * nEM, S->F, Gf);
  SF_LAUNCH(k_sj_new_elts, 3 * nES, 3 * nES, T->F, dup, newid, nM, Gf + 3 * nEM);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipFree(W); (void)hipFree(Gf); return pa_fail(ctx, std::string("pa_surfjoin_merge: ") + hipGetErrorString(e)); }
  (void)hipFree(S->V); (void)hipFree(S->F);
  S->V = W; S->F = Gf; S->nN = nW; S->nE = nEW;
  rec[5] = nnew; rec[6] = nES;
  return done(1);
}

extern "C" int pa_surfjoin_scale(pa_ctx* ctx, pa_surf* S, int n, const int32_t* comps, const double* vals) {
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surfjoin_scale: null argument, or the object belongs to another context");
  if (n < 0 || (n > 0 && (!comps || !vals))) return pa_fail(ctx, "pa_surfjoin_scale: null or negative argument");
  for (int k = 0; k < n; ++k)
    if (comps[k] < 0 || comps[k] >= S->nc) return pa_fail(ctx, "pa_surfjoin_scale: component " + std::to_string(comps[k]) + " is not one of the " + std::to_string(S->nc) + " node components");
  hipStream_t st = ctx->stream;
  int launches = 0;
  S->sliced = false; S->nsegs = 0; S->nverts = 0;  // a slice it held was of other values
  sj_rec(S, 5);
  for (int k = 0; k < n; ++k) SF_LAUNCH(k_sj_scale, S->nN, S->nN, S->V + (long long)comps[k] * S->nN, vals[k]);  // in list order, on one stream
  SF_HIP(hipGetLastError());
  SF_HIP(hipStreamSynchronize(st));
  S->rec[1] = (long long)n * S->nN; S->rec[7] = launches;
  return 0;
}

extern "C" pa_surf* pa_surfjoin_product(pa_ctx* ctx, const pa_surf* S, int n, const int32_t* comps) {
  PaBind bind_(ctx);
  auto bad = [&](const std::string& m) -> pa_surf* { if (ctx) ctx->err = m; return nullptr; };
  if (!sf_own(ctx, S)) return bad("pa_surfjoin_product: null argument, or the object belongs to another context");
  if (n < 1 || n > 32 || !comps) return bad("pa_surfjoin_product: takes 1 to 32 components");
  SjComps C;
  C.n = n;
  for (int k = 0; k < n; ++k) {
    if (comps[k] < 0 || comps[k] >= S->nc) return bad("pa_surfjoin_product: component " + std::to_string(comps[k]) + " is not one of the " + std::to_string(S->nc) + " node components");
    C.c[k] = comps[k];
  }
  pa_surf* R = sj_new(ctx, S->nN, S->nE, 1);
  if (!R) return nullptr;
  auto run = [&]() -> int {
    hipStream_t st = ctx->stream;
    int launches = 0;
    SF_LAUNCH(k_sj_product, S->nN, S->nN, S->V, C, R->V);
    SF_LAUNCH(k_sj_copy_int, 3 * S->nE, 3 * S->nE, S->F, R->F);
    SF_HIP(hipGetLastError());
    SF_HIP(hipStreamSynchronize(st));
    sj_rec(R, 6);
    R->rec[1] = S->nN; R->rec[7] = launches;
    return 0;
  };
  if (run() != 0) { const std::string keep = ctx->err; pa_surf_destroy(R); ctx->err = keep; return nullptr; }
  return R;
}

extern "C" pa_surf* pa_surfjoin_select(pa_ctx* ctx, const pa_surf* L, const pa_surf* R_or_null, int nsel, const int32_t* which, const int32_t* comps) {
  PaBind bind_(ctx);
  const pa_surf* S = L;
  const pa_surf* R = R_or_null;
  auto bad = [&](const std::string& m) -> pa_surf* { if (ctx) ctx->err = m; return nullptr; };
  if (!sf_own(ctx, S) || (R && !sf_own(ctx, R))) return bad("pa_surfjoin_select: null argument, or an object belongs to another context");
  if (nsel < 1 || !which || !comps) return bad("pa_surfjoin_select: needs at least one component");
  if (R && R->nE != S->nE) return bad("pa_surfjoin_select: MEF files not compible (the element counts differ: " + std::to_string(S->nE) + " and " + std::to_string(R->nE) + ")");
  if (R && R->nN != S->nN) return bad("pa_surfjoin_select: the node counts differ: " + std::to_string(S->nN) + " and " + std::to_string(R->nN));
  for (int k = 0; k < nsel; ++k) {
    if (which[k] != 0 && which[k] != 1) return bad("pa_surfjoin_select: which is 0 (L) or 1 (R)");
    if (which[k] == 1 && !R) return bad("pa_surfjoin_select: a component of R is asked for, and there is no R");
    const int nc = which[k] ? R->nc : S->nc;
    if (comps[k] < 0 || comps[k] >= nc) return bad("pa_surfjoin_select: component " + std::to_string(comps[k]) + " is not one of the " + std::to_string(nc) + " node components of " + (which[k] ? "R" : "L"));
  }
  pa_surf* O = sj_new(ctx, S->nN, S->nE, nsel);
  if (!O) return nullptr;
  auto run = [&]() -> int {
    hipStream_t st = ctx->stream;
    int launches = 0;
    for (int k = 0; k < nsel; ++k) SF_LAUNCH(k_sj_copy_col, S->nN, S->nN, (which[k] ? R->V : S->V) + (long long)comps[k] * S->nN, O->V + (long long)k * S->nN);
    SF_LAUNCH(k_sj_copy_int, 3 * S->nE, 3 * S->nE, S->F, O->F);
    SF_HIP(hipGetLastError());
    SF_HIP(hipStreamSynchronize(st));
    sj_rec(O, 7);
    O->rec[1] = (long long)nsel * S->nN; O->rec[7] = launches;
    return 0;
  };
  if (run() != 0) { const std::string keep = ctx->err; pa_surf_destroy(O); ctx->err = keep; return nullptr; }
  return O;
}
