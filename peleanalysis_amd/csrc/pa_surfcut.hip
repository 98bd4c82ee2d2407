// pa_surfcut.hip -- cutting and trimming a triangulated surface that stays in device memory (sliceMEF.cpp, trimMEFgen.cpp).
// A pa_surf (pa_surf.h: the handle is shared with pa_surfjoin.hip) holds the nodes COMPONENT-MAJOR, V[c * nN + n] (the classification reads one dense column, the gathers read whole columns),
// and the elements as 0-based int triples F[3 * e + q].
//   slice   1. case     bit q of case[e] = V[comp][node q of e] < val (strict); a flag where the case is not 0 or 7
//           2. scan     exclusive scan of the flags: segment s of element e, in element order
//           3. requests two per segment, (apex, other) in the reference's order: an UNORDERED key min << 32 | max and the DIRECTED pair
//           4. sort     stable radix sort of (unordered key, request index): the head of a run is the FIRST request for that vertex
//                       (by element, then first or second end) and gives the direction it lives under (sliceMEF.cpp:607-630)
//           5. number   the unique vertices sorted by their directed pair: rank = the reference's map order (sliceMEF.cpp:260-268)
//           6. ends     segs[r] = rank of the vertex of request r
//           7. values   VI_doIt (sliceMEF.cpp:581-605) in the direction of the first request, one thread per value
//           8. CSR      vertex -> its segments in ascending segment index: the runs of step 4, laid out in rank order
//   trim    node flags (any condition holds -> removed), element flags (all three nodes kept), used flags (plain stores of 1), three
//           exclusive scans, order-preserving gathers of the node columns and of the renumbered elements.  No atomics place anything.
//   area    every triangle's area by ONE thread with the written expression of surface_area (trimMEFgen.cpp:76-84), a striding grid;
//           min and max as unsigned minima / maxima of the bit patterns (areas are not negative); the total is the 192-bit fixed-point
//           sum of pa_fixed192.h, scaled from the largest area, rounded ONCE.  The reference adds serially, in element order: its total
//           can differ in the last bits.
// Every floating-point value is computed by ONE thread in a written order (the file is built with -ffp-contract=off); lane groups and
// atomics combine only flags, integer minima / maxima and fixed-point limbs.  The same input gives the same bytes: those of
// tests/surfcut_ref.py.
#include <cfloat>
#include "pa_fixed192.h"
#include "pa_surf.h"

namespace {
constexpr double SC_EPS = 1.0e-8;  // epsilon_DEF of sliceMEF.cpp
constexpr int AR_BLOCKS = 2048;    // the area kernels stride with a grid of at most this many blocks (256 CUs x 8)
enum { SC_LT = 0, SC_LE = 1, SC_GT = 2, SC_GE = 3, SC_EQ = 4 };

__device__ __forceinline__ bool sc_holds(double d, int op, double v) {
  return ((op == SC_LT) & (d < v)) | ((op == SC_LE) & (d <= v)) | ((op == SC_GT) & (d > v)) | ((op == SC_GE) & (d >= v)) | ((op == SC_EQ) & (d == v));
}

// ---------------------------------------------------------------- slice
__global__ __launch_bounds__(256) void k_sc_case(int nE, const int* F, const double* col, double val, unsigned char* cs, int* flag) {
  const int e = sc_item();
  if (e >= nE) return;
  int c = 0;
  if (col[F[3LL * e]] < val) c |= 1;
  if (col[F[3LL * e + 1]] < val) c |= 2;
  if (col[F[3LL * e + 2]] < val) c |= 4;
  cs[e] = (unsigned char)c;
  flag[e] = (c != 0 && c != 7) ? 1 : 0;
}
// cases 1/6: (p0,p1),(p0,p2); 2/5: (p1,p0),(p1,p2); 3/4: (p2,p0),(p2,p1)  (sliceMEF.cpp:658-674)
__global__ __launch_bounds__(256) void k_sc_requests(int nE, const int* F, const unsigned char* cs, const int* flag, const int* pos, int* src, u64* ukey, u64* dkey,
                                                     int* ridx) {
  const int e = sc_item();
  if (e >= nE || !flag[e]) return;
  const int s = pos[e];
  const int p0 = F[3LL * e], p1 = F[3LL * e + 1], p2 = F[3LL * e + 2];
  // which node is the apex, two bits per case: 1 -> 0, 2 -> 1, 3 -> 2, 4 -> 2, 5 -> 1, 6 -> 0 (selects, no branches)
  const int aq = (0x690 >> (2 * (int)cs[e])) & 3;
  const int a = aq == 0 ? p0 : (aq == 1 ? p1 : p2);
  const int o1 = aq == 0 ? p1 : p0;
  const int o2 = aq == 2 ? p1 : p2;
  src[s] = e;
  const int o[2] = {o1, o2};
  for (int q = 0; q < 2; ++q) {
    const long long r = 2LL * s + q;
    const unsigned lo = (unsigned)min(a, o[q]), hi = (unsigned)max(a, o[q]);
    ukey[r] = ((u64)lo << 32) | hi;
    dkey[r] = ((u64)(unsigned)a << 32) | (unsigned)o[q];
    ridx[r] = (int)r;
  }
}
__global__ __launch_bounds__(256) void k_sc_heads(int nR, const u64* uks, int* head) {
  const int i = sc_item();
  if (i < nR) head[i] = (i == 0 || uks[i] != uks[i - 1]) ? 1 : 0;
}
// uid of sorted request i = hscan[i] + head[i] - 1; the head of run u records its position and the directed pair of the first request
__global__ __launch_bounds__(256) void k_sc_unique(int nR, const int* head, const int* hscan, const int* rs, const u64* dkey, int* requ, int* hstart, u64* vdk,
                                                   int* vu) {
  const int i = sc_item();
  if (i >= nR) return;
  const int u = hscan[i] + head[i] - 1;
  requ[rs[i]] = u;
  if (head[i]) { hstart[u] = i; vdk[u] = dkey[rs[i]]; vu[u] = u; }
}
__global__ __launch_bounds__(256) void k_sc_rank(int nV, const int* perm, const int* hstart, int nR, int* rank, int* len) {
  const int j = sc_item();
  if (j >= nV) return;
  const int u = perm[j];
  rank[u] = j;
  len[j] = (u + 1 < nV ? hstart[u + 1] : nR) - hstart[u];
}
__global__ __launch_bounds__(256) void k_sc_ends(int nR, const int* requ, const int* rank, int32_t* segs) {
  const int r = sc_item();
  if (r < nR) segs[r] = rank[requ[r]];
}
__global__ __launch_bounds__(256) void k_sc_adj(int nR, const int* head, const int* hscan, const int* rs, const int* hstart, const int* rank, const int* off, int nV,
                                                int32_t* adj, int32_t* off_out) {
  const int i = sc_item();
  if (i >= nR) return;
  const int u = hscan[i] + head[i] - 1;
  const int j = rank[u];
  adj[off[j] + (i - hstart[u])] = rs[i] >> 1;
  if (head[i]) off_out[j] = off[j];
  if (i == 0) off_out[nV] = nR;
}
__global__ __launch_bounds__(256) void k_sc_pairs(int nV, const u64* vdks, int32_t* pairs) {
  const int j = sc_item();
  if (j >= nV) return;
  pairs[2LL * j] = (int32_t)(vdks[j] >> 32);
  pairs[2LL * j + 1] = (int32_t)(vdks[j] & 0xffffffffull);
}
// VI_doIt (sliceMEF.cpp:581-605): thread t computes component t % nc of vertex t / nc
__global__ __launch_bounds__(256) void k_sc_values(long long n, int nc, long long nN, const double* V, const u64* vdks, int comp, double val, double* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const long long j = t / nc;
  const int c = (int)(t - j * nc);
  const long long p1 = (long long)(vdks[j] >> 32), p2 = (long long)(vdks[j] & 0xffffffffull);
  const double v1 = V[(long long)comp * nN + p1], v2 = V[(long long)comp * nN + p2];
  const double a = V[(long long)c * nN + p1];
  double r;
  if (fabs(val - v1) < SC_EPS) r = a;
  else if (fabs(val - v2) < SC_EPS) r = V[(long long)c * nN + p2];
  else if (fabs(v1 - v2) < SC_EPS) r = a;
  else {
    const double mu = (val - v1) / (v2 - v1);
    const double b = V[(long long)c * nN + p2];
    r = a + mu * (b - a);
  }
  out[t] = r;
}

// ---------------------------------------------------------------- trim
__global__ __launch_bounds__(256) void k_tr_nodes(int nN, const double* V, int ncond, const int* comps, const int* ops, const double* vals, int use_rxy, int rxy_op,
                                                  double rxy, int* keep) {
  const int n = sc_item();
  if (n >= nN) return;
  bool rem = false;
  for (int i = 0; i < ncond; ++i) rem = rem || sc_holds(V[(long long)comps[i] * nN + n], ops[i], vals[i]);
  if (use_rxy) {
    const double x = V[n], y = V[(long long)nN + n];
    const double r = sqrt(x * x + y * y);
    rem = rem || sc_holds(r, rxy_op, rxy);
  }
  keep[n] = rem ? 0 : 1;
}
__global__ __launch_bounds__(256) void k_tr_elts(int nE, const int* F, const int* keep, int* ekeep, int* used) {
  const int e = sc_item();
  if (e >= nE) return;
  const int a = F[3LL * e], b = F[3LL * e + 1], c = F[3LL * e + 2];
  const int k = (keep[a] && keep[b] && keep[c]) ? 1 : 0;
  ekeep[e] = k;
  if (k) { used[a] = 1; used[b] = 1; used[c] = 1; }
}
__global__ __launch_bounds__(256) void k_tr_gather_nodes(long long n, long long nN, long long nNew, const int* used, const int* nid, const double* V, double* W) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const long long c = t / nN, i = t - c * nN;
  if (used[i]) W[c * nNew + nid[i]] = V[t];
}
__global__ __launch_bounds__(256) void k_tr_gather_elts(int nE, const int* F, const int* ekeep, const int* eid, const int* nid, int* G) {
  const int e = sc_item();
  if (e >= nE || !ekeep[e]) return;
  const long long o = 3LL * eid[e];
  for (int q = 0; q < 3; ++q) G[o + q] = nid[F[3LL * e + q]];
}

// ---------------------------------------------------------------- area, read-back
__device__ __forceinline__ u64 sc_wave_min(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o); v = w < v ? w : v; } return v; }
__device__ __forceinline__ u64 sc_wave_max(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o); v = w > v ? w : v; } return v; }
// trimMEFgen.cpp:76-84; mm[0] = min bits, mm[1] = max bits, mm[2] = elements whose area is not finite
__global__ __launch_bounds__(256) void k_ar_area(int nE, long long nN, const int* F, const double* V, double* area, u64* mm) {
  u64 lo = ~0ull, hi = 0ull;
  u64 bad = 0;
  // a grid of at most AR_BLOCKS blocks strides over the elements: one atomic minimum / maximum per wave of the grid, not per 64 elements
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nE; e += (long long)gridDim.x * 256) {
    const long long a = F[3LL * e], b = F[3LL * e + 1], c = F[3LL * e + 2];
    const double p0x = V[a], p0y = V[nN + a], p0z = V[2 * nN + a];
    const double p1x = V[b], p1y = V[nN + b], p1z = V[2 * nN + b];
    const double p2x = V[c], p2y = V[nN + c], p2z = V[2 * nN + c];
    const double t0 = (p1y - p0y) * (p2z - p0z) - (p1z - p0z) * (p2y - p0y);
    const double t1 = (p1z - p0z) * (p2x - p0x) - (p1x - p0x) * (p2z - p0z);
    const double t2 = (p1x - p0x) * (p2y - p0y) - (p1y - p0y) * (p2x - p0x);
    const double A = 0.5 * sqrt(t0 * t0 + t1 * t1 + t2 * t2);
    area[e] = A;
    if (A <= DBL_MAX) {
      const u64 ab = (u64)__double_as_longlong(A);
      lo = ab < lo ? ab : lo; hi = ab > hi ? ab : hi;
    } else {
      bad += 1;
    }
  }
  lo = sc_wave_min(lo); hi = sc_wave_max(hi); bad = wave_sum_u64(bad);
  if ((threadIdx.x & 63) == 0) {
    if (lo != ~0ull) { atomicMin(&mm[0], lo); atomicMax(&mm[1], hi); }
    if (bad) atomicAdd(&mm[2], bad);
  }
}
__global__ __launch_bounds__(256) void k_ar_sum(int nE, const double* area, int s, u64* limbs, int* flag) {
  int f = 0;
  U192 v = {{0, 0, 0}};
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nE; e += (long long)gridDim.x * 256) u192_add(v, to_fixed(area[e], s, f));  // integers: any order
  v = wave_sum_u192(v);
  if ((threadIdx.x & 63) == 0 && !u192_zero(v)) u192_atomic_add(limbs, v);
  if (f) atomicOr(flag, f);
}
__global__ __launch_bounds__(256) void k_sf_nodes_out(long long n, int nc, long long nN, const double* V, double* out) {  // out[node][comp]
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const long long i = t / nc, c = t - i * nc;
  out[t] = V[c * nN + i];
}
__global__ __launch_bounds__(256) void k_sf_elts_out(long long n, const int* F, int32_t* out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < n) out[t] = F[t] + 1;
}

int sf_key_bits(long long nN) {  // the directed and unordered keys hold node ids below nN in both halves
  int b = 1;
  while (b < 32 && (1LL << b) < nN) ++b;
  return 32 + b;
}
}  // namespace

extern "C" void pa_surf_destroy(pa_surf* S) {
  if (!S) return;
  PaBind bind_(S->ctx);
  for (DevBufG& b : S->buf) if (b.p) (void)hipFree(b.p);
  if (S->V) (void)hipFree(S->V);
  if (S->F) (void)hipFree(S->F);
  delete S;
}

extern "C" pa_surf* pa_surf_create(pa_ctx* ctx, int64_t nnodes, int ncomp, const double* nodes, int64_t nelts, const int32_t* elts) {
  PaBind bind_(ctx);
  auto bad = [&](const std::string& m) -> pa_surf* { if (ctx) ctx->err = m; return nullptr; };
  if (!ctx || nnodes < 0 || nelts < 0 || (nnodes > 0 && !nodes) || (nelts > 0 && !elts)) return bad("pa_surf_create: null or negative argument");
  if (ncomp < 3) return bad("pa_surf_create: a surface needs the node coordinates x, y, z as its first three components (ncomp = " + std::to_string(ncomp) + ")");
  if (nnodes > 0x7fffffffLL || 3 * nelts > 0x7fffffffLL) return bad("pa_surf_create: more than 2^31 - 1 nodes or 3 * nelts");
  std::vector<int> F((size_t)(3 * nelts));
  for (int64_t t = 0; t < nelts; ++t)
    for (int q = 0; q < 3; ++q) {
      const int32_t a = elts[3 * t + q];
      if (a < 1 || a > nnodes) return bad("pa_surf_create: element " + std::to_string(t + 1) + " names a node that does not exist");
      F[(size_t)(3 * t + q)] = a - 1;
    }
  std::vector<double> V((size_t)nnodes * (size_t)ncomp);
  for (int64_t i = 0; i < nnodes; ++i)
    for (int c = 0; c < ncomp; ++c) V[(size_t)c * (size_t)nnodes + (size_t)i] = nodes[(size_t)i * (size_t)ncomp + (size_t)c];
  pa_surf* S = new pa_surf;
  S->ctx = ctx; S->nN = nnodes; S->nE = nelts; S->nc = ncomp;
  auto build = [&]() -> int {
    hipStream_t st = ctx->stream;
    SF_HIP(hipMalloc((void**)&S->V, std::max<size_t>(V.size(), 1) * sizeof(double)));
    SF_HIP(hipMalloc((void**)&S->F, std::max<size_t>(F.size(), 1) * sizeof(int)));
    if (!V.empty()) SF_HIP(hipMemcpyAsync(S->V, V.data(), V.size() * sizeof(double), hipMemcpyHostToDevice, st));
    if (!F.empty()) SF_HIP(hipMemcpyAsync(S->F, F.data(), F.size() * sizeof(int), hipMemcpyHostToDevice, st));
    SF_HIP(hipStreamSynchronize(st));
    return 0;
  };
  if (build() != 0) {
    const std::string keep = ctx->err;
    pa_surf_destroy(S);
    ctx->err = keep;
    return nullptr;
  }
  return S;
}

extern "C" int pa_surf_counts(const pa_surf* S, int64_t* nnodes, int64_t* nelts, int* ncomp) {
  if (!S) return 1;
  if (nnodes) *nnodes = S->nN;
  if (nelts) *nelts = S->nE;
  if (ncomp) *ncomp = S->nc;
  return 0;
}

extern "C" int pa_surf_last_launch(const pa_surf* S, int64_t rec[8]) {
  if (!S || !rec) return 1;
  for (int i = 0; i < 8; ++i) rec[i] = S->rec[i];
  return 0;
}

extern "C" int pa_surf_read(pa_ctx* ctx, pa_surf* S, double* nodes, int32_t* elts) {  // not const: the handle's scratch is rewritten
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surf_read: null argument, or the object belongs to another context");
  hipStream_t st = ctx->stream;
  int launches = 0;
  const long long nv = S->nN * S->nc, ne = 3 * S->nE;
  if (nodes && nv > 0) {
    double* d = nullptr;
    if (sf_need(S, pa_surf::B_AUX, (size_t)nv, d)) return 1;
    SF_LAUNCH(k_sf_nodes_out, nv, nv, S->nc, S->nN, S->V, d);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(nodes, d, (size_t)nv * sizeof(double), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
  }
  if (elts && ne > 0) {
    int32_t* d = nullptr;
    if (sf_need(S, pa_surf::B_AUX, (size_t)ne, d)) return 1;
    SF_LAUNCH(k_sf_elts_out, ne, ne, S->F, d);
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(elts, d, (size_t)ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
  }
  (void)launches;
  return 0;
}

extern "C" int pa_surf_slice(pa_ctx* ctx, pa_surf* S, int comp, double val, int64_t* nverts, int64_t* nsegs) {
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surf_slice: null argument, or the object belongs to another context");
  if (comp < 0 || comp >= S->nc) return pa_fail(ctx, "pa_surf_slice: component " + std::to_string(comp) + " is not one of the " + std::to_string(S->nc) + " node components");
  if (!(val == val)) return pa_fail(ctx, "pa_surf_slice: the location is not a number");
  hipStream_t st = ctx->stream;
  int launches = 0;
  const int nE = (int)S->nE;
  S->sliced = false; S->nsegs = 0; S->nverts = 0;
  for (int64_t& r : S->rec) r = 0;
  S->rec[0] = 1; S->rec[1] = nE;
  const double* col = S->V + (long long)comp * S->nN;
  unsigned char* cs; int *flag, *pos;
  if (sf_need(S, pa_surf::B_CS, (size_t)nE, cs) || sf_need(S, pa_surf::B_FLAG, (size_t)nE, flag) || sf_need(S, pa_surf::B_POS, (size_t)nE, pos)) return 1;
  long long ns = 0;
  if (nE > 0) {
    SF_LAUNCH(k_sc_case, nE, nE, S->F, col, val, cs, flag);
    if (sf_scan(S, flag, pos, (size_t)nE)) return 1;
    if (sf_total(S, flag, pos, nE, &ns)) return 1;
  }
  const long long nR = 2 * ns;
  long long nV = 0;
  if (ns > 0) {
    int *src, *ridx, *rs, *head, *hscan, *requ, *hstart, *vu, *perm, *rank, *len, *off;
    u64 *ukey, *dkey, *uks, *vdk, *vdks;
    int32_t *segs, *adj, *offout, *pairs;
    if (sf_need(S, pa_surf::B_SRC, (size_t)ns, src) || sf_need(S, pa_surf::B_UKEY, (size_t)nR, ukey) || sf_need(S, pa_surf::B_DKEY, (size_t)nR, dkey) ||
        sf_need(S, pa_surf::B_RIDX, (size_t)nR, ridx) || sf_need(S, pa_surf::B_UKS, (size_t)nR, uks) || sf_need(S, pa_surf::B_RS, (size_t)nR, rs) ||
        sf_need(S, pa_surf::B_HEAD, (size_t)nR, head) || sf_need(S, pa_surf::B_HSCAN, (size_t)nR, hscan) || sf_need(S, pa_surf::B_REQU, (size_t)nR, requ) ||
        sf_need(S, pa_surf::B_SEGS, (size_t)nR, segs) || sf_need(S, pa_surf::B_ADJ, (size_t)nR, adj))
      return 1;
    const int bits = sf_key_bits(S->nN);
    SF_LAUNCH(k_sc_requests, nE, nE, S->F, cs, flag, pos, src, ukey, dkey, ridx);
    if (sf_sort_pairs(S, ukey, uks, ridx, rs, (size_t)nR, bits)) return 1;
    SF_LAUNCH(k_sc_heads, nR, (int)nR, uks, head);
    if (sf_scan(S, head, hscan, (size_t)nR)) return 1;
    if (sf_total(S, head, hscan, nR, &nV)) return 1;
    if (nV < 1 || nV > nR) return pa_fail(ctx, "pa_surf_slice: vertex count out of range");
    if (sf_need(S, pa_surf::B_HSTART, (size_t)nV, hstart) || sf_need(S, pa_surf::B_VDK, (size_t)nV, vdk) || sf_need(S, pa_surf::B_VU, (size_t)nV, vu) ||
        sf_need(S, pa_surf::B_VDKS, (size_t)nV, vdks) || sf_need(S, pa_surf::B_PERM, (size_t)nV, perm) || sf_need(S, pa_surf::B_RANK, (size_t)nV, rank) ||
        sf_need(S, pa_surf::B_LEN, (size_t)nV, len) || sf_need(S, pa_surf::B_OFF, (size_t)nV, off) || sf_need(S, pa_surf::B_OFFOUT, (size_t)nV + 1, offout) ||
        sf_need(S, pa_surf::B_PAIRS, 2 * (size_t)nV, pairs))
      return 1;
    double* verts;
    if (sf_need(S, pa_surf::B_VERTS, (size_t)nV * (size_t)S->nc, verts)) return 1;
    SF_LAUNCH(k_sc_unique, nR, (int)nR, head, hscan, rs, dkey, requ, hstart, vdk, vu);
    if (sf_sort_pairs(S, vdk, vdks, vu, perm, (size_t)nV, bits)) return 1;
    SF_LAUNCH(k_sc_rank, nV, (int)nV, perm, hstart, (int)nR, rank, len);
    if (sf_scan(S, len, off, (size_t)nV)) return 1;
    SF_LAUNCH(k_sc_ends, nR, (int)nR, requ, rank, segs);
    SF_LAUNCH(k_sc_adj, nR, (int)nR, head, hscan, rs, hstart, rank, off, (int)nV, adj, offout);
    SF_LAUNCH(k_sc_pairs, nV, (int)nV, vdks, pairs);
    const long long nval = nV * S->nc;
    SF_LAUNCH(k_sc_values, nval, nval, S->nc, S->nN, S->V, vdks, comp, val, verts);
    SF_HIP(hipGetLastError());
    SF_HIP(hipStreamSynchronize(st));
  }
  S->sliced = true; S->nsegs = ns; S->nverts = nV;
  S->rec[2] = ns; S->rec[3] = nR; S->rec[4] = nV; S->rec[5] = nV * S->nc; S->rec[6] = nR; S->rec[7] = launches;
  if (nverts) *nverts = nV;
  if (nsegs) *nsegs = ns;
  return 0;
}

extern "C" int pa_surf_slice_read(pa_ctx* ctx, const pa_surf* S, double* verts, int32_t* pairs, int32_t* segs, int32_t* src_elt, int32_t* csr_off, int32_t* csr_adj) {
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surf_slice_read: null argument, or the object belongs to another context");
  if (!S->sliced) return pa_fail(ctx, "pa_surf_slice_read: no slice has been computed since the surface was created or trimmed");
  hipStream_t st = ctx->stream;
  const size_t nV = (size_t)S->nverts, ns = (size_t)S->nsegs;
  if (csr_off && ns == 0) csr_off[0] = 0;
  if (ns > 0) {
    auto dev = [&](int which) { return S->buf[which].p; };
    if (verts) SF_HIP(hipMemcpyAsync(verts, dev(pa_surf::B_VERTS), nV * (size_t)S->nc * sizeof(double), hipMemcpyDeviceToHost, st));
    if (pairs) SF_HIP(hipMemcpyAsync(pairs, dev(pa_surf::B_PAIRS), 2 * nV * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (segs) SF_HIP(hipMemcpyAsync(segs, dev(pa_surf::B_SEGS), 2 * ns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (src_elt) SF_HIP(hipMemcpyAsync(src_elt, dev(pa_surf::B_SRC), ns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (csr_off) SF_HIP(hipMemcpyAsync(csr_off, dev(pa_surf::B_OFFOUT), (nV + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (csr_adj) SF_HIP(hipMemcpyAsync(csr_adj, dev(pa_surf::B_ADJ), 2 * ns * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
  }
  return 0;
}

extern "C" int pa_surf_trim(pa_ctx* ctx, pa_surf* S, int ncond, const int32_t* comps, const int32_t* ops, const double* vals, double rxy, int rxy_op,
                            int64_t* nodes_unused) {
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surf_trim: null argument, or the object belongs to another context");
  if (ncond < 0 || (ncond > 0 && (!comps || !ops || !vals))) return pa_fail(ctx, "pa_surf_trim: null or negative argument");
  for (int i = 0; i < ncond; ++i) {
    if (comps[i] < 0 || comps[i] >= S->nc) return pa_fail(ctx, "pa_surf_trim: component " + std::to_string(comps[i]) + " is not one of the " + std::to_string(S->nc) + " node components");
    if (ops[i] < SC_LT || ops[i] > SC_EQ) return pa_fail(ctx, "pa_surf_trim: Bad signs data. Use one of [lt,le,gt,ge,eq]");
  }
  const int use_rxy = rxy >= 0 ? 1 : 0;
  if (use_rxy && S->nc < 3) return pa_fail(ctx, "pa_surf_trim: RXY needs the node coordinates x, y, z as the first three components, the surface has " + std::to_string(S->nc));
  if (use_rxy && (rxy_op < SC_LT || rxy_op > SC_EQ)) return pa_fail(ctx, "pa_surf_trim: Bad sign data.  Use one of [lt,le,gt,ge,eq]");
  hipStream_t st = ctx->stream;
  int launches = 0;
  const int nN = (int)S->nN, nE = (int)S->nE;
  S->sliced = false;
  for (int64_t& r : S->rec) r = 0;
  S->rec[0] = 2; S->rec[1] = nN; S->rec[2] = nE;
  // scratch: B_FLAG keep, B_POS its scan, B_HEAD used, B_HSCAN nid, B_REQU ekeep, B_RIDX eid; B_AUX the conditions
  int *keep, *kscan, *used, *nid, *ekeep, *eid;
  if (sf_need(S, pa_surf::B_FLAG, (size_t)nN, keep) || sf_need(S, pa_surf::B_POS, (size_t)nN, kscan) || sf_need(S, pa_surf::B_HEAD, (size_t)nN, used) ||
      sf_need(S, pa_surf::B_HSCAN, (size_t)nN, nid) || sf_need(S, pa_surf::B_REQU, (size_t)nE, ekeep) || sf_need(S, pa_surf::B_RIDX, (size_t)nE, eid))
    return 1;
  unsigned char* aux;
  const size_t ncs = (size_t)std::max(ncond, 1);
  if (sf_need(S, pa_surf::B_AUX, ncs * 16 + 64, aux)) return 1;
  double* dvals = (double*)aux;
  int* dcomps = (int*)(aux + ncs * 8);
  int* dops = (int*)(aux + ncs * 12);
  if (ncond > 0) {
    std::vector<int> hc(comps, comps + ncond), ho(ops, ops + ncond);
    SF_HIP(hipMemcpyAsync(dvals, vals, (size_t)ncond * sizeof(double), hipMemcpyHostToDevice, st));
    SF_HIP(hipMemcpyAsync(dcomps, hc.data(), (size_t)ncond * sizeof(int), hipMemcpyHostToDevice, st));
    SF_HIP(hipMemcpyAsync(dops, ho.data(), (size_t)ncond * sizeof(int), hipMemcpyHostToDevice, st));
    SF_HIP(hipStreamSynchronize(st));  // the host vectors leave scope
  }
  long long nkeep = 0, nused = 0, nek = 0;
  if (nN > 0) {
    SF_HIP(hipMemsetAsync(used, 0, (size_t)nN * sizeof(int), st));
    SF_LAUNCH(k_tr_nodes, nN, nN, S->V, ncond, dcomps, dops, dvals, use_rxy, rxy_op, rxy, keep);
    SF_LAUNCH(k_tr_elts, nE, nE, S->F, keep, ekeep, used);
    if (sf_scan(S, keep, kscan, (size_t)nN) || sf_scan(S, used, nid, (size_t)nN)) return 1;
    if (nE > 0 && sf_scan(S, ekeep, eid, (size_t)nE)) return 1;
    if (sf_total(S, keep, kscan, nN, &nkeep) || sf_total(S, used, nid, nN, &nused) || sf_total(S, ekeep, eid, nE, &nek)) return 1;
  }
  double* W = nullptr;
  int* G = nullptr;
  SF_HIP(hipMalloc((void**)&W, std::max<size_t>((size_t)nused * (size_t)S->nc, 1) * sizeof(double)));
  if (hipMalloc((void**)&G, std::max<size_t>(3 * (size_t)nek, 1) * sizeof(int)) != hipSuccess) { (void)hipFree(W); return pa_fail(ctx, "pa_surf_trim: out of memory"); }
  const long long nall = (long long)nN * S->nc;
  SF_LAUNCH(k_tr_gather_nodes, nall, nall, (long long)nN, nused, used, nid, S->V, W);
  SF_LAUNCH(k_tr_gather_elts, nE, nE, S->F, ekeep, eid, nid, G);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) { (void)hipFree(W); (void)hipFree(G); return pa_fail(ctx, std::string("pa_surf_trim: ") + hipGetErrorString(e)); }
  (void)hipFree(S->V); (void)hipFree(S->F);
  S->V = W; S->F = G; S->nN = nused; S->nE = nek;
  S->rec[3] = nkeep; S->rec[4] = nused; S->rec[5] = nek; S->rec[6] = nused * S->nc; S->rec[7] = launches;
  if (nodes_unused) *nodes_unused = nkeep - nused;
  return 0;
}

extern "C" int pa_surf_area(pa_ctx* ctx, pa_surf* S, double* total, double* amin, double* amax) {  // not const: scratch and the launch record
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surf_area: null argument, or the object belongs to another context");
  if (S->nc < 3) return pa_fail(ctx, "pa_surf_area: needs the node coordinates x, y, z as the first three components, the surface has " + std::to_string(S->nc));
  hipStream_t st = ctx->stream;
  int launches = 0;
  const int nE = (int)S->nE;
  for (int64_t& r : S->rec) r = 0;
  S->rec[0] = 3; S->rec[1] = nE;
  double tot = 0.0, lo = 0.0, hi = 0.0;
  if (nE > 0) {
    unsigned char* aux;  // B_AUX holds nothing of a slice: its results stay readable
    if (sf_need(S, pa_surf::B_AUX, (size_t)nE * sizeof(double) + 64, aux)) return 1;
    u64* mm = (u64*)aux;          // [0] min bits, [1] max bits, [2] not finite, [3..5] limbs, [6] flag
    double* area = (double*)(aux + 64);
    u64 init[8] = {~0ull, 0, 0, 0, 0, 0, 0, 0};
    SF_HIP(hipMemcpyAsync(mm, init, sizeof init, hipMemcpyHostToDevice, st));
    const long long span = std::min<long long>((nE + 3LL) / 4, (long long)AR_BLOCKS * 256);  // threads of the striding grid: four elements each, or more
    SF_LAUNCH(k_ar_area, span, nE, S->nN, S->F, S->V, area, mm);
    u64 h[8];
    SF_HIP(hipMemcpyAsync(h, mm, sizeof h, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if (h[2] != 0) return pa_fail(ctx, "pa_surf_area: " + std::to_string(h[2]) + " elements have an area that is not finite");
    memcpy(&lo, &h[0], 8); memcpy(&hi, &h[1], 8);
    const int s = scale_of(hi);
    SF_LAUNCH(k_ar_sum, span, nE, area, s, mm + 3, (int*)(mm + 6));
    SF_HIP(hipGetLastError());
    SF_HIP(hipMemcpyAsync(h, mm, sizeof h, hipMemcpyDeviceToHost, st));
    SF_HIP(hipStreamSynchronize(st));
    if ((int)(h[6] & 0xffffffffull) != 0) return pa_fail(ctx, "pa_surf_area: a term of the area sum cannot be held in fixed point");
    tot = from_fixed(h + 3, s);
    S->rec[2] = nE;
  }
  S->rec[7] = launches;
  if (total) *total = tot;
  if (amin) *amin = lo;
  if (amax) *amax = hi;
  return 0;
}
