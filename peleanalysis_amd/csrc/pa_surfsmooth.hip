// pa_surfsmooth.hip -- smoothing one node field over the surface handle of pa_surf.h (smoothMEF.cpp).  With d the
// smoothed component and (n0, n1, n2) the nodes of element e in file order:
//   weights    w_e = ((A[n0] + A[n1]) + A[n2]) * (1./3) of an area component (:249-256), or the triangle's own area by the written
//              expression of triangle_area (:160-194)
//   values     q_e = ((d[n0] + d[n1]) + d[n2]) * (1./3)
//   incidence  ONE stable radix sort of the pairs (node, 3e + q): behind every node its entries stand in ascending 3e + q, hence in
//              ascending element id; an element that names a node twice stands there twice, side by side
//   N(e)       buildNodeNeighbors (:94-131): one thread per element merges the three ascending incidence lists of its nodes and drops
//              itself and repeats -- a count pass, a scan, and a fill pass that also forms W_e = w_e + sum of w_nb in that order
//   iterate    nsmooth Jacobi launches, one thread per element: q'_e = ((w_e*q_e) + sum of (w_nb*q_nb)) / W_e, nb ascending, read from the
//              other buffer of a ping-pong pair; !(W_e > 0) keeps q_e
//   nodes      one thread per node walks its incidence list: Wn = sum of w_e, Sn = sum of (w_e*q_e), each element once, the sums begun
//              with their first term; d[n] = Sn / Wn where Wn > 0
// The neighbour lists are STORED as a CSR of element ids and w_nb is gathered, not kept next to the index (DESIGN.md 3.18 counts the
// bytes).  No thread relies on a bound of the valence: every list is walked by a loop to its end.
// Every floating-point value is computed by ONE thread in a written order (the file is built with -ffp-contract=off); atomics combine
// only integer counts and a maximum.  The same input gives the same bytes: those of tests/surfsmooth_ref.py.
#include <cmath>
#include "pa_surf.h"

namespace {
__device__ __forceinline__ u64 sm_wave_sum(u64 v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ u64 sm_wave_max(u64 v) { for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o); v = w > v ? w : v; } return v; }

__global__ __launch_bounds__(256) void k_sm_pairs(int n3, const int* F, u64* key, int* val) {
  const int t = sc_item();
  if (t >= n3) return;
  key[t] = (u64)F[t];
  val[t] = t;
}
// noff[n] = the first sorted entry whose node is not below n, for n = 0 .. nN (noff[nN] = n3)
__global__ __launch_bounds__(256) void k_sm_nodeoff(int nN, int n3, const u64* skey, int* noff) {
  const int n = sc_item();
  if (n > nN) return;
  int a = 0, b = n3;
  while (a < b) {
    const int m = (int)(((long long)a + b) >> 1);
    if (skey[m] < (u64)n) a = m + 1; else b = m;
  }
  noff[n] = a;
}
__global__ __launch_bounds__(256) void k_sm_weights(int nE, long long nN, const int* F, const double* V, const double* d, const double* A, double* w, double* q) {
  const int e = sc_item();
  if (e >= nE) return;
  const long long a = F[3LL * e], b = F[3LL * e + 1], c = F[3LL * e + 2];
  if (A) {
    w[e] = ((A[a] + A[b]) + A[c]) * (1. / 3);
  } else {
    const double R1x = V[b] - V[a], R1y = V[nN + b] - V[nN + a], R1z = V[2 * nN + b] - V[2 * nN + a];
    const double R2x = V[c] - V[a], R2y = V[nN + c] - V[nN + a], R2z = V[2 * nN + c] - V[2 * nN + a];
    const double R3x = R1y * R2z - R2y * R1z;
    const double R3y = R1z * R2x - R2z * R1x;
    const double R3z = R1x * R2y - R2x * R1y;
    const double res = ((0.0 + R3x * R3x) + R3y * R3y) + R3z * R3z;
    w[e] = 0.5 * sqrt(res);
  }
  q[e] = ((d[a] + d[b]) + d[c]) * (1. / 3);
}
// the merge of the three incidence lists of element e: emit(k, nb) for the k-th neighbour in ascending id; -> |N(e)|
template <class Emit> __device__ __forceinline__ int sm_merge(int e, const int* F, const int* noff, const int* sval, Emit emit) {
  int p[3], end[3];
  for (int j = 0; j < 3; ++j) {
    const int n = F[3LL * e + j];
    p[j] = noff[n]; end[j] = noff[n + 1];
  }
  int last = -1, cnt = 0;
  for (;;) {
    int h[3], m = 0x7fffffff;
    for (int j = 0; j < 3; ++j) {
      h[j] = p[j] < end[j] ? sval[p[j]] / 3 : 0x7fffffff;
      m = h[j] < m ? h[j] : m;
    }
    if (m == 0x7fffffff) break;
    for (int j = 0; j < 3; ++j) if (h[j] == m) ++p[j];
    if (m != e && m != last) { emit(cnt, m); ++cnt; }
    last = m;
  }
  return cnt;
}
// cnt[e] = |N(e)| for e < nE, cnt[nE] = 0 (the scan then leaves the total in off[nE]); tot[0] += |N(e)|, tot[1] = the largest
__global__ __launch_bounds__(256) void k_sm_count(int nE, const int* F, const int* noff, const int* sval, int* cnt, u64* tot) {
  const int e = sc_item();
  u64 c = 0;
  if (e < nE) {
    c = (u64)sm_merge(e, F, noff, sval, [](int, int) {});
    cnt[e] = (int)c;
  } else if (e == nE) {
    cnt[e] = 0;
  }
  const u64 s = sm_wave_sum(c), m = sm_wave_max(c);
  if ((threadIdx.x & 63) == 0 && s) { atomicAdd(&tot[0], s); atomicMax(&tot[1], m); }
}
__global__ __launch_bounds__(256) void k_sm_fill(int nE, const int* F, const int* noff, const int* sval, const int* off, const double* w, int* adj, double* wsum) {
  const int e = sc_item();
  if (e >= nE) return;
  int* out = adj + off[e];
  double W = w[e];
  sm_merge(e, F, noff, sval, [&](int k, int nb) { out[k] = nb; W = W + w[nb]; });
  wsum[e] = W;
}
__global__ __launch_bounds__(256) void k_sm_iter(int nE, const int* off, const int* adj, const double* w, const double* wsum, const double* q, double* qn) {
  const int e = sc_item();
  if (e >= nE) return;
  const double W = wsum[e], qe = q[e];
  double r = qe;
  if (W > 0) {
    double s = w[e] * qe;
    const int b = off[e + 1];
    for (int k = off[e]; k < b; ++k) { const int nb = adj[k]; s = s + w[nb] * q[nb]; }
    r = s / W;
  }
  qn[e] = r;
}
__global__ __launch_bounds__(256) void k_sm_nodes(int nN, const int* noff, const int* sval, const double* w, const double* q, double* d, u64* written) {
  const int n = sc_item();
  u64 did = 0;
  if (n < nN) {
    double Wn = 0.0, Sn = 0.0;
    int last = -1;
    const int b = noff[n + 1];
    for (int i = noff[n]; i < b; ++i) {
      const int e = sval[i] / 3;
      if (e == last) continue;
      const double we = w[e], t = we * q[e];
      if (last < 0) { Wn = we; Sn = t; } else { Wn = Wn + we; Sn = Sn + t; }
      last = e;
    }
    if (last >= 0 && Wn > 0) { d[n] = Sn / Wn; did = 1; }
  }
  did = sm_wave_sum(did);
  if ((threadIdx.x & 63) == 0 && did) atomicAdd(written, did);
}

#define SM_TRY(call)           \
  do {                         \
    const int rc_ = (call);    \
    if (rc_ != 0) return rc_;  \
  } while (0)
}  // namespace

extern "C" int pa_surfsmooth_run(pa_ctx* ctx, pa_surf* S, int comp, int area_comp, int nsmooth) {
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surfsmooth_run: null argument, or the object belongs to another context");
  if (comp < 0 || comp >= S->nc) return pa_fail(ctx, "pa_surfsmooth_run: component " + std::to_string(comp) + " is not one of the " + std::to_string(S->nc) + " node components");
  if (nsmooth < 0) return pa_fail(ctx, "pa_surfsmooth_run: nSmooth is negative");
  const bool by_comp = area_comp >= 0 && area_comp < S->nc;
  if (!by_comp && S->nc < 3) return pa_fail(ctx, "pa_surfsmooth_run: the triangle areas need the node coordinates x, y, z as the first three components, the surface has " + std::to_string(S->nc));
  if (3 * S->nE > 0x7fffffffLL || S->nN > 0x7fffffffLL) return pa_fail(ctx, "pa_surfsmooth_run: more than 2^31 - 1 nodes or 3 * nelts");
  hipStream_t st = ctx->stream;
  int launches = 0;
  const int nE = (int)S->nE, nN = (int)S->nN, n3 = 3 * nE;
  // A call that fails leaves the handle as it was: the scratch used before the last refusal holds nothing that pa_surf_slice_read or
  // pa_surfsmooth_read reads, and `done` runs only where the call succeeds.
  int64_t rec[8] = {8, nE, n3, 0, nsmooth, 0, 0, 0};
  auto done = [&](int which_q) {
    S->sliced = false; S->nsegs = 0; S->nverts = 0;  // a slice it held was of other values
    S->sm_q = which_q;
    rec[7] = launches;
    for (int k = 0; k < 8; ++k) S->rec[k] = rec[k];
    return 0;
  };
  int* off;
  SM_TRY(sf_need(S, pa_surf::B_SM_OFF, (size_t)nE + 1, off));
  if (nE == 0) {  // no element: every node keeps its value
    SF_HIP(hipMemsetAsync(off, 0, sizeof(int), st));
    SF_HIP(hipStreamSynchronize(st));
    return done(0);
  }
  u64 *key, *skey, *aux;
  int *val, *sval, *noff, *cnt;
  SM_TRY(sf_need(S, pa_surf::B_UKEY, (size_t)n3, key));
  SM_TRY(sf_need(S, pa_surf::B_UKS, (size_t)n3, skey));
  SM_TRY(sf_need(S, pa_surf::B_RIDX, (size_t)n3, val));
  SM_TRY(sf_need(S, pa_surf::B_RS, (size_t)n3, sval));
  SM_TRY(sf_need(S, pa_surf::B_HSTART, (size_t)nN + 1, noff));
  SM_TRY(sf_need(S, pa_surf::B_FLAG, (size_t)nE + 1, cnt));
  SM_TRY(sf_need(S, pa_surf::B_AUX, 4, aux));  // [0] the sum of |N(e)|, [1] the largest, [2] nodes written
  SF_HIP(hipMemsetAsync(aux, 0, 4 * sizeof(u64), st));
  int bits = 1;
  while (bits < 32 && (1LL << bits) < nN) ++bits;
  SF_LAUNCH(k_sm_pairs, n3, n3, S->F, key, val);
  SM_TRY(sf_sort_pairs(S, key, skey, val, sval, (size_t)n3, bits));  // stable: behind a node, 3e + q ascends
  SF_LAUNCH(k_sm_nodeoff, (long long)nN + 1, nN, n3, skey, noff);
  SF_LAUNCH(k_sm_count, (long long)nE + 1, nE, S->F, noff, sval, cnt, aux);
  u64 tot[2] = {0, 0};
  SF_HIP(hipGetLastError());
  SF_HIP(hipMemcpyAsync(tot, aux, sizeof tot, hipMemcpyDeviceToHost, st));
  SF_HIP(hipStreamSynchronize(st));
  if (tot[0] > 0x7fffffffull) return pa_fail(ctx, "pa_surfsmooth_run: the neighbour lists would hold more than 2^31 - 1 entries (" + std::to_string(tot[0]) + ")");
  rec[3] = (int64_t)tot[0]; rec[6] = (int64_t)tot[1];
  int* adj;
  double *w, *wsum, *q[2];
  SM_TRY(sf_need(S, pa_surf::B_SM_ADJ, (size_t)tot[0], adj));
  SM_TRY(sf_need(S, pa_surf::B_SM_W, (size_t)nE, w));
  SM_TRY(sf_need(S, pa_surf::B_SM_WSUM, (size_t)nE, wsum));
  SM_TRY(sf_need(S, pa_surf::B_SM_Q0, (size_t)nE, q[0]));
  SM_TRY(sf_need(S, pa_surf::B_SM_Q1, (size_t)nE, q[1]));
  double* d = S->V + (long long)comp * S->nN;
  SM_TRY(sf_scan(S, cnt, off, (size_t)nE + 1));
  SF_LAUNCH(k_sm_weights, nE, nE, S->nN, S->F, S->V, d, by_comp ? S->V + (long long)area_comp * S->nN : (const double*)nullptr, w, q[0]);
  SF_LAUNCH(k_sm_fill, nE, nE, S->F, noff, sval, off, w, adj, wsum);
  int cur = 0;
  for (int it = 0; it < nsmooth; ++it, cur ^= 1) SF_LAUNCH(k_sm_iter, nE, nE, off, adj, w, wsum, q[cur], q[cur ^ 1]);
  SF_LAUNCH(k_sm_nodes, nN, nN, noff, sval, w, q[cur], d, aux + 2);
  u64 written = 0;
  SF_HIP(hipGetLastError());
  SF_HIP(hipMemcpyAsync(&written, aux + 2, sizeof written, hipMemcpyDeviceToHost, st));
  SF_HIP(hipStreamSynchronize(st));
  rec[5] = (int64_t)written;
  return done(cur);
}

extern "C" int pa_surfsmooth_read(pa_ctx* ctx, const pa_surf* S, int32_t* nbr_off, int32_t* nbr_adj, double* w, double* q) {
  PaBind bind_(ctx);
  if (!sf_own(ctx, S)) return pa_fail(ctx, "pa_surfsmooth_read: null argument, or the object belongs to another context");
  if (S->rec[0] != 8) return pa_fail(ctx, "pa_surfsmooth_read: the last operation on the surface was not a smooth");
  hipStream_t st = ctx->stream;
  const size_t nE = (size_t)S->rec[1], nA = (size_t)S->rec[3];
  auto dev = [&](int which) { return S->buf[which].p; };
  if (nbr_off) SF_HIP(hipMemcpyAsync(nbr_off, dev(pa_surf::B_SM_OFF), (nE + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (nbr_adj && nA > 0) SF_HIP(hipMemcpyAsync(nbr_adj, dev(pa_surf::B_SM_ADJ), nA * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (w && nE > 0) SF_HIP(hipMemcpyAsync(w, dev(pa_surf::B_SM_W), nE * sizeof(double), hipMemcpyDeviceToHost, st));
  if (q && nE > 0) SF_HIP(hipMemcpyAsync(q, dev(S->sm_q ? pa_surf::B_SM_Q1 : pa_surf::B_SM_Q0), nE * sizeof(double), hipMemcpyDeviceToHost, st));
  SF_HIP(hipStreamSynchronize(st));
  return 0;
}
