// pa_decimate.hip -- quadric edge-collapse decimation of a triangulated surface (the job of the reference's qslim wrapper,
// Tools/qslim/main.cpp; mixkit itself is not in the reference tree, so this is an algorithm of our own: DESIGN.md 3.14).
// qslim pulls one contraction at a time from a heap; here a ROUND contracts an independent set of the cheapest edges at once:
//   1. topology   live faces (stable scan of the valid flags) -> 3 undirected edge keys (min << 32 | max) per face, radix sort,
//                 run-length encode: edge id = rank, faces per edge = run length; vertex -> face CSR (sort of vertex << 32 | face)
//                 and vertex -> neighbour CSR (sort of both directions of every edge), rows found by binary search; an edge whose
//                 face count is not 1 or 2 locks both of its ends, an edge with one face marks both as boundary vertices
//   2. candidates a group of DC_G lanes per edge: locks, the boundary rule, the link condition (common neighbours == faces of the
//                 edge; the two faces beside the edge's own must not collapse onto each other), placement and cost from
//                 Q[a] + Q[b], no surviving face of either star may turn its normal by 90 degrees or more;
//                 key = float_bits((float)cost) << 32 | edge id: unsigned order is cost order and every key is unique
//   3. budget     radix sort of the keys; with R = valid faces - target only the ceil(R / 2) cheapest stay candidates
//   4. selection  vk[v] = min key of the candidate edges at v (64-bit integer atomicMin), rk[v] = min of vk over the closed 1-ring
//                 of v (CSR gather); an edge is selected when key == rk[a] == rk[b]
//   5. cut        in key order, an edge is applied while the faces removed before it are fewer than R
//   6. apply      P[a] = vbar, Q[a] = Q[a] + Q[b], b -> a in every live face, faces that held both die
// Every floating-point value is computed by ONE thread in a written order (the file is built with -ffp-contract=off); what lane
// groups and atomics combine are logical flags, integer counts and minima of unique integer keys, which do not depend on an order.
// No floating-point atomics; no kernel waits for another workgroup.  tests/decimate_ref.py restates all of it; the results are its
// bits, round by round.
#include <cfloat>
#include <climits>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include "pa_internal.h"

namespace {
typedef unsigned long long u64;
constexpr u64 DC_MAX = ~0ull;
constexpr double DC_DET_EPS = 1.0e-12;  // -O 3: the solve is accepted when det(A) > DC_DET_EPS * trace(A)^3
constexpr int DC_G = 8;                 // lanes that share one edge (candidate test) or one vertex (1-ring minimum)
enum { DC_NLOCKED = 0, DC_NCAND = 1, DC_NSEL = 2, DC_NAPPLIED = 3, DC_NREMOVED = 4, DC_NE = 5, DC_NUSED = 6 };

struct V3 { double x, y, z; };
__device__ __forceinline__ V3 ld3(const double* P, int v) { return V3{P[3LL * v], P[3LL * v + 1], P[3LL * v + 2]}; }
__device__ __forceinline__ V3 sub3(const V3& a, const V3& b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double dot3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross3(const V3& u, const V3& v) { return V3{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x}; }

// w * (n, d)(n, d)^T / (n . n), d = -n . p: the plane through p with the unnormalised normal n; false for n = 0
__device__ __forceinline__ bool plane_quadric(const V3& n, const V3& p, double w, double k[10]) {
  const double nn = dot3(n, n);
  if (!(nn > 0.0)) return false;
  const double d = -dot3(n, p);
  const double s = w / nn;
  k[0] = s * (n.x * n.x); k[1] = s * (n.x * n.y); k[2] = s * (n.x * n.z); k[3] = s * (n.x * d);
  k[4] = s * (n.y * n.y); k[5] = s * (n.y * n.z); k[6] = s * (n.y * d);
  k[7] = s * (n.z * n.z); k[8] = s * (n.z * d); k[9] = s * (d * d);
  return true;
}
__device__ __forceinline__ double qcost(const double q[10], const V3& v) {
  const double x = v.x, y = v.y, z = v.z;
  return q[0] * x * x + 2.0 * q[1] * x * y + 2.0 * q[2] * x * z + 2.0 * q[3] * x + q[4] * y * y + 2.0 * q[5] * y * z + 2.0 * q[6] * y
         + q[7] * z * z + 2.0 * q[8] * z + q[9];
}
__device__ __forceinline__ bool optimal(const double q[10], V3& v) {  // cofactors of the symmetric 3 x 3 block
  const double a00 = q[0], a01 = q[1], a02 = q[2], b0 = q[3], a11 = q[4], a12 = q[5], b1 = q[6], a22 = q[7], b2 = q[8];
  const double c00 = a11 * a22 - a12 * a12;
  const double c01 = a02 * a12 - a01 * a22;
  const double c02 = a01 * a12 - a02 * a11;
  const double c11 = a00 * a22 - a02 * a02;
  const double c12 = a01 * a02 - a00 * a12;
  const double c22 = a00 * a11 - a01 * a01;
  const double det = a00 * c00 + a01 * c01 + a02 * c02;
  const double t = a00 + a11 + a22;
  if (!(det > DC_DET_EPS * (t * t * t))) return false;
  v.x = -(c00 * b0 + c01 * b1 + c02 * b2) / det;
  v.y = -(c01 * b0 + c11 * b1 + c12 * b2) / det;
  v.z = -(c02 * b0 + c12 * b1 + c22 * b2) / det;
  return true;
}
__device__ __forceinline__ int lower_bound(const u64* k, int lo, int hi, u64 want) {  // first i in [lo, hi) with k[i] >= want, else hi
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (k[mid] < want) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ u64 edge_key(int u, int v) { return u < v ? ((u64)(unsigned)u << 32) | (unsigned)v : ((u64)(unsigned)v << 32) | (unsigned)u; }
// reductions over the DC_G lanes of a group (aligned in the wave); called where the whole wave has reconverged
__device__ __forceinline__ int grp_sum(int x) { for (int m = 1; m < DC_G; m <<= 1) x += __shfl_xor(x, m); return x; }
__device__ __forceinline__ int grp_min(int x) { for (int m = 1; m < DC_G; m <<= 1) x = min(x, __shfl_xor(x, m)); return x; }
__device__ __forceinline__ int grp_max(int x) { for (int m = 1; m < DC_G; m <<= 1) x = max(x, __shfl_xor(x, m)); return x; }
__device__ __forceinline__ u64 grp_min64(u64 x) {
  for (int m = 1; m < DC_G; m <<= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(x & 0xffffffffull), m), hi = (unsigned)__shfl_xor((int)(unsigned)(x >> 32), m);
    const u64 y = ((u64)hi << 32) | lo;
    x = y < x ? y : x;
  }
  return x;
}

// ---------------------------------------------------------------- topology
__global__ __launch_bounds__(256) void k_dc_live(int nF, const int* valid, const int* pos, int* live) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f < nF && valid[f]) live[pos[f]] = f;
}
__global__ __launch_bounds__(256) void k_dc_keys(int nL, const int* live, const int* F, u64* ek, u64* vfk) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nL) return;
  const int f = live[j];
  const int a = F[3LL * f], b = F[3LL * f + 1], c = F[3LL * f + 2];
  ek[3LL * j] = edge_key(a, b); ek[3LL * j + 1] = edge_key(b, c); ek[3LL * j + 2] = edge_key(c, a);
  vfk[3LL * j] = ((u64)(unsigned)a << 32) | (unsigned)f; vfk[3LL * j + 1] = ((u64)(unsigned)b << 32) | (unsigned)f; vfk[3LL * j + 2] = ((u64)(unsigned)c << 32) | (unsigned)f;
}
__global__ __launch_bounds__(256) void k_dc_rowstart(int nV, const u64* keys, int n, int* start) {  // start[0 .. nV]
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v <= nV) start[v] = lower_bound(keys, 0, n, (u64)(unsigned)v << 32);
}
__global__ __launch_bounds__(256) void k_dc_nbkeys(int nE, const u64* ekey, u64* nbk) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nE) return;
  const u64 k = ekey[e];
  nbk[2LL * e] = k;
  nbk[2LL * e + 1] = (k << 32) | (k >> 32);
}
__global__ __launch_bounds__(256) void k_dc_flags(int nE, const u64* ekey, const int* ecnt, unsigned char* lock, unsigned char* bnd, int* cnt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= nE) return;
  const int a = (int)(ekey[e] >> 32), b = (int)(ekey[e] & 0xffffffffull), c = ecnt[e];
  if (c != 1 && c != 2) { lock[a] = 1; lock[b] = 1; atomicAdd(&cnt[DC_NLOCKED], 1); }
  if (c == 1) { bnd[a] = 1; bnd[b] = 1; }
}

// ---------------------------------------------------------------- initial quadrics: one thread per vertex, faces in ascending order
__global__ __launch_bounds__(256) void k_dc_quadrics(int nV, const double* P, const int* F, const int* vstart, const u64* vfs, int nE, const u64* ekey,
                                                     const int* ecnt, double bw, int weighting, double* Q) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nV) return;
  double q[10], k[10];
  for (int i = 0; i < 10; ++i) q[i] = 0.0;
  const int s = vstart[v], t = vstart[v + 1];
  for (int i = s; i < t; ++i) {
    const int f = (int)(vfs[i] & 0xffffffffull);
    const V3 p0 = ld3(P, F[3LL * f]), p1 = ld3(P, F[3LL * f + 1]), p2 = ld3(P, F[3LL * f + 2]);
    const V3 n = cross3(sub3(p1, p0), sub3(p2, p0));
    double w = 1.0;
    if (weighting == 1) w = 0.5 * sqrt(dot3(n, n));
    if (plane_quadric(n, p0, w, k))
      for (int c = 0; c < 10; ++c) q[c] = q[c] + k[c];
  }
  for (int i = s; i < t; ++i) {  // the boundary planes: within a face the edge leaving v, then the edge arriving at v
    const int f = (int)(vfs[i] & 0xffffffffull);
    const int w3[3] = {F[3LL * f], F[3LL * f + 1], F[3LL * f + 2]};
    const int at = w3[0] == v ? 0 : (w3[1] == v ? 1 : 2);
    const V3 p0 = ld3(P, w3[0]), p1 = ld3(P, w3[1]), p2 = ld3(P, w3[2]);
    const V3 m = cross3(sub3(p1, p0), sub3(p2, p0));
    for (int side = 0; side < 2; ++side) {
      const int p = side == 0 ? w3[at] : w3[(at + 2) % 3], r = side == 0 ? w3[(at + 1) % 3] : w3[at];
      const u64 key = edge_key(p, r);
      const int id = lower_bound(ekey, 0, nE, key);
      if (id >= nE || ekey[id] != key || ecnt[id] != 1) continue;
      const V3 pp = ld3(P, p);
      const V3 e = sub3(ld3(P, r), pp);
      const double w = weighting == 1 ? bw * dot3(e, e) : bw;
      if (plane_quadric(cross3(e, m), pp, w, k))
        for (int c = 0; c < 10; ++c) q[c] = q[c] + k[c];
    }
  }
  for (int c = 0; c < 10; ++c) Q[(long long)c * nV + v] = q[c];
}

// ---------------------------------------------------------------- step 2: DC_G lanes per edge
__global__ __launch_bounds__(256) void k_dc_candidates(int nE, const u64* ekey, const int* ecnt, const unsigned char* lock, const unsigned char* bnd,
                                                       const int* vstart, const u64* vfs, const int* nstart, const u64* nbs, const int* F, const double* P,
                                                       const double* Q, int nV, int placement, u64* ckey, double* vbar, int* cnt) {
  const int e = blockIdx.x * (256 / DC_G) + (int)(threadIdx.x / DC_G);
  const int lane = threadIdx.x % DC_G;
  const bool act = e < nE;
  int a = 0, b = 0, c = 0;
  if (act) { a = (int)(ekey[e] >> 32); b = (int)(ekey[e] & 0xffffffffull); c = ecnt[e]; }
  bool ok = act && (c == 1 || c == 2) && !lock[a] && !lock[b] && !(c == 2 && bnd[a] && bnd[b]);
  // pass 1: common neighbours, and the third vertices of the edge's own faces
  int common = 0, tmin = INT_MAX, tmax = -1;
  if (ok) {
    const int b0 = nstart[b], b1 = nstart[b + 1];
    for (int i = nstart[a] + lane; i < nstart[a + 1]; i += DC_G) {
      const u64 want = ((u64)(unsigned)b << 32) | (nbs[i] & 0xffffffffull);
      const int p = lower_bound(nbs, b0, b1, want);
      if (p < b1 && nbs[p] == want) ++common;
    }
    for (int i = vstart[a] + lane; i < vstart[a + 1]; i += DC_G) {
      const int f = (int)(vfs[i] & 0xffffffffull);
      const int w0 = F[3LL * f], w1 = F[3LL * f + 1], w2 = F[3LL * f + 2];
      if (w0 == b || w1 == b || w2 == b) {
        const int t = (w0 != a && w0 != b) ? w0 : ((w1 != a && w1 != b) ? w1 : w2);
        tmin = min(tmin, t); tmax = max(tmax, t);
      }
    }
  }
  common = grp_sum(common); tmin = grp_min(tmin); tmax = grp_max(tmax);
  ok = ok && common == c;
  // placement and cost (every lane of the group computes the same values)
  V3 vb = V3{0.0, 0.0, 0.0};
  double cost = 0.0;
  if (ok) {
    double q[10];
    for (int i = 0; i < 10; ++i) q[i] = Q[(long long)i * nV + a] + Q[(long long)i * nV + b];
    bool solved = false;
    if (placement == 3) solved = optimal(q, vb);
    if (solved) {
      cost = qcost(q, vb);
    } else {  // the cheapest of a, b and (unless -O 0) the midpoint; ties go to the first
      const V3 pa = ld3(P, a), pb = ld3(P, b);
      vb = pa; cost = qcost(q, pa);
      const double cb = qcost(q, pb);
      if (cb < cost) { vb = pb; cost = cb; }
      if (placement != 0) {
        const V3 pm = V3{0.5 * (pa.x + pb.x), 0.5 * (pa.y + pb.y), 0.5 * (pa.z + pb.z)};
        const double cm = qcost(q, pm);
        if (cm < cost) { vb = pm; cost = cm; }
      }
    }
    if (!(cost <= DBL_MAX && cost >= -DBL_MAX)) ok = false;
    if (cost < 0.0) cost = 0.0;
  }
  // pass 2: the surviving faces of both stars
  int bad = 0, hasA = 0, hasB = 0;
  if (ok) {
    const int sa = vstart[a], na = vstart[a + 1] - sa, sb = vstart[b], nb = vstart[b + 1] - sb;
    for (int i = lane; i < na + nb; i += DC_G) {
      const bool ina = i < na;
      const int f = (int)(vfs[ina ? sa + i : sb + (i - na)] & 0xffffffffull);
      const int w0 = F[3LL * f], w1 = F[3LL * f + 1], w2 = F[3LL * f + 2];
      const bool fa = w0 == a || w1 == a || w2 == a, fb = w0 == b || w1 == b || w2 == b;
      if (fa && fb) continue;  // dies with the edge
      if (c == 2 && (w0 == tmin || w1 == tmin || w2 == tmin) && (w0 == tmax || w1 == tmax || w2 == tmax)) { if (ina) hasA = 1; else hasB = 1; }
      const V3 p0 = ld3(P, w0), p1 = ld3(P, w1), p2 = ld3(P, w2);
      const V3 on = cross3(sub3(p1, p0), sub3(p2, p0));
      if (dot3(on, on) == 0.0) continue;
      const V3 r0 = (w0 == a || w0 == b) ? vb : p0, r1 = (w1 == a || w1 == b) ? vb : p1, r2 = (w2 == a || w2 == b) ? vb : p2;
      const V3 nn = cross3(sub3(r1, r0), sub3(r2, r0));
      if (!(dot3(nn, on) > 0.0)) bad = 1;
    }
  }
  bad = grp_max(bad); hasA = grp_max(hasA); hasB = grp_max(hasB);
  ok = ok && !bad && !(c == 2 && hasA && hasB);
  if (act && lane == 0) {
    ckey[e] = ok ? (((u64)__float_as_uint((float)cost) << 32) | (unsigned)e) : DC_MAX;
    if (ok) {
      vbar[3LL * e] = vb.x; vbar[3LL * e + 1] = vb.y; vbar[3LL * e + 2] = vb.z;
      atomicAdd(&cnt[DC_NCAND], 1);
    }
  }
}

// ---------------------------------------------------------------- steps 4 - 6
__global__ __launch_bounds__(256) void k_dc_vk(int K, const u64* cs, const u64* ekey, u64* vk) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K) return;
  const u64 key = cs[i], ab = ekey[key & 0xffffffffull];
  atomicMin(&vk[ab >> 32], key);
  atomicMin(&vk[ab & 0xffffffffull], key);
}
__global__ __launch_bounds__(256) void k_dc_rk(int nV, const u64* vk, const int* nstart, const u64* nbs, u64* rk) {
  const int v = blockIdx.x * (256 / DC_G) + (int)(threadIdx.x / DC_G);
  const int lane = threadIdx.x % DC_G;
  u64 m = DC_MAX;
  if (v < nV) {
    if (lane == 0) m = vk[v];
    for (int i = nstart[v] + lane; i < nstart[v + 1]; i += DC_G) {
      const u64 x = vk[nbs[i] & 0xffffffffull];
      m = x < m ? x : m;
    }
  }
  m = grp_min64(m);
  if (v < nV && lane == 0) rk[v] = m;
}
__global__ __launch_bounds__(256) void k_dc_select(int K, const u64* cs, const u64* ekey, const int* ecnt, const u64* rk, int* selc, int* cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K) return;
  const u64 key = cs[i];
  const int e = (int)(key & 0xffffffffull);
  const u64 ab = ekey[e];
  const bool sel = rk[ab >> 32] == key && rk[ab & 0xffffffffull] == key;
  selc[i] = sel ? ecnt[e] : 0;
  if (sel) atomicAdd(&cnt[DC_NSEL], 1);
}
__global__ __launch_bounds__(256) void k_dc_apply_v(int K, const u64* cs, const int* selc, const int* pre, long long R, const u64* ekey, const double* vbar,
                                                    double* P, double* Q, int nV, int* remap, int* cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K || selc[i] == 0 || !((long long)pre[i] < R)) return;
  const int e = (int)(cs[i] & 0xffffffffull);
  const int a = (int)(ekey[e] >> 32), b = (int)(ekey[e] & 0xffffffffull);
  P[3LL * a] = vbar[3LL * e]; P[3LL * a + 1] = vbar[3LL * e + 1]; P[3LL * a + 2] = vbar[3LL * e + 2];
  for (int c = 0; c < 10; ++c) Q[(long long)c * nV + a] = Q[(long long)c * nV + a] + Q[(long long)c * nV + b];
  remap[b] = a;
  atomicAdd(&cnt[DC_NAPPLIED], 1);
  atomicAdd(&cnt[DC_NREMOVED], selc[i]);
}
__global__ __launch_bounds__(256) void k_dc_apply_f(int nL, const int* live, const int* remap, int* F, int* valid) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nL) return;
  const int f = live[j];
  int w[3];
  for (int q = 0; q < 3; ++q) {
    w[q] = F[3LL * f + q];
    const int r = remap[w[q]];
    if (r >= 0) { w[q] = r; F[3LL * f + q] = r; }
  }
  if (w[0] == w[1] || w[1] == w[2] || w[0] == w[2]) valid[f] = 0;
}

// ---------------------------------------------------------------- output
__global__ __launch_bounds__(256) void k_dc_mark_used(int nL, const int* live, const int* F, int* used) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nL) return;
  const int f = live[j];
  used[F[3LL * f]] = 1; used[F[3LL * f + 1]] = 1; used[F[3LL * f + 2]] = 1;
}
__global__ __launch_bounds__(256) void k_dc_out_xyz(int nV, const int* used, const int* newid, const double* P, double* out) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nV || !used[v]) return;
  const long long o = 3LL * newid[v];
  out[o] = P[3LL * v]; out[o + 1] = P[3LL * v + 1]; out[o + 2] = P[3LL * v + 2];
}
__global__ __launch_bounds__(256) void k_dc_out_elts(int nL, const int* live, const int* F, const int* newid, int32_t* out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= nL) return;
  const int f = live[j];
  for (int q = 0; q < 3; ++q) out[3LL * j + q] = newid[F[3LL * f + q]] + 1;
}
__global__ __launch_bounds__(256) void k_dc_valid_bytes(int nF, const int* valid, unsigned char* out) {
  const int f = blockIdx.x * 256 + threadIdx.x;
  if (f < nF) out[f] = valid[f] ? 1 : 0;
}

inline dim3 grid_of(long long n, int per = 256) { return dim3((unsigned)((n + per - 1) / per)); }
}  // namespace

struct pa_decimate {
  pa_ctx* ctx = nullptr;
  int nV = 0, nF = 0;
  double bw = 1000.0;
  int weighting = 1, placement = 3;
  int nvalid = 0, nL = 0, nE = 0, nlocked = 0, nused = 0;
  int64_t rounds = 0;
  int64_t rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool topo_fresh = false, live_fresh = false;
  double *P = nullptr, *Q = nullptr, *vbar = nullptr;
  int *F = nullptr, *valid = nullptr, *live = nullptr, *iscr = nullptr, *iscr2 = nullptr, *ecnt = nullptr, *vstart = nullptr, *nstart = nullptr, *selc = nullptr,
      *pre = nullptr, *remap = nullptr, *cnt = nullptr;
  u64 *k1 = nullptr, *k2 = nullptr, *ekey = nullptr, *vfs = nullptr, *nbs = nullptr, *ckey = nullptr, *cs = nullptr, *vk = nullptr, *rk = nullptr;
  unsigned char *lock = nullptr, *bnd = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  std::vector<void*> allocs;
};

namespace {
int dc_fail(pa_ctx* ctx, const std::string& m) { if (ctx) ctx->err = m; return -1; }
#define DC_HIP(call)                                                                                           \
  do {                                                                                                         \
    const hipError_t e_ = (call);                                                                              \
    if (e_ != hipSuccess) return dc_fail(D->ctx, std::string("pa_decimate: " #call ": ") + hipGetErrorString(e_)); \
  } while (0)
#define DC_LAUNCH(kernel, n, per, ...)                                                             \
  do {                                                                                             \
    if ((n) > 0) hipLaunchKernelGGL(kernel, grid_of((n), (per)), dim3(256), 0, st, __VA_ARGS__); \
  } while (0)

template <class T> int dc_alloc(pa_decimate* D, T*& p, size_t n) {
  void* q = nullptr;
  DC_HIP(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
  D->allocs.push_back(q);
  p = (T*)q;
  return 0;
}
int dc_read_cnt(pa_decimate* D, int h[8]) {
  DC_HIP(hipMemcpyAsync(h, D->cnt, 8 * sizeof(int), hipMemcpyDeviceToHost, D->ctx->stream));
  DC_HIP(hipStreamSynchronize(D->ctx->stream));
  return 0;
}
int dc_scan(pa_decimate* D, const int* in, int* out, size_t n) {
  size_t tb = D->tmp_bytes;
  DC_HIP(rocprim::exclusive_scan(D->tmp, tb, in, out, 0, n, rocprim::plus<int>(), D->ctx->stream));
  return 0;
}
int dc_sort(pa_decimate* D, const u64* in, u64* out, size_t n) {
  size_t tb = D->tmp_bytes;
  DC_HIP(rocprim::radix_sort_keys(D->tmp, tb, in, out, n, 0, 64, D->ctx->stream));
  return 0;
}

// the live list: the valid faces in ascending order
int dc_live(pa_decimate* D) {
  if (D->live_fresh) return 0;
  hipStream_t st = D->ctx->stream;
  D->nL = D->nvalid;
  if (D->nF > 0) {
    if (dc_scan(D, D->valid, D->iscr, (size_t)D->nF)) return -1;
    DC_LAUNCH(k_dc_live, D->nF, 256, D->nF, D->valid, D->iscr, D->live);
    int last[2];  // the flags must agree with the count the rounds keep (the faces an applied edge removes = its face count)
    DC_HIP(hipMemcpyAsync(&last[0], D->iscr + (D->nF - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    DC_HIP(hipMemcpyAsync(&last[1], D->valid + (D->nF - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    DC_HIP(hipStreamSynchronize(st));
    if (last[0] + last[1] != D->nvalid) return dc_fail(D->ctx, "pa_decimate: the valid flags do not add up to the face count of the rounds");
  }
  D->live_fresh = true;
  return 0;
}

// step 1
int dc_topology(pa_decimate* D) {
  if (D->topo_fresh) return 0;
  hipStream_t st = D->ctx->stream;
  if (dc_live(D)) return -1;
  const int nL = D->nL, nV = D->nV;
  const long long n3 = 3LL * nL;
  DC_HIP(hipMemsetAsync(D->cnt, 0, 8 * sizeof(int), st));
  DC_HIP(hipMemsetAsync(D->lock, 0, (size_t)std::max(nV, 1), st));
  DC_HIP(hipMemsetAsync(D->bnd, 0, (size_t)std::max(nV, 1), st));
  D->nE = 0; D->nlocked = 0;
  if (n3 > 0) {
    DC_LAUNCH(k_dc_keys, nL, 256, nL, D->live, D->F, D->k1, D->k2);
    if (dc_sort(D, D->k2, D->vfs, (size_t)n3)) return -1;
    if (dc_sort(D, D->k1, D->k2, (size_t)n3)) return -1;
    size_t tb = D->tmp_bytes;
    DC_HIP(rocprim::run_length_encode(D->tmp, tb, D->k2, (unsigned int)n3, D->ekey, D->ecnt, D->cnt + DC_NE, st));
    int h[8];
    if (dc_read_cnt(D, h)) return -1;
    D->nE = h[DC_NE];
    if (D->nE < 0 || D->nE > n3) return dc_fail(D->ctx, "pa_decimate: edge count out of range");
    DC_LAUNCH(k_dc_nbkeys, D->nE, 256, D->nE, D->ekey, D->k1);
    if (dc_sort(D, D->k1, D->nbs, (size_t)(2LL * D->nE))) return -1;
    DC_LAUNCH(k_dc_flags, D->nE, 256, D->nE, D->ekey, D->ecnt, D->lock, D->bnd, D->cnt);
  }
  DC_LAUNCH(k_dc_rowstart, nV + 1, 256, nV, D->vfs, (int)n3, D->vstart);
  DC_LAUNCH(k_dc_rowstart, nV + 1, 256, nV, D->nbs, 2 * D->nE, D->nstart);
  int h[8];
  if (dc_read_cnt(D, h)) return -1;
  D->nlocked = h[DC_NLOCKED];
  DC_HIP(hipGetLastError());
  D->topo_fresh = true;
  return 0;
}

int dc_count_used(pa_decimate* D) {  // vertices the valid faces use: iscr2 = flags, iscr = their exclusive scan
  hipStream_t st = D->ctx->stream;
  if (dc_live(D)) return -1;
  D->nused = 0;
  if (D->nV == 0) return 0;
  DC_HIP(hipMemsetAsync(D->iscr2, 0, (size_t)D->nV * sizeof(int), st));
  DC_LAUNCH(k_dc_mark_used, D->nL, 256, D->nL, D->live, D->F, D->iscr2);
  if (dc_scan(D, D->iscr2, D->iscr, (size_t)D->nV)) return -1;
  int last[2];
  DC_HIP(hipMemcpyAsync(&last[0], D->iscr + (D->nV - 1), sizeof(int), hipMemcpyDeviceToHost, st));
  DC_HIP(hipMemcpyAsync(&last[1], D->iscr2 + (D->nV - 1), sizeof(int), hipMemcpyDeviceToHost, st));
  DC_HIP(hipStreamSynchronize(st));
  D->nused = last[0] + last[1];
  return 0;
}
}  // namespace

extern "C" void pa_decimate_destroy(pa_decimate* D) {
  if (!D) return;
  PaBind bind_(D->ctx);
  for (void* p : D->allocs) (void)hipFree(p);
  delete D;
}

extern "C" pa_decimate* pa_decimate_create(pa_ctx* ctx, int64_t nnodes, const double* xyz, int64_t nelts, const int32_t* elts, double boundary_weight,
                                           int weighting, int placement) {
  PaBind bind_(ctx);
  auto bad = [&](const std::string& m) -> pa_decimate* { if (ctx) ctx->err = m; return nullptr; };
  if (!ctx || nnodes < 0 || nelts < 0 || (nnodes > 0 && !xyz) || (nelts > 0 && !elts)) return bad("pa_decimate_create: null or negative argument");
  if (weighting != 0 && weighting != 1) return bad("pa_decimate_create: weighting must be 0 (uniform) or 1 (area)");
  if (placement != 0 && placement != 1 && placement != 3) return bad("pa_decimate_create: placement must be 0 (endpoints), 1 (endpoints or midpoint) or 3 (optimal)");
  // 3 edge keys per face are sorted with 32-bit positions: more cannot be numbered
  if (nnodes > 0x7fffffffLL || 3 * nelts > 0x7fffffffLL) return bad("pa_decimate_create: more than 2^31 - 1 nodes or edges");
  std::vector<int> F((size_t)(3 * nelts));
  for (int64_t t = 0; t < nelts; ++t) {
    const int32_t a = elts[3 * t], b = elts[3 * t + 1], c = elts[3 * t + 2];
    if (a < 1 || b < 1 || c < 1 || a > nnodes || b > nnodes || c > nnodes)
      return bad("pa_decimate_create: element " + std::to_string(t + 1) + " names a node that does not exist");
    if (a == b || b == c || a == c) return bad("pa_decimate_create: element " + std::to_string(t + 1) + " names a node twice");
    F[(size_t)(3 * t)] = a - 1; F[(size_t)(3 * t + 1)] = b - 1; F[(size_t)(3 * t + 2)] = c - 1;
  }
  pa_decimate* D = new pa_decimate;
  D->ctx = ctx; D->nV = (int)nnodes; D->nF = (int)nelts; D->bw = boundary_weight; D->weighting = weighting; D->placement = placement;
  D->nvalid = D->nF;
  D->rec[7] = D->nF;
  const size_t nV = (size_t)D->nV, nF = (size_t)D->nF, n3 = 3 * nF, n6 = 6 * nF;
  hipStream_t st = ctx->stream;
  auto build = [&]() -> int {
    size_t t1 = 0, t2 = 0, t3 = 0;
    DC_HIP(rocprim::radix_sort_keys(nullptr, t1, (u64*)nullptr, (u64*)nullptr, std::max<size_t>(n6, 1), 0, 64, st));
    DC_HIP(rocprim::exclusive_scan(nullptr, t2, (int*)nullptr, (int*)nullptr, 0, std::max<size_t>(std::max(n3, nV), 1), rocprim::plus<int>(), st));
    DC_HIP(rocprim::run_length_encode(nullptr, t3, (u64*)nullptr, (unsigned int)std::max<size_t>(n3, 1), (u64*)nullptr, (int*)nullptr, (int*)nullptr, st));
    D->tmp_bytes = std::max(std::max(t1, t2), t3) + 256;
    unsigned char* tmpb = nullptr;
    if (dc_alloc(D, tmpb, D->tmp_bytes)) return -1;
    D->tmp = tmpb;
    if (dc_alloc(D, D->P, 3 * nV) || dc_alloc(D, D->Q, 10 * nV) || dc_alloc(D, D->vbar, 3 * n3) || dc_alloc(D, D->F, n3) || dc_alloc(D, D->valid, nF) ||
        dc_alloc(D, D->live, nF) || dc_alloc(D, D->iscr, std::max(n3, nV) + 1) || dc_alloc(D, D->iscr2, std::max(n3, nV) + 1) || dc_alloc(D, D->ecnt, n3) ||
        dc_alloc(D, D->vstart, nV + 1) || dc_alloc(D, D->nstart, nV + 1) || dc_alloc(D, D->selc, n3) || dc_alloc(D, D->pre, n3) || dc_alloc(D, D->remap, nV) ||
        dc_alloc(D, D->cnt, 8) || dc_alloc(D, D->k1, n6) || dc_alloc(D, D->k2, n6) || dc_alloc(D, D->ekey, n3) || dc_alloc(D, D->vfs, n3) ||
        dc_alloc(D, D->nbs, n6) || dc_alloc(D, D->ckey, n3) || dc_alloc(D, D->cs, n3) || dc_alloc(D, D->vk, nV) || dc_alloc(D, D->rk, nV) ||
        dc_alloc(D, D->lock, nV) || dc_alloc(D, D->bnd, nV))
      return -1;
    std::vector<double> P(3 * nV);
    for (size_t i = 0; i < 3 * nV; ++i) P[i] = xyz[i];
    std::vector<int> ones(nF, 1);
    if (nV) DC_HIP(hipMemcpyAsync(D->P, P.data(), 3 * nV * sizeof(double), hipMemcpyHostToDevice, st));
    if (nF) DC_HIP(hipMemcpyAsync(D->F, F.data(), n3 * sizeof(int), hipMemcpyHostToDevice, st));
    if (nF) DC_HIP(hipMemcpyAsync(D->valid, ones.data(), nF * sizeof(int), hipMemcpyHostToDevice, st));
    DC_HIP(hipStreamSynchronize(st));
    if (dc_topology(D)) return -1;
    DC_LAUNCH(k_dc_quadrics, D->nV, 256, D->nV, D->P, D->F, D->vstart, D->vfs, D->nE, D->ekey, D->ecnt, D->bw, D->weighting, D->Q);
    DC_HIP(hipGetLastError());
    if (dc_count_used(D)) return -1;
    return 0;
  };
  if (build() != 0) {
    const std::string keep = ctx->err;
    pa_decimate_destroy(D);
    ctx->err = keep;
    return nullptr;
  }
  return D;
}

extern "C" int pa_decimate_round(pa_ctx* ctx, pa_decimate* D, int64_t face_target) {
  PaBind bind_(ctx);
  if (!ctx || !D || D->ctx != ctx) return dc_fail(ctx, "pa_decimate_round: null argument, or the object belongs to another context");
  const long long target = face_target < 0 ? 0 : face_target;
  if (D->nvalid <= target) return 0;
  hipStream_t st = ctx->stream;
  if (dc_topology(D)) return -1;
  const int nE = D->nE, nV = D->nV, nL = D->nL;
  const long long R = D->nvalid - target, budget = (R + 1) / 2;
  int h[8];
  DC_HIP(hipMemsetAsync(D->cnt, 0, 8 * sizeof(int), st));
  DC_LAUNCH(k_dc_candidates, nE, 256 / DC_G, nE, D->ekey, D->ecnt, D->lock, D->bnd, D->vstart, D->vfs, D->nstart, D->nbs, D->F, D->P, D->Q, nV, D->placement,
            D->ckey, D->vbar, D->cnt);
  if (dc_read_cnt(D, h)) return -1;
  const int ncand = h[DC_NCAND];
  int64_t* rec = D->rec;
  rec[0] = nE; rec[1] = D->nlocked; rec[2] = ncand; rec[3] = budget; rec[4] = 0; rec[5] = 0; rec[6] = 0; rec[7] = D->nvalid;
  if (ncand <= 0) return 0;
  if (dc_sort(D, D->ckey, D->cs, (size_t)nE)) return -1;
  const int K = (int)std::min<long long>(ncand, budget);
  DC_HIP(hipMemsetAsync(D->vk, 0xff, (size_t)nV * sizeof(u64), st));
  DC_HIP(hipMemsetAsync(D->remap, 0xff, (size_t)nV * sizeof(int), st));
  DC_LAUNCH(k_dc_vk, K, 256, K, D->cs, D->ekey, D->vk);
  DC_LAUNCH(k_dc_rk, nV, 256 / DC_G, nV, D->vk, D->nstart, D->nbs, D->rk);
  DC_LAUNCH(k_dc_select, K, 256, K, D->cs, D->ekey, D->ecnt, D->rk, D->selc, D->cnt);
  if (dc_scan(D, D->selc, D->pre, (size_t)K)) return -1;
  DC_LAUNCH(k_dc_apply_v, K, 256, K, D->cs, D->selc, D->pre, R, D->ekey, D->vbar, D->P, D->Q, nV, D->remap, D->cnt);
  DC_LAUNCH(k_dc_apply_f, nL, 256, nL, D->live, D->remap, D->F, D->valid);
  DC_HIP(hipGetLastError());
  if (dc_read_cnt(D, h)) return -1;
  D->nvalid -= h[DC_NREMOVED];
  D->topo_fresh = false; D->live_fresh = false;
  rec[4] = h[DC_NSEL]; rec[5] = h[DC_NAPPLIED]; rec[6] = h[DC_NREMOVED]; rec[7] = D->nvalid;
  ++D->rounds;
  if (dc_count_used(D)) return -1;
  return 1;
}

extern "C" int pa_decimate_run(pa_ctx* ctx, pa_decimate* D, int64_t face_target, int max_rounds) {
  int n = 0;
  while (n < max_rounds) {  // the host loop: a hard cap, and every round ends with a read-back
    const int rc = pa_decimate_round(ctx, D, face_target);
    if (rc < 0) return -1;
    if (rc == 0) break;
    ++n;
  }
  return n;
}

extern "C" int pa_decimate_last_round(const pa_decimate* D, int64_t rec[8]) {
  if (!D || !rec) return 1;
  for (int i = 0; i < 8; ++i) rec[i] = D->rec[i];
  return 0;
}

extern "C" int pa_decimate_counts(const pa_decimate* D, int64_t* nverts, int64_t* nfaces, int64_t* rounds) {
  if (!D) return 1;
  if (nverts) *nverts = D->nused;
  if (nfaces) *nfaces = D->nvalid;
  if (rounds) *rounds = D->rounds;
  return 0;
}

extern "C" int pa_decimate_read(pa_ctx* ctx, const pa_decimate* Dc, double* xyz, int32_t* elts) {
  PaBind bind_(ctx);
  pa_decimate* D = const_cast<pa_decimate*>(Dc);  // the scratch arrays are rewritten, the surface is not
  if (!ctx || !D || D->ctx != ctx) return pa_fail(ctx, "pa_decimate_read: null argument, or the object belongs to another context");
  if ((D->nused > 0 && !xyz) || (D->nvalid > 0 && !elts)) return pa_fail(ctx, "pa_decimate_read: null output");
  hipStream_t st = ctx->stream;
  if (dc_count_used(D)) return 1;  // leaves the flags in iscr2 and the new ids in iscr
  double* dx = nullptr;
  int32_t* de = nullptr;
  PA_HIP(hipMalloc(&dx, std::max<size_t>(3 * (size_t)D->nused, 1) * sizeof(double)));
  if (hipMalloc(&de, std::max<size_t>(3 * (size_t)D->nvalid, 1) * sizeof(int32_t)) != hipSuccess) { (void)hipFree(dx); return pa_fail(ctx, "pa_decimate_read: out of memory"); }
  DC_LAUNCH(k_dc_out_xyz, D->nV, 256, D->nV, D->iscr2, D->iscr, D->P, dx);
  DC_LAUNCH(k_dc_out_elts, D->nL, 256, D->nL, D->live, D->F, D->iscr, de);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && D->nused > 0) e = hipMemcpyAsync(xyz, dx, 3 * (size_t)D->nused * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && D->nvalid > 0) e = hipMemcpyAsync(elts, de, 3 * (size_t)D->nvalid * sizeof(int32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(dx); (void)hipFree(de);
  if (e != hipSuccess) return pa_fail(ctx, std::string("pa_decimate_read: ") + hipGetErrorString(e));
  return 0;
}

extern "C" int pa_decimate_read_state(pa_ctx* ctx, const pa_decimate* D, double* xyz_all, int32_t* faces_all, uint8_t* face_valid, double* quadrics) {
  PaBind bind_(ctx);
  if (!ctx || !D || D->ctx != ctx) return pa_fail(ctx, "pa_decimate_read_state: null argument, or the object belongs to another context");
  hipStream_t st = ctx->stream;
  const size_t nV = (size_t)D->nV, nF = (size_t)D->nF;
  if (xyz_all && nV) PA_HIP(hipMemcpyAsync(xyz_all, D->P, 3 * nV * sizeof(double), hipMemcpyDeviceToHost, st));
  if (quadrics && nV) PA_HIP(hipMemcpyAsync(quadrics, D->Q, 10 * nV * sizeof(double), hipMemcpyDeviceToHost, st));
  if (faces_all && nF) PA_HIP(hipMemcpyAsync(faces_all, D->F, 3 * nF * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (face_valid && nF) {
    unsigned char* vb = (unsigned char*)D->iscr2;  // nF bytes of an int array of at least nF entries
    DC_LAUNCH(k_dc_valid_bytes, D->nF, 256, D->nF, D->valid, vb);
    PA_HIP(hipGetLastError());
    PA_HIP(hipMemcpyAsync(face_valid, vb, nF, hipMemcpyDeviceToHost, st));
  }
  PA_HIP(hipStreamSynchronize(st));
  return 0;
}
