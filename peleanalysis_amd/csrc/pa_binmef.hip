// pa_binmef.hip -- the area-weighted (joint) PDF of node fields over a triangulated surface (binMEF.cpp): every triangle is clipped
// against the bin edges of each binned component and the pieces (leaves) add their area to the bin they lie in.
//
// SPLITTING: the reference recurses (processTriangle, :231-331).  Here a WORK ITEM is a triangle with the bin vector of
// each vertex and binID, the component being clipped.  A lane follows ONE path of the recursion in a loop of bounded length: the area
// test, binID + 1 while the three vertices share the bin, the leaf, or a split -- it keeps the remainder that stays at binID (its
// top bin is one lower, so the loop ends after at most nBins + 2 splits per component) and APPENDS the at most two other children to
// the next list.  Rounds are separated by kernel boundaries; no kernel waits for another workgroup.  Every round is count -> scan ->
// emit (the pattern of pa_mc.hip): k_sb_count walks the paths and counts the children of every item, the host scans the counts --
// it needs the totals anyway to choose how much of the list fits -- and k_sb_emit walks the same paths again, writes the children at
// their exact places and adds the leaves.  The list is a stack of `cap` items worked off depth first: a round pops a top slice and pushes its
// children, keeping room for what the items left on top may still need (pa_binmef_slice), so device memory is bounded by cap, not
// by the input (a top triangle over s bins yields O(s^2) leaves).
//
// NUMERICS: the leaves are the reference's, operation for operation (contraction is off); their order is not, and need not be: the
// sums are the 192-bit fixed-point integers of pa_fixed192.h, scaled from the largest element area and rounded once at read.
// Lanes of a wavefront that hold the same key are summed in integers first and one lane adds (an isosurface of a binned field lands
// in ONE bin: one add per wavefront); `uncombined` is one set of global atomics per leaf, with identical bits.
#include "pa_internal.h"
#include "pa_fixed192.h"
#include <algorithm>
#include <cmath>
#include <cstring>

#define SB_MAXC 4                 // binned components
#define SB_NV (3 + SB_MAXC + 1)   // x y z, the binned components, the condition component
#define SB_MAXBINS (1LL << 24)
#define SB_DEFAULT_ITEMS (1LL << 19)
enum { PA_SB_BADFRAC = 8, PA_SB_LISTOVER = 16, PA_SB_ITER = 32 };

struct SbVert {
  double v[SB_NV];
  int bin[SB_MAXC];
};
struct SbItem {  // 248 bytes
  SbVert p[3];
  int binID;  // -1: a skipped element
  int pad;
};

struct SbArgs {
  int nc, cond_apply, cond_sgn, maxiter, uncombined, s_area;
  double cond_val, area_eps;
  int nb[SB_MAXC], eoff[SB_MAXC];
  double bmax[SB_MAXC];
  const double* edges;  // the lower edges of every component, one after the other
  long long ntab;       // the product of nb; entry ntab: outside the condition, ntab + 1: the elements
  u64* tab;             // [ntab + 2][4]: 3 limbs of area, hits
  int* flags;
  u64* nonfinite;
};

struct SbRounds {  // what sb_rounds counts
  long long rounds = 0, peak = 0, sliced = 0, items = 0, elements = 0;
  long long stuck_n = 0, stuck_children = 0;  // return 2: the list and the children of its top item
};

struct pa_surfbin {
  pa_ctx* ctx = nullptr;
  int nc = 0;
  int nb[SB_MAXC] = {};
  int eoff[SB_MAXC] = {};
  double bmin[SB_MAXC] = {}, bmax[SB_MAXC] = {};
  long long ntab = 0, cap = 0;
  bool begun = false;
  int s_area = 0;
  double area_max = 0.0;
  std::vector<double> h_edges;
  double* d_edges = nullptr;
  u64* d_tab = nullptr;
  int* d_flags = nullptr;
  u64* d_nonfinite = nullptr;
  SbItem* d_list[2] = {nullptr, nullptr};
  int* d_cnt = nullptr;
  long long* d_off = nullptr;
  // the upload of a surface: kept from call to call, grown when a surface needs more
  std::vector<double> h_nodes;
  double* d_nodes = nullptr;
  int* d_elts = nullptr;
  size_t nodes_cap = 0, elts_cap = 0;
  SbRounds st;
};

// binMEF.cpp:477-489: binLO[i] = binMin + i * dBin
std::vector<double> pa_binmef_edges(double bmin, double bmax, int n) {
  std::vector<double> e((size_t)n);
  const double d = (bmax - bmin) / n;
  for (int i = 0; i < n; ++i) e[(size_t)i] = bmin + i * d;
  return e;
}

// :46-60; pow(x, 2) is x * x
__host__ __device__ __forceinline__ double sb_area(const double* p0, const double* p1, const double* p2) {
  const double a = (p1[1] - p0[1]) * (p2[2] - p0[2]) - (p1[2] - p0[2]) * (p2[1] - p0[1]);
  const double b = (p1[2] - p0[2]) * (p2[0] - p0[0]) - (p1[0] - p0[0]) * (p2[2] - p0[2]);
  const double c = (p1[0] - p0[0]) * (p2[1] - p0[1]) - (p1[1] - p0[1]) * (p2[0] - p0[0]);
  return 0.5 * sqrt(a * a + b * b + c * c);
}

// the members of a vertex by a run-time index, without an indexed private array
__host__ __device__ __forceinline__ int sb_bin(const SbVert& V, int k) {
  int r = V.bin[0];
#pragma unroll
  for (int j = 1; j < SB_MAXC; ++j) r = k == j ? V.bin[j] : r;
  return r;
}
__host__ __device__ __forceinline__ void sb_setbin(SbVert& V, int k, int b) {
#pragma unroll
  for (int j = 0; j < SB_MAXC; ++j) V.bin[j] = k == j ? b : V.bin[j];
}
__host__ __device__ __forceinline__ double sb_val(const SbVert& V, int c) {
  double r = V.v[0];
#pragma unroll
  for (int j = 1; j < SB_NV; ++j) r = c == j ? V.v[j] : r;
  return r;
}
__host__ __device__ __forceinline__ void sb_swap(SbVert& a, SbVert& b) {
  const SbVert t = a;
  a = b;
  b = t;
}

// getBin (:168-200): -1 below the first edge, nBins above binMax, else upper_bound - 1 (a value == binMax is in the last bin)
__host__ __device__ __forceinline__ void sb_getbin(const SbArgs& P, SbVert& V) {
#pragma unroll
  for (int j = 0; j < SB_MAXC; ++j) {
    if (j >= P.nc) { V.bin[j] = 0; continue; }
    const double v = V.v[3 + j];
    const double* lo = P.edges + P.eoff[j];
    int r;
    if (v < lo[0]) r = -1;
    else if (v > P.bmax[j]) r = P.nb[j];
    else {
      int a = 0, b = P.nb[j];  // the first edge > v in [a, b)
      while (a < b) {
        const int m = (a + b) >> 1;
        if (lo[m] > v) b = m; else a = m + 1;
      }
      r = a - 1;
    }
    V.bin[j] = r;
  }
}

template <bool EMIT>
__host__ __device__ __forceinline__ void sb_child(SbItem* out, long long base, long long cap, int n, const SbVert& a, const SbVert& b, const SbVert& c, int k, int& flag) {
  if (!EMIT) return;
  const long long pos = base + n;
  if (pos >= cap) { flag |= PA_SB_LISTOVER; return; }  // cannot happen: the count pass walked the same path
  SbItem it;
  it.p[0] = a; it.p[1] = b; it.p[2] = c;
  it.binID = k;
  it.pad = 0;
  out[pos] = it;
}

// One path of processTriangle (:231-331) from the work item (A, B, C, k).  Returns the number of children appended to the next
// list (EMIT: written at out[base ..]); the leaf at the end of the path, if there is one, comes back in (key, area): key = the flat
// bin, P.ntab = outside the condition, -1 = none.
template <bool EMIT>
__host__ __device__ int sb_chain(const SbArgs& P, SbVert A, SbVert B, SbVert C, int k, SbItem* out, long long base, long long cap, int& flag, long long& key, double& leaf) {
  int nchild = 0;
  key = -1;
  leaf = 0.0;
  if (k < 0) return 0;
  for (int it = 0;; ++it) {
    if (it >= P.maxiter) { flag |= PA_SB_ITER; break; }
    const double area = sb_area(A.v, B.v, C.v);
    if (area < P.area_eps) break;  // :244, at every call
    if (k >= P.nc) {                // :248-269
      bool in = true;
      long long f = 0;
#pragma unroll
      for (int j = 0; j < SB_MAXC; ++j) {
        if (j >= P.nc) continue;
        in = in && A.bin[j] >= 0 && A.bin[j] < P.nb[j];
        f = f * P.nb[j] + A.bin[j];
      }
      if (in) {
        bool ok = true;
        if (P.cond_apply) {  // :206-226
          const double a = A.v[SB_NV - 1], b = B.v[SB_NV - 1], c = C.v[SB_NV - 1], cv = P.cond_val;
          ok = P.cond_sgn > 0 ? (a > cv && b > cv && c > cv) : (P.cond_sgn < 0 ? (a < cv && b < cv && c < cv) : (a == cv && b == cv && c == cv));
        }
        key = ok ? f : P.ntab;
        leaf = area;
      }
      break;
    }
    {
      const int a = sb_bin(A, k), b = sb_bin(B, k), c = sb_bin(C, k);
      if (a == b && b == c) {  // :270-274; a leaf under an index out of range adds nothing: dropped here
        if (a < 0 || a >= P.nb[k]) break;
        ++k;
        continue;
      }
    }
    // orderNodes (:63-90): big to small on the bin index
    if (sb_bin(B, k) > sb_bin(A, k)) sb_swap(A, B);
    if (sb_bin(C, k) > sb_bin(B, k)) sb_swap(B, C);
    if (sb_bin(B, k) > sb_bin(A, k)) sb_swap(A, B);
    const int ab = sb_bin(A, k);
    const double* lo = P.edges + P.eoff[k];
    const int nbk = P.nb[k];
    const double bmx = P.bmax[k];
    const double Av = sb_val(A, 3 + k), Bv = sb_val(B, 3 + k), Cv = sb_val(C, 3 + k);
    const bool keep = ab >= 0 && ab < nbk;  // the children that stay in A's bin of this component
    if (ab == sb_bin(B, k)) {               // :284-306
      double fAC, fBC;                      // findDE (:93-129)
      if (ab < 0) { fAC = (lo[0] - Av) / (Cv - Av); fBC = (lo[0] - Bv) / (Cv - Bv); }
      else if (ab >= nbk) { fAC = (Av - bmx) / (Av - Cv); fBC = (Bv - bmx) / (Bv - Cv); }
      else { fAC = (Av - lo[ab]) / (Av - Cv); fBC = (Bv - lo[ab]) / (Bv - Cv); }
      if (!(fAC >= 0 && fAC <= 1 && fBC >= 0 && fBC <= 1)) { flag |= PA_SB_BADFRAC; break; }  // :121
      SbVert D, E;
#pragma unroll
      for (int i = 0; i < SB_NV; ++i) {
        D.v[i] = A.v[i] - fAC * (A.v[i] - C.v[i]);
        E.v[i] = B.v[i] - fBC * (B.v[i] - C.v[i]);
      }
      sb_getbin(P, D);
      sb_getbin(P, E);
#pragma unroll
      for (int i = 0; i < SB_MAXC; ++i)  // :291-295
        if (i <= k) { D.bin[i] = A.bin[i]; E.bin[i] = D.bin[i]; }
      if (keep) {
        sb_child<EMIT>(out, base, cap, nchild, A, B, E, k + 1, flag);
        sb_child<EMIT>(out, base, cap, nchild + 1, A, E, D, k + 1, flag);
        nchild += 2;
      }
      sb_setbin(D, k, ab - 1);  // :302-303
      sb_setbin(E, k, ab - 1);
      A = D;  // (D, C, E) stays at binID
      B = C;
      C = E;
    } else {  // :307-329
      double fAB, fAC;  // findFG (:132-165)
      if (ab < 0) { fAB = (lo[0] - Av) / (Av - Bv); fAC = (lo[0] - Cv) / (Av - Cv); }
      else if (ab >= nbk) { fAB = (Av - bmx) / (Av - Bv); fAC = (Av - bmx) / (Av - Cv); }
      else { fAB = (Av - lo[ab]) / (Av - Bv); fAC = (Av - lo[ab]) / (Av - Cv); }
      if (!(fAB >= 0 && fAB <= 1 && fAC >= 0 && fAC <= 1)) { flag |= PA_SB_BADFRAC; break; }  // :159
      SbVert F, G;
#pragma unroll
      for (int i = 0; i < SB_NV; ++i) {
        F.v[i] = A.v[i] - fAB * (A.v[i] - B.v[i]);
        G.v[i] = A.v[i] - fAC * (A.v[i] - C.v[i]);
      }
      sb_getbin(P, F);
      sb_getbin(P, G);
#pragma unroll
      for (int i = 0; i < SB_MAXC; ++i)  // :314-318
        if (i <= k) { F.bin[i] = A.bin[i]; G.bin[i] = F.bin[i]; }
      if (keep) {
        sb_child<EMIT>(out, base, cap, nchild, A, F, G, k + 1, flag);
        nchild += 1;
      }
      sb_setbin(F, k, ab - 1);  // :323-324
      sb_setbin(G, k, ab - 1);
      sb_child<EMIT>(out, base, cap, nchild, F, C, G, k, flag);  // :327
      nchild += 1;
      A = F;  // (F, B, C) stays at binID (:325)
    }
  }
  return nchild;
}

// the leaves (or element areas) of a wavefront into the table.  Every lane of the wavefront calls this; key < 0: nothing to add.
__device__ __forceinline__ void sb_accumulate(const SbArgs& P, long long key, double area, int& flag) {
  const U192 zero = {{0, 0, 0}};
  const U192 fx = key >= 0 ? to_fixed(area, P.s_area, flag) : zero;
  if (P.uncombined) {
    if (key >= 0) {
      if (!u192_zero(fx)) u192_atomic_add(P.tab + key * 4, fx);
      atomicAdd(P.tab + key * 4 + 3, 1ull);
    }
    return;
  }
  u64 pending = __ballot(key >= 0);
  const int lane = (int)(threadIdx.x & 63);
  while (pending) {  // one turn per distinct key of the wavefront
    const int first = __ffsll((long long)pending) - 1;
    const long long k0 = __shfl(key, first);
    const bool mine = key == k0;
    const u64 m = __ballot(mine);
    const U192 v = wave_sum_u192(mine ? fx : zero);
    if (lane == first) {
      if (!u192_zero(v)) u192_atomic_add(P.tab + k0 * 4, v);
      atomicAdd(P.tab + k0 * 4 + 3, (u64)__popcll(m));
    }
    pending &= ~m;
  }
}

// elements e0 .. e0 + n - 1 -> work items list[0 .. n - 1] (:522-538); the element areas are summed before the areaEps test (:535)
__global__ __launch_bounds__(256) void k_sb_init(SbArgs P, const double* __restrict__ nodes, long long nnodes, int nv, const int* __restrict__ elts, long long e0, long long n,
                                                  SbItem* __restrict__ list) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  long long key = -1;
  double area = 0.0;
  int flag = 0;
  if (t < n) {
    SbItem it;
    bool finite = true;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const long long node = (long long)elts[3 * (e0 + t) + q] - 1;  // validated on the host
#pragma unroll
      for (int c = 0; c < SB_NV; ++c) {
        // slots: x y z, the nc binned components, then (last slot) the condition component
        const int src = c < 3 + P.nc ? c : (c == SB_NV - 1 && P.cond_apply ? 3 + P.nc : -1);
        const double v = src >= 0 && src < nv ? nodes[(long long)src * nnodes + node] : 0.0;
        finite = finite && isfinite(v);
        it.p[q].v[c] = v;
      }
    }
    it.pad = 0;
    if (finite) {
#pragma unroll
      for (int q = 0; q < 3; ++q) sb_getbin(P, it.p[q]);
      it.binID = 0;
      area = sb_area(it.p[0].v, it.p[1].v, it.p[2].v);
      key = P.ntab + 1;
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int j = 0; j < SB_MAXC; ++j) it.p[q].bin[j] = 0;
      it.binID = -1;
      atomicAdd(P.nonfinite, 1ull);
    }
    list[t] = it;
  }
  sb_accumulate(P, key, area, flag);
  if (flag) atomicOr(P.flags, flag);
}

// r of a work item: a bound on the splits that are left on ANY path below it.  Component j >= binID is cut once per bin between
// its top and its bottom vertex (the sub-triangles of a triangle lie inside it and the fields are linear on it, so their spans are no
// wider), with 2 to spare for the ends out of range.  A path appends at most 2 children per split: children <= 2 r; a child that
// stays at binID has its top bin lowered by one, one that moves on has lost the component: r(child) <= r - 1.  That last step is
// exact arithmetic's: the + 2 is in the parent's r and in the child's alike, so an interpolated value of a LATER component that lands
// an ulp beyond an edge its triangle did not reach can leave a child with r(child) = r.  The bound then costs nothing but the
// promise below: a slice is only ever taken when its children fit (pa_binmef_slice) and sb_child checks every position.
__host__ __device__ __forceinline__ int sb_rem(const SbArgs& P, const SbItem& it) {
  if (it.binID < 0) return 0;
  int r = 0;
#pragma unroll
  for (int j = 0; j < SB_MAXC; ++j) {
    if (j >= P.nc || j < it.binID) continue;
    const int a = it.p[0].bin[j], b = it.p[1].bin[j], c = it.p[2].bin[j];
    const int hi = a > b ? (a > c ? a : c) : (b > c ? b : c), lo = a < b ? (a < c ? a : c) : (b < c ? b : c);
    r += hi - lo + 2;
  }
  return r;
}

__global__ __launch_bounds__(256) void k_sb_count(SbArgs P, const SbItem* __restrict__ in, long long n, int* __restrict__ cnt /* [n][2]: children, r */) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const SbItem it = in[t];
  int flag = 0;
  long long key;
  double leaf;
  cnt[2 * t] = sb_chain<false>(P, it.p[0], it.p[1], it.p[2], it.binID, nullptr, 0, 0, flag, key, leaf);
  cnt[2 * t + 1] = sb_rem(P, it);
  // the flags are raised by the emit pass, which walks the same path
}

// The slice of a round.  The list is a stack that is worked off depth first, a slice at a time; cr[i] = (children, r) of item i.
// An item with bound r grows the stack by at most B(r) = r * r while it and everything below it in the tree is worked off ONE item at
// a time (children <= 2 r and r(child) <= r - 1: B(r) >= B(r - 1) + 2 r - 1).  A stack is SAFE when (i + 1) + B(r_i) <= cap for
// every position i: popping the top item alone keeps it safe, so the top item can always be popped.  The slice is the top item, then
// every item below it as long as the stack stays safe with the children in place of the slice -- they inherit the largest r of the
// slice as their bound: i0 + tot + B(max r) <= cap.  Returns i0, the first item of the slice, and the number of children in *tot;
// n when not even the top item's children fit (the stack was not safe: cap is below what the input needs, or a child's r came
// out above r - 1 by the rounding case of sb_rem -- the caller fails with a message, nothing is written out of bounds).
long long pa_binmef_slice(const int* cr, long long n, long long cap, long long* tot) {
  *tot = 0;
  if (n <= 0) return n;
  long long t = cr[2 * (n - 1)], rmax = cr[2 * (n - 1) + 1], i0 = n - 1;
  if (i0 + t > cap) return n;
  while (i0 > 0) {
    const long long j = i0 - 1, t2 = t + cr[2 * j], r2 = std::max<long long>(rmax, cr[2 * j + 1]);
    if (j + t2 + r2 * r2 > cap) break;
    i0 = j; t = t2; rmax = r2;
  }
  *tot = t;
  return i0;
}

__global__ __launch_bounds__(256) void k_sb_emit(SbArgs P, const SbItem* __restrict__ in, long long n, const long long* __restrict__ off, SbItem* __restrict__ out,
                                                  long long out_n) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  long long key = -1;
  double leaf = 0.0;
  int flag = 0;
  if (t < n) {
    const SbItem it = in[t];
    (void)sb_chain<true>(P, it.p[0], it.p[1], it.p[2], it.binID, out, off[t], out_n, flag, key, leaf);
  }
  sb_accumulate(P, key, leaf, flag);
  if (flag) atomicOr(P.flags, flag);
}

// The rounds of one surface: the ONE loop behind pa_surfbin_add_surface (SbDeviceOps launches the kernels) and
// tools/bench/binmef_host.hip (its ops walk the items on the host).  Elements enter cap / 4 at a time -- room for the first rounds'
// fan-out without slicing -- and each batch is worked off before the next.  ops.init(e0, n, L): elements e0 .. e0 + n - 1 -> L[0 .. n);
// ops.count(L, from, n, cr): (children, r) of items from .. n - 1 -> cr[2 from .. 2 n) on the host; ops.emit(L, i0, m, off, T, tot):
// items i0 .. i0 + m - 1 add their leaves and write their children at T[off[t] ..], tot in all, which then replace the slice at
// L + i0 unless the whole list went (i0 == 0: the caller's two lists swap); all three return 0 when done, with L, T and off free
// to be reused.  Returns 0, 1 (an op failed) or 2 (the children of the top item do not fit: st.stuck_*).
template <class Ops>
int sb_rounds(Ops& ops, long long nelts, long long cap, SbItem* L, SbItem* T, SbRounds& st) {
  const long long chunk = std::max<long long>(1, cap / 4);
  std::vector<int> hcnt;  // (children, r) of every item of the stack
  std::vector<long long> hoff;
  for (long long e0 = 0; e0 < nelts; e0 += chunk) {
    long long n = std::min<long long>(chunk, nelts - e0), counted = 0;
    if (ops.init(e0, n, L)) return 1;
    st.elements += n;
    hcnt.assign((size_t)n * 2, 0);
    while (n > 0) {
      st.peak = std::max(st.peak, n);
      // count the children of the items that were pushed last (a slice without children pushes nothing)
      if (n > counted && ops.count(L, counted, n, hcnt.data())) return 1;
      long long tot = 0;
      const long long i0 = pa_binmef_slice(hcnt.data(), n, cap, &tot);
      if (i0 == n) {
        st.stuck_n = n;
        st.stuck_children = hcnt[(size_t)(2 * (n - 1))];
        return 2;
      }
      const long long m = n - i0;
      hoff.resize((size_t)m);
      long long run = 0;
      for (long long t = 0; t < m; ++t) { hoff[(size_t)t] = run; run += hcnt[(size_t)(2 * (i0 + t))]; }
      if (ops.emit(L, i0, m, hoff.data(), T, tot)) return 1;
      if (i0 == 0) std::swap(L, T);  // the whole list went: the children ARE the next list
      st.rounds += 1;
      st.items += m;
      if (i0 > 0) st.sliced += 1;
      n = i0 + tot;
      counted = i0;
      hcnt.resize((size_t)n * 2);
    }
  }
  return 0;
}

struct SbDeviceOps {
  pa_ctx* ctx;
  pa_surfbin* S;
  SbArgs P;
  long long nnodes;
  int nv;
  static dim3 blocks(long long n) { return dim3((unsigned)((n + 255) / 256)); }
  int init(long long e0, long long n, SbItem* L) {
    hipLaunchKernelGGL(k_sb_init, blocks(n), dim3(256), 0, ctx->stream, P, S->d_nodes, nnodes, nv, S->d_elts, e0, n, L);
    PA_HIP(hipGetLastError());
    return 0;
  }
  int count(const SbItem* L, long long from, long long n, int* cr) {
    hipLaunchKernelGGL(k_sb_count, blocks(n - from), dim3(256), 0, ctx->stream, P, L + from, n - from, S->d_cnt + 2 * from);
    PA_HIP(hipGetLastError());
    PA_HIP(hipMemcpyAsync(cr + 2 * from, S->d_cnt + 2 * from, (size_t)(n - from) * 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PA_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
  }
  int emit(SbItem* L, long long i0, long long m, const long long* off, SbItem* T, long long tot) {
    PA_HIP(hipMemcpyAsync(S->d_off, off, (size_t)m * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_sb_emit, blocks(m), dim3(256), 0, ctx->stream, P, L + i0, m, S->d_off, T, tot);
    PA_HIP(hipGetLastError());
    if (i0 > 0 && tot) PA_HIP(hipMemcpyAsync(L + i0, T, (size_t)tot * sizeof(SbItem), hipMemcpyDeviceToDevice, ctx->stream));
    PA_HIP(hipStreamSynchronize(ctx->stream));  // off is reused by the next round
    return 0;
  }
};

extern "C" void pa_surfbin_destroy(pa_surfbin* S) {
  if (!S) return;
  PaBind bind_(S->ctx);
  if (S->ctx && S->ctx->stream) (void)hipStreamSynchronize(S->ctx->stream);
  if (S->d_edges) (void)hipFree(S->d_edges);
  if (S->d_tab) (void)hipFree(S->d_tab);
  if (S->d_flags) (void)hipFree(S->d_flags);
  if (S->d_nonfinite) (void)hipFree(S->d_nonfinite);
  if (S->d_list[0]) (void)hipFree(S->d_list[0]);
  if (S->d_list[1]) (void)hipFree(S->d_list[1]);
  if (S->d_cnt) (void)hipFree(S->d_cnt);
  if (S->d_off) (void)hipFree(S->d_off);
  if (S->d_nodes) (void)hipFree(S->d_nodes);
  if (S->d_elts) (void)hipFree(S->d_elts);
  delete S;
}

// binMEF.cpp:417-458, :477-489: the binned components' ranges and the bin edges
extern "C" pa_surfbin* pa_surfbin_create(pa_ctx* ctx, int nc, const int32_t* nbins, const double* bin_min, const double* bin_max, int64_t work_items) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  if (!nbins || !bin_min || !bin_max) { pa_fail(ctx, "pa_surfbin_create: bad argument"); return nullptr; }
  if (nc < 1 || nc > SB_MAXC) { pa_fail(ctx, "pa_surfbin_create: 1 to " + std::to_string(SB_MAXC) + " binned components"); return nullptr; }
  if (work_items < 0) { pa_fail(ctx, "pa_surfbin_create: work_items must not be negative"); return nullptr; }
  long long nt = 1;
  for (int j = 0; j < nc; ++j) {
    if (nbins[j] < 1) { pa_fail(ctx, "pa_surfbin_create: nBins must be positive"); return nullptr; }
    if (!std::isfinite(bin_min[j]) || !std::isfinite(bin_max[j])) { pa_fail(ctx, "pa_surfbin_create: binMin or binMax is not finite"); return nullptr; }
    nt *= nbins[j];
    if (nt > SB_MAXBINS) { pa_fail(ctx, "pa_surfbin_create: more than 2^24 bins"); return nullptr; }
  }
  pa_surfbin* S = new pa_surfbin;
  S->ctx = ctx;
  S->nc = nc;
  S->ntab = nt;
  S->cap = work_items ? (long long)work_items : SB_DEFAULT_ITEMS;
  for (int j = 0; j < nc; ++j) {
    S->nb[j] = nbins[j];
    S->bmin[j] = bin_min[j];
    S->bmax[j] = bin_max[j];
    S->eoff[j] = (int)S->h_edges.size();
    const std::vector<double> e = pa_binmef_edges(bin_min[j], bin_max[j], nbins[j]);
    S->h_edges.insert(S->h_edges.end(), e.begin(), e.end());
  }
  const size_t tabw = (size_t)(nt + 2) * 4;
  bool ok = hipMalloc((void**)&S->d_edges, S->h_edges.size() * sizeof(double)) == hipSuccess;
  ok = ok && hipMalloc((void**)&S->d_tab, tabw * sizeof(u64)) == hipSuccess;
  ok = ok && hipMalloc((void**)&S->d_flags, sizeof(int)) == hipSuccess;
  ok = ok && hipMalloc((void**)&S->d_nonfinite, sizeof(u64)) == hipSuccess;
  ok = ok && hipMalloc((void**)&S->d_list[0], (size_t)S->cap * sizeof(SbItem)) == hipSuccess;
  ok = ok && hipMalloc((void**)&S->d_list[1], (size_t)S->cap * sizeof(SbItem)) == hipSuccess;
  ok = ok && hipMalloc((void**)&S->d_cnt, (size_t)S->cap * 2 * sizeof(int)) == hipSuccess;
  ok = ok && hipMalloc((void**)&S->d_off, (size_t)S->cap * sizeof(long long)) == hipSuccess;
  ok = ok && hipMemcpy(S->d_edges, S->h_edges.data(), S->h_edges.size() * sizeof(double), hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    pa_fail(ctx, "pa_surfbin_create: out of device memory");
    pa_surfbin_destroy(S);
    return nullptr;
  }
  return S;
}

extern "C" int pa_surfbin_begin(pa_ctx* ctx, pa_surfbin* S, double area_max) {
  PaBind bind_(ctx);
  if (!ctx || !S) return pa_fail(ctx, "pa_surfbin_begin: bad argument");
  if (!(area_max >= 0.0) || !std::isfinite(area_max)) return pa_fail(ctx, "pa_surfbin_begin: area_max must be finite and not negative");
  PA_HIP(hipStreamSynchronize(ctx->stream));
  S->area_max = area_max;
  S->s_area = scale_of(area_max);
  PA_HIP(hipMemsetAsync(S->d_tab, 0, (size_t)(S->ntab + 2) * 4 * sizeof(u64), ctx->stream));
  PA_HIP(hipMemsetAsync(S->d_flags, 0, sizeof(int), ctx->stream));
  PA_HIP(hipMemsetAsync(S->d_nonfinite, 0, sizeof(u64), ctx->stream));
  S->st = SbRounds();
  S->begun = true;
  return 0;
}

// the largest finite element area (the magnitude for pa_surfbin_begin); -1: an element names a node that does not exist
extern "C" double pa_surfbin_max_area(int64_t nnodes, const double* x, const double* y, const double* z, int64_t nelts, const int32_t* elts) {
  double mx = 0.0;
  if (!x || !y || !z || (nelts > 0 && !elts)) return -1.0;
  for (int64_t e = 0; e < nelts; ++e) {
    double p[3][3];
    for (int q = 0; q < 3; ++q) {
      const int64_t n = (int64_t)elts[3 * e + q] - 1;
      if (n < 0 || n >= nnodes) return -1.0;
      p[q][0] = x[n]; p[q][1] = y[n]; p[q][2] = z[n];
    }
    const double a = sb_area(p[0], p[1], p[2]);
    if (std::isfinite(a) && a > mx) mx = a;
  }
  return mx;
}

// the element loop of binMEF.cpp:522-540 with processTriangle (:231-331) for one surface
extern "C" int pa_surfbin_add_surface(pa_ctx* ctx, pa_surfbin* S, int64_t nnodes, const double* x, const double* y, const double* z, const double* const* comps,
                                      const double* cond, int64_t nelts, const int32_t* elts, int cond_apply, int cond_sgn, double cond_val, double area_eps,
                                      int uncombined) {
  PaBind bind_(ctx);
  if (!ctx || !S || !x || !y || !z || !comps || (nelts > 0 && !elts)) return pa_fail(ctx, "pa_surfbin_add_surface: bad argument");
  if (!S->begun) return pa_fail(ctx, "pa_surfbin_add_surface: pa_surfbin_begin has not been called");
  if (cond_apply && !cond) return pa_fail(ctx, "pa_surfbin_add_surface: condApply without the condition component");
  if (area_eps != area_eps || cond_val != cond_val) return pa_fail(ctx, "pa_surfbin_add_surface: areaEps or condVal is NaN");
  if (nnodes < 0 || nnodes >= (1LL << 31) || nelts < 0 || nelts >= (1LL << 31) / 3) return pa_fail(ctx, "pa_surfbin_add_surface: surface too large");
  for (int j = 0; j < S->nc; ++j)
    if (!comps[j]) return pa_fail(ctx, "pa_surfbin_add_surface: bad argument");
  if (nelts == 0) return 0;
  for (int64_t q = 0; q < 3 * nelts; ++q)
    if (elts[q] < 1 || elts[q] > nnodes) return pa_fail(ctx, "pa_surfbin_add_surface: an element names a node that does not exist");
  // only the components that matter, as structure-of-arrays
  const int nv = 3 + S->nc + (cond_apply ? 1 : 0);
  std::vector<double>& h = S->h_nodes;
  h.resize((size_t)nv * (size_t)nnodes);
  for (int c = 0; c < nv; ++c) {
    const double* src = c == 0 ? x : c == 1 ? y : c == 2 ? z : (c < 3 + S->nc ? comps[c - 3] : cond);
    std::memcpy(h.data() + (size_t)c * (size_t)nnodes, src, (size_t)nnodes * sizeof(double));
  }
  if (h.size() > S->nodes_cap || (size_t)nelts * 3 > S->elts_cap) PA_HIP(hipStreamSynchronize(ctx->stream));
  if (h.size() > S->nodes_cap) {
    if (S->d_nodes) (void)hipFree(S->d_nodes);
    S->d_nodes = nullptr;
    S->nodes_cap = 0;
    if (hipMalloc((void**)&S->d_nodes, h.size() * sizeof(double)) != hipSuccess) return pa_fail(ctx, "pa_surfbin_add_surface: out of device memory");
    S->nodes_cap = h.size();
  }
  if ((size_t)nelts * 3 > S->elts_cap) {
    if (S->d_elts) (void)hipFree(S->d_elts);
    S->d_elts = nullptr;
    S->elts_cap = 0;
    if (hipMalloc((void**)&S->d_elts, (size_t)nelts * 3 * sizeof(int)) != hipSuccess) return pa_fail(ctx, "pa_surfbin_add_surface: out of device memory");
    S->elts_cap = (size_t)nelts * 3;
  }
  struct Sync {  // the caller's arrays are read by the stream until then
    hipStream_t s;
    ~Sync() { (void)hipStreamSynchronize(s); }
  } sync_{ctx->stream};
  PA_HIP(hipMemcpyAsync(S->d_nodes, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  PA_HIP(hipMemcpyAsync(S->d_elts, elts, (size_t)nelts * 3 * sizeof(int), hipMemcpyHostToDevice, ctx->stream));

  SbArgs P;
  std::memset(&P, 0, sizeof P);
  P.nc = S->nc;
  P.cond_apply = cond_apply ? 1 : 0;
  P.cond_sgn = cond_sgn;
  P.cond_val = cond_val;
  P.area_eps = area_eps;
  P.uncombined = uncombined ? 1 : 0;
  P.s_area = S->s_area;
  P.maxiter = S->nc + 4;
  for (int j = 0; j < S->nc; ++j) {
    P.nb[j] = S->nb[j];
    P.eoff[j] = S->eoff[j];
    P.bmax[j] = S->bmax[j];
    P.maxiter += S->nb[j] + 3;  // per component: one split per bin between the top and the bottom vertex, both ends out of range included
  }
  P.edges = S->d_edges;
  P.ntab = S->ntab;
  P.tab = S->d_tab;
  P.flags = S->d_flags;
  P.nonfinite = S->d_nonfinite;

  SbDeviceOps ops{ctx, S, P, (long long)nnodes, nv};
  const int rc = sb_rounds(ops, (long long)nelts, S->cap, S->d_list[0], S->d_list[1], S->st);
  if (rc == 2) {
    long long rr = 0;
    for (int j = 0; j < S->nc; ++j) rr += S->nb[j] + 3;
    return pa_fail(ctx, "pa_surfbin_add_surface: work_items = " + std::to_string(S->cap) + " cannot hold the " + std::to_string(S->st.stuck_children) +
                            " children of the top work item on a list of " + std::to_string(S->st.stuck_n) + "; " + std::to_string((4 * rr * rr + 2) / 3) +
                            " suffices for these bins");
  }
  return rc;
}

// the bins (binMEF.cpp:594-670 prints them), the area sums of :535 and :265 and NmyTriangles (:257)
extern "C" int pa_surfbin_read(pa_ctx* ctx, const pa_surfbin* S, double* area, int64_t* hits, double* total_area, double* outside_area, int64_t* counters) {
  PaBind bind_(ctx);
  if (!ctx || !S || !area || !hits) return pa_fail(ctx, "pa_surfbin_read: bad argument");
  if (!S->begun) return pa_fail(ctx, "pa_surfbin_read: pa_surfbin_begin has not been called");
  int fl = 0;
  u64 nonfinite = 0;
  std::vector<u64> h((size_t)(S->ntab + 2) * 4);
  PA_HIP(hipMemcpyAsync(&fl, S->d_flags, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipMemcpyAsync(&nonfinite, S->d_nonfinite, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipMemcpyAsync(h.data(), S->d_tab, h.size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipStreamSynchronize(ctx->stream));
  if (fl & PA_SB_BADFRAC) return pa_fail(ctx, "pa_surfbin_read: Assertion `fAC>=0 && fAC<=1 && fBC>=0 && fBC<=1' failed (a split fraction outside [0, 1])");
  if (fl & (PA_SB_LISTOVER | PA_SB_ITER)) return pa_fail(ctx, "pa_surfbin_read: internal error: a path left its bounds");
  if (fl & (PA_ST_OVERFLOW | PA_ST_NONFINITE)) return pa_fail(ctx, "pa_surfbin_read: an area exceeds the magnitude declared at begin (accumulator overflow)");
  int64_t nmy = 0;
  for (long long k = 0; k <= S->ntab; ++k) {
    const u64* e = h.data() + (size_t)k * 4;
    if (k < S->ntab) {
      area[k] = from_fixed(e, S->s_area);
      hits[k] = (int64_t)e[3];
    } else if (outside_area) {
      *outside_area = from_fixed(e, S->s_area);
    }
    nmy += (int64_t)e[3];
  }
  if (total_area) *total_area = from_fixed(h.data() + (size_t)(S->ntab + 1) * 4, S->s_area);
  if (counters) {
    counters[0] = nmy;                   // NmyTriangles: the leaves in range, inside the condition or not
    counters[1] = (int64_t)nonfinite;    // skipped elements
    counters[2] = S->st.rounds;
    counters[3] = S->st.peak;               // the most work items the list held
    counters[4] = S->st.sliced;             // rounds that could take only a part of the list
    counters[5] = S->st.items;              // work items walked
    counters[6] = S->st.elements;
    counters[7] = S->cap;
  }
  return 0;
}
