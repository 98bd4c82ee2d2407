// pa_streamsel.hip -- selecting streamlines (PeleAnalysis Src/streamScatter.cpp and Src/stream2plt.cpp) on gfx950: the peak of a
// conditioning component along every line, scanned from the middle (streamScatter.cpp:129-143), the range test with the ordered
// gather of the chosen variables (:145-154), the dense array of the selected lines (stream2plt.cpp:504-547), the line filters
// (:556-651) and the signed arc length (:654-713).
// Layout: that of pa_tubestats.hip -- the Str FABs of all levels and boxes flat, box g holds ncomp components of ni * nj doubles at
// ncomp * off_g, component-major, i (line in box) fastest, then j.  A pa_ssel holds the tables: per box (ni, nj, jlo, off) and node
// id -> (box, i).  The dense array of stream2plt ("final") is [component][point][line], line fastest.
// NUMERICS: one thread owns one line from its first point to its last, so neighbouring threads read neighbouring addresses and no
// value crosses threads: there is no floating-point atomic, no reduction and no scan over doubles.  Every expression keeps the
// reference's association (-ffp-contract=off: val_lo + alpha * (val_hi - val_lo) is not fused), every running sum its order in j,
// and the comparisons are the reference's literal >, <, std::max(a, b) = (a < b) ? b : a and std::min(a, b) = (b < a) ? b : a, so
// NaN goes the way it goes in the serial code.  The results are the serial code's bits for every launch shape.  The only scan is
// over the integer keep flags: it compacts the kept nodes in node-id order.
#include "pa_internal.h"
#include "pa_streamsel.h"

#include <algorithm>

namespace {

#define SS_BLOCK 256

struct SsTab {
  const long long* box;
  const int* node;
  long long nNodes;
};

// where line i of box b lives in a buffer of ncomp components
struct SsLine {
  long long base;  // ncomp * off + i
  long long ni, np;
  int nj, jlo;
};
__device__ __forceinline__ SsLine ss_line_of(const long long* box, int b, int i, int ncomp) {
  const long long* B = box + 4 * (long long)b;
  SsLine L;
  L.ni = B[0];
  L.nj = (int)B[1];
  L.jlo = (int)B[2];
  L.np = B[0] * B[1];
  L.base = (long long)ncomp * B[3] + i;
  return L;
}
__device__ __forceinline__ SsLine ss_line(const SsTab& T, int id, int ncomp) { return ss_line_of(T.box, T.node[2 * (long long)id], T.node[2 * (long long)id + 1], ncomp); }
__device__ __forceinline__ long long ss_at(const SsLine& L, int c, int j) { return L.base + (long long)c * L.np + (long long)(j - L.jlo) * L.ni; }

// streamScatter.cpp:129-143: start in the middle of the box's own j range -- (int)(0.5 * (lo + hi)) truncates toward zero -- and
// scan lo .. hi ascending, replacing on strict >
__global__ __launch_bounds__(SS_BLOCK) void k_ssel_peak(SsTab T, const int* order, const double* data, int ncomp, int comp, int* jpeak, double* hival) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= T.nNodes) return;
  const int id = order[t];
  const SsLine V = ss_line(T, id, ncomp);
  const int lo = V.jlo, hi = V.jlo + V.nj - 1;
  int ptOnStr = (int)(0.5 * (lo + hi));
  double hiVal = data[ss_at(V, comp, ptOnStr)];
  for (int j = lo; j <= hi; ++j) {
    const double val = data[ss_at(V, comp, j)];
    if (val > hiVal) {
      hiVal = val;
      ptOnStr = j;
    }
  }
  jpeak[id] = ptOnStr;
  hival[id] = hiVal;
}

// :145: the range test of node `id`
__device__ __forceinline__ int ss_keep(const double* hival, long long id, long long n, double moreThan, double lessThan) {
  if (id >= n) return 0;
  const double h = hival[id];
  return ((h >= moreThan) && (h < lessThan)) ? 1 : 0;
}
// inclusive scan of one int per thread over the workgroup (SS_BLOCK threads); every thread calls it
__device__ __forceinline__ int ss_block_scan(int v, int* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < SS_BLOCK; off <<= 1) {
    const int t = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  return s[tid];
}
__global__ __launch_bounds__(SS_BLOCK) void k_ssel_count(long long n, const double* hival, double moreThan, double lessThan, int* bsum) {
  __shared__ int s[SS_BLOCK];
  const long long id = blockIdx.x * (long long)SS_BLOCK + threadIdx.x;
  const int inc = ss_block_scan(ss_keep(hival, id, n, moreThan, lessThan), s);
  if (threadIdx.x == SS_BLOCK - 1) bsum[blockIdx.x] = inc;
}
// exclusive scan of n counts by ONE workgroup (one count per SS_BLOCK nodes: a single pass up to 4 M nodes); out[n] = the total
#define SS_SCAN_PER 16
__global__ __launch_bounds__(1024) void k_ssel_scan(const int* cnt, long long* out, long long n) {
  __shared__ long long s[1024];
  __shared__ long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (long long base = 0; base < n; base += 1024 * SS_SCAN_PER) {
    const long long q0 = base + (long long)tid * SS_SCAN_PER;
    long long mine = 0;
    for (int k = 0; k < SS_SCAN_PER; ++k)
      if (q0 + k < n) mine += cnt[q0 + k];
    s[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const long long t = tid >= off ? s[tid - off] : 0;
      __syncthreads();
      s[tid] += t;
      __syncthreads();
    }
    long long run = carry + s[tid] - mine;
    for (int k = 0; k < SS_SCAN_PER; ++k)
      if (q0 + k < n) {
        out[q0 + k] = run;
        run += cnt[q0 + k];
      }
    __syncthreads();
    if (tid == 1023) carry += s[1023];
    __syncthreads();
  }
  if (tid == 0) out[n] = carry;
}
// :145-154: the kept nodes in node-id order; row = kept nodes before this one, columns col0 .. col0 + nv - 1 of a row of `stride`
#define PA_SSEL_MAXVARS 64
struct SsVars { int n; int comp[PA_SSEL_MAXVARS]; };
__global__ __launch_bounds__(SS_BLOCK) void k_ssel_scatter(SsTab T, const double* data, int ncomp, SsVars S, const int* jpeak, const double* hival, double moreThan,
                                                           double lessThan, const long long* boff, int stride, int col0, double* out, int* err) {
  __shared__ int s[SS_BLOCK];
  const long long id = blockIdx.x * (long long)SS_BLOCK + threadIdx.x;
  const int keep = ss_keep(hival, id, T.nNodes, moreThan, lessThan);
  const int inc = ss_block_scan(keep, s);
  if (!keep) return;
  const SsLine V = ss_line(T, (int)id, ncomp);
  const int j = jpeak[id];
  if (j < V.jlo || j > V.jlo + V.nj - 1) {  // not a j of pa_ssel_peaks: nothing is read or written for the node, the call fails
    *err = 1;
    return;
  }
  double* row = out + (boff[blockIdx.x] + (inc - 1)) * (long long)stride + col0;
  for (int v = 0; v < S.n; ++v) row[v] = data[ss_at(V, S.comp[v], j)];
}

// stream2plt.cpp:504-547: component comps[c] of line (box, i) of the selection -> final [c][j - slo][new index], one thread per line and
// component (the selection is in level -> box -> line order: neighbouring threads read neighbouring lines of one box)
__global__ __launch_bounds__(SS_BLOCK) void k_ssel_lines(const long long* box, const int* sel, long long nSel, const double* data, int ncomp, const int* comps, int npts,
                                                         double* final) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= nSel) return;
  const int c = blockIdx.y;
  const SsLine V = ss_line_of(box, sel[2 * i], sel[2 * i + 1], ncomp);
  const int src = comps[c];
  for (int j = 0; j < npts; ++j) final[((long long)c * npts + j) * nSel + i] = data[ss_at(V, src, V.jlo + j)];
}

// do_test (stream2plt.cpp:732-751); sgn: 0 ge, 1 gt, 2 lt, 3 le, 4 eq, 5 ne, anything else (an unknown string) tests false
__device__ __forceinline__ bool ss_test(double thisVal, int sgn, double critVal) {
  switch (sgn) {
    case 0: return thisVal >= critVal;
    case 1: return thisVal > critVal;
    case 2: return thisVal < critVal;
    case 3: return thisVal <= critVal;
    case 4: return thisVal == critVal;
    case 5: return thisVal != critVal;
    default: return false;
  }
}
// the first segment j with a strict bracket of loc_val (:634-640, :681-687); npts - 1 when there is none
__device__ __forceinline__ int ss_crossing(const double* F, long long nSel, long long i, int npts, int loc_comp, double loc_val, double& alpha) {
  for (int j = 0; j < npts - 1; ++j) {
    const double loc_val_lo = F[((long long)loc_comp * npts + j) * nSel + i], loc_val_hi = F[((long long)loc_comp * npts + j + 1) * nSel + i];
    if (((loc_val_lo > loc_val) && (loc_val_hi < loc_val)) || ((loc_val_lo < loc_val) && (loc_val_hi > loc_val))) {
      alpha = (loc_val - loc_val_lo) / (loc_val_hi - loc_val_lo);
      return j;
    }
  }
  return npts - 1;
}
// :556-651, one thread per line walking the table of conditions in the reference's order.  The running max / min of EVERY line starts
// from the first point of line 0 (:574, :591); an at-test that finds a crossing ASSIGNS the flag (:646)
__global__ __launch_bounds__(SS_BLOCK) void k_ssel_filter(const double* F, int npts, long long nSel, int ncond, const pa_ssel_cond* conds, int jmid, int* write_lines) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= nSel) return;
  int w = 1;
  for (int n = 0; n < ncond; ++n) {
    const pa_ssel_cond q = conds[n];
    if (q.kind == PA_SSEL_MAX || q.kind == PA_SSEL_MIN) {
      const double* p = F + (long long)q.comp * npts * nSel;
      double m = p[0];  // fab(se, nc): line 0
      if (q.kind == PA_SSEL_MAX) {
        for (int j = 0; j < npts; ++j) {
          const double x = p[(long long)j * nSel + i];
          m = (x < m) ? m : x;  // std::max(x, m)
        }
      } else {
        for (int j = 0; j < npts; ++j) {
          const double x = p[(long long)j * nSel + i];
          m = (m < x) ? m : x;  // std::min(x, m)
        }
      }
      if (!ss_test(m, q.sgn, q.val)) w = 0;
    } else if (q.kind == PA_SSEL_RXY) {
      double radius = 0;
      for (int c = 0; c < 2; ++c) {
        const double val = F[((long long)c * npts + jmid) * nSel + i];
        radius += val * val;
      }
      radius = sqrt(radius);
      if (!ss_test(radius, q.sgn, q.val)) w = 0;
    } else {  // PA_SSEL_AT: where comp crosses val2, comp2 there against val
      double alpha = 0;
      const int j = ss_crossing(F, nSel, i, npts, q.comp, q.val2, alpha);
      if (j < npts - 1) {
        const double val_lo = F[((long long)q.comp2 * npts + j) * nSel + i], val_hi = F[((long long)q.comp2 * npts + j + 1) * nSel + i];
        const double val_test = val_lo + alpha * (val_hi - val_lo);
        w = ss_test(val_test, q.sgn, q.val) ? 1 : 0;
      }
    }
  }
  write_lines[i] = w;
}

// :654-713: component nDist = the serial running sum of the segment lengths, shifted by its value where distComp crosses distVal, or
// 2 * the line's length everywhere when it does not.  The thread reads back its own stores only.
__global__ __launch_bounds__(SS_BLOCK) void k_ssel_arc(double* F, int nDist, int npts, long long nSel, int distComp, double distVal) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= nSel) return;
  double* D = F + (long long)nDist * npts * nSel + i;
  double lo[3], run = 0;
  for (int n = 0; n < 3; ++n) lo[n] = F[((long long)n * npts) * nSel + i];
  D[0] = 0;
  for (int j = 1; j < npts; ++j) {
    double ds = 0;
    for (int n = 0; n < 3; ++n) {
      const double hi = F[((long long)n * npts + j) * nSel + i];
      const double dx = hi - lo[n];
      ds += dx * dx;
      lo[n] = hi;
    }
    ds = sqrt(ds);
    run = run + ds;
    D[(long long)j * nSel] = run;
  }
  double alpha = 0;
  const int j = ss_crossing(F, nSel, i, npts, distComp, distVal, alpha);
  if (j < npts - 1) {
    const double val_lo = D[(long long)j * nSel], val_hi = D[(long long)(j + 1) * nSel];
    const double loc_offset = val_lo + alpha * (val_hi - val_lo);
    for (int jj = 0; jj < npts; ++jj) D[(long long)jj * nSel] = D[(long long)jj * nSel] - loc_offset;
  } else {
    const double err_val = D[(long long)(npts - 1) * nSel] * 2;
    for (int jj = 0; jj < npts; ++jj) D[(long long)jj * nSel] = err_val;
  }
}

inline dim3 ss_grid(long long n) { return dim3((unsigned)((n + SS_BLOCK - 1) / SS_BLOCK)); }
inline SsTab ss_tab(const pa_ssel* s) { return SsTab{s->d_box, s->d_node, s->nNodes}; }
bool ss_comp_ok(int ncomp, int comp) { return ncomp >= 1 && comp >= 0 && comp < ncomp; }

// a host table in device memory for the length of one call
struct SsTmp {
  void* p = nullptr;
  ~SsTmp() { if (p) (void)hipFree(p); }
  bool up(const void* h, size_t bytes) {
    if (hipMalloc(&p, std::max<size_t>(bytes, 8)) != hipSuccess) return false;
    return bytes == 0 || hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
  }
};

}  // namespace

extern "C" pa_ssel* pa_ssel_create(pa_ctx* ctx, int32_t nbt, const int64_t* box_desc, int64_t nNodes, const int32_t* node_table) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  auto fail = [&](const std::string& m) -> pa_ssel* { pa_fail(ctx, "pa_ssel_create: " + m); return nullptr; };
  if (nbt < 1 || !box_desc || nNodes < 0 || (nNodes > 0 && !node_table)) return fail("bad argument");
  if (nNodes >= (1LL << 31) - SS_BLOCK) return fail("more than 2^31 nodes");
  for (int g = 0; g < nbt; ++g) {
    const int64_t* B = box_desc + 4 * g;
    if (B[0] < 1 || B[1] < 1 || B[0] >= (1LL << 31) || B[1] >= (1LL << 31) || B[2] < -(1LL << 30) || B[2] + B[1] - 1 > (1LL << 30) || B[3] < 0) return fail("box " + std::to_string(g) + ": bad (ni, nj, jlo, offset)");
  }
  std::unique_ptr<pa_ssel> s(new pa_ssel);
  s->ctx = ctx;
  s->nbt = nbt;
  s->nNodes = nNodes;
  s->box.assign(box_desc, box_desc + 4 * (size_t)nbt);
  s->node.assign(node_table, node_table + 2 * (size_t)nNodes);
  for (long long n = 0; n < nNodes; ++n) {
    const int b = s->node[2 * (size_t)n], i = s->node[2 * (size_t)n + 1];
    if (b == -1) return fail("node id " + std::to_string(n + 1) + " is listed by no box");
    if (b < 0 || b >= nbt) return fail("node " + std::to_string(n + 1) + ": box " + std::to_string(b) + " out of range");
    if (i < 0 || i >= s->box[4 * (size_t)b]) return fail("node " + std::to_string(n + 1) + ": line " + std::to_string(i) + " outside its box");
  }
  std::vector<int> order((size_t)nNodes);
  for (long long n = 0; n < nNodes; ++n) order[(size_t)n] = (int)n;
  std::sort(order.begin(), order.end(), [&](int p, int q) {
    const int *a = &s->node[2 * (size_t)p], *b = &s->node[2 * (size_t)q];
    return a[0] != b[0] ? a[0] < b[0] : (a[1] != b[1] ? a[1] < b[1] : p < q);
  });
  const long long nblk = (nNodes + SS_BLOCK - 1) / SS_BLOCK;
  const size_t nb = sizeof(long long) * 4 * (size_t)nbt, nn = sizeof(int) * 2 * (size_t)std::max<long long>(nNodes, 1), no = sizeof(int) * (size_t)std::max<long long>(nNodes, 1);
  bool ok = hipMalloc(&s->d_box, nb) == hipSuccess && hipMalloc(&s->d_node, nn) == hipSuccess && hipMalloc(&s->d_order, no) == hipSuccess &&
            hipMalloc(&s->d_bsum, sizeof(int) * (size_t)std::max<long long>(nblk, 1)) == hipSuccess && hipMalloc(&s->d_boff, sizeof(long long) * (size_t)(nblk + 1)) == hipSuccess &&
            hipMalloc(&s->d_err, sizeof(int)) == hipSuccess;
  ok = ok && hipMemcpy(s->d_box, s->box.data(), nb, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && nNodes > 0)
    ok = hipMemcpy(s->d_node, s->node.data(), sizeof(int) * 2 * (size_t)nNodes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(s->d_order, order.data(), sizeof(int) * (size_t)nNodes, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    pa_ssel_destroy(s.release());
    return fail("device allocation or copy failed");
  }
  return s.release();
}

extern "C" void pa_ssel_destroy(pa_ssel* s) {
  if (!s) return;
  PaBind bind_(s->ctx);
  for (void* p : {(void*)s->d_box, (void*)s->d_node, (void*)s->d_order, (void*)s->d_bsum, (void*)s->d_boff, (void*)s->d_err, (void*)s->d_nline})
    if (p) (void)hipFree(p);
  delete s;
}

extern "C" int pa_ssel_peaks(pa_ctx* ctx, pa_ssel* s, const double* data, int32_t ncomp, int32_t comp, int32_t* jpeak, double* hival) {
  PaBind bind_(ctx);
  if (!ctx || !s) return pa_fail(ctx, "pa_ssel_peaks: bad argument");
  if (!ss_comp_ok(ncomp, comp)) return pa_fail(ctx, "pa_ssel_peaks: conditioning component " + std::to_string(comp) + " out of range (the buffer holds " + std::to_string(ncomp) + ")");
  if (s->nNodes == 0) return 0;
  if (!data || !jpeak || !hival) return pa_fail(ctx, "pa_ssel_peaks: null device array");
  hipLaunchKernelGGL(k_ssel_peak, ss_grid(s->nNodes), dim3(SS_BLOCK), 0, ctx->stream, ss_tab(s), s->d_order, data, (int)ncomp, (int)comp, jpeak, hival);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_ssel_peaks: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_ssel_scatter(pa_ctx* ctx, pa_ssel* s, const double* data, int32_t ncomp, int32_t nvars, const int32_t* comps, const int32_t* jpeak, const double* hival,
                               double moreThan, double lessThan, int32_t stride, int32_t col0, double* out, int64_t* nkept) {
  PaBind bind_(ctx);
  if (!ctx || !s || !nkept || nvars < 0 || nvars > PA_SSEL_MAXVARS || (nvars > 0 && !comps) || col0 < 0 || stride < col0 + nvars)
    return pa_fail(ctx, "pa_ssel_scatter: bad argument (more than 64 variables in one call, or columns outside the row)");
  SsVars S{};
  S.n = nvars;
  for (int v = 0; v < nvars; ++v) {
    if (!ss_comp_ok(ncomp, comps[v])) return pa_fail(ctx, "pa_ssel_scatter: component " + std::to_string(comps[v]) + " out of range (the buffer holds " + std::to_string(ncomp) + ")");
    S.comp[v] = comps[v];
  }
  *nkept = 0;
  if (s->nNodes == 0) return 0;
  if (!hival || (nvars > 0 && (!jpeak || !data || !out))) return pa_fail(ctx, "pa_ssel_scatter: null device array");
  const long long nblk = (s->nNodes + SS_BLOCK - 1) / SS_BLOCK;
  PA_HIP(hipMemsetAsync(s->d_err, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(k_ssel_count, ss_grid(s->nNodes), dim3(SS_BLOCK), 0, ctx->stream, s->nNodes, hival, moreThan, lessThan, s->d_bsum);
  hipLaunchKernelGGL(k_ssel_scan, dim3(1), dim3(1024), 0, ctx->stream, s->d_bsum, s->d_boff, nblk);
  if (nvars > 0)
    hipLaunchKernelGGL(k_ssel_scatter, ss_grid(s->nNodes), dim3(SS_BLOCK), 0, ctx->stream, ss_tab(s), data, (int)ncomp, S, jpeak, hival, moreThan, lessThan, s->d_boff,
                       (int)stride, (int)col0, out, s->d_err);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_ssel_scatter: launch failed");
  long long n = 0;
  int err = 0;
  PA_HIP(hipMemcpyAsync(&n, s->d_boff + nblk, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
  PA_HIP(hipMemcpyAsync(&err, s->d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream));
  if (pa_sync(ctx) != 0) return 1;
  if (err) return pa_fail(ctx, "pa_ssel_scatter: a peak index lies outside its line's j range (jpeak is not the output of pa_ssel_peaks on these tables)");
  *nkept = n;
  return 0;
}

extern "C" int pa_ssel_gather_lines(pa_ctx* ctx, pa_ssel* s, const double* data, int32_t ncomp, int32_t ncompSel, const int32_t* comps, int64_t nSel, const int32_t* sel,
                                    int32_t slo, int32_t shi, double* final) {
  PaBind bind_(ctx);
  if (!ctx || !s || ncompSel < 1 || ncompSel > 65535 || !comps || nSel < 0 || (nSel > 0 && !sel) || shi < slo) return pa_fail(ctx, "pa_ssel_gather_lines: bad argument");
  for (int c = 0; c < ncompSel; ++c)
    if (!ss_comp_ok(ncomp, comps[c])) return pa_fail(ctx, "pa_ssel_gather_lines: component " + std::to_string(comps[c]) + " out of range (the buffer holds " + std::to_string(ncomp) + ")");
  for (long long q = 0; q < nSel; ++q) {
    const int b = sel[2 * q], i = sel[2 * q + 1];
    if (b < 0 || b >= s->nbt) return pa_fail(ctx, "pa_ssel_gather_lines: selected line " + std::to_string(q) + ": box " + std::to_string(b) + " out of range");
    const long long* B = &s->box[4 * (size_t)b];
    if (i < 0 || i >= B[0]) return pa_fail(ctx, "pa_ssel_gather_lines: selected line " + std::to_string(q) + ": line " + std::to_string(i) + " outside its box");
    if (B[2] != slo || B[2] + B[1] - 1 != shi)
      return pa_fail(ctx, "pa_ssel_gather_lines: Str box " + std::to_string(b) + " (j = " + std::to_string(B[2]) + " .. " + std::to_string(B[2] + B[1] - 1) + ") does not span the directory's j = " +
                              std::to_string(slo) + " .. " + std::to_string(shi));
  }
  if (nSel == 0) return 0;
  if (!data || !final) return pa_fail(ctx, "pa_ssel_gather_lines: null device array");
  SsTmp dsel, dcomps;
  if (!dsel.up(sel, sizeof(int32_t) * 2 * (size_t)nSel) || !dcomps.up(comps, sizeof(int32_t) * (size_t)ncompSel)) return pa_fail(ctx, "pa_ssel_gather_lines: device allocation or copy failed");
  dim3 grid = ss_grid(nSel);
  grid.y = (unsigned)ncompSel;
  hipLaunchKernelGGL(k_ssel_lines, grid, dim3(SS_BLOCK), 0, ctx->stream, s->d_box, (const int*)dsel.p, (long long)nSel, data, (int)ncomp, (const int*)dcomps.p, (int)(shi - slo + 1), final);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_ssel_gather_lines: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_ssel_filter(pa_ctx* ctx, const double* final, int32_t ncompSel, int32_t slo, int32_t shi, int64_t nSel, int32_t ncond, const pa_ssel_cond* conds,
                              int32_t* write_lines) {
  PaBind bind_(ctx);
  if (!ctx || ncompSel < 1 || shi < slo || nSel < 0 || ncond < 0 || (ncond > 0 && !conds)) return pa_fail(ctx, "pa_ssel_filter: bad argument");
  for (int n = 0; n < ncond; ++n) {
    const pa_ssel_cond& q = conds[n];
    const std::string at = "pa_ssel_filter: condition " + std::to_string(n) + ": ";
    if (q.kind < PA_SSEL_MAX || q.kind > PA_SSEL_AT) return pa_fail(ctx, at + "unknown kind");
    if (n > 0 && q.kind < conds[n - 1].kind) return pa_fail(ctx, at + "out of order (max-tests, min-tests, RXY, at-tests)");
    if (q.kind == PA_SSEL_RXY) {
      if (ncompSel < 2) return pa_fail(ctx, at + "the radius needs selected components 0 and 1");
    } else if (!ss_comp_ok(ncompSel, q.comp) || (q.kind == PA_SSEL_AT && !ss_comp_ok(ncompSel, q.comp2))) {
      return pa_fail(ctx, at + "component out of range (" + std::to_string(ncompSel) + " are selected)");
    }
  }
  if (nSel == 0) return 0;
  if (!final || !write_lines) return pa_fail(ctx, "pa_ssel_filter: null device array");
  SsTmp dc;
  if (!dc.up(conds, sizeof(pa_ssel_cond) * (size_t)ncond)) return pa_fail(ctx, "pa_ssel_filter: device allocation or copy failed");
  const int jmid = (int)(0.5 * (slo + shi)) - slo;  // :608: IntVect(i, 0.5 * (slo + shi), 0) truncates
  if (jmid < 0 || jmid > shi - slo) return pa_fail(ctx, "pa_ssel_filter: the middle point lies outside slo .. shi");
  hipLaunchKernelGGL(k_ssel_filter, ss_grid(nSel), dim3(SS_BLOCK), 0, ctx->stream, final, (int)(shi - slo + 1), (long long)nSel, (int)ncond, (const pa_ssel_cond*)dc.p, jmid, write_lines);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_ssel_filter: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_ssel_arclength(pa_ctx* ctx, double* final, int32_t ncompSel, int32_t npts, int64_t nSel, int32_t distComp, double distVal) {
  PaBind bind_(ctx);
  if (!ctx || npts < 1 || nSel < 0) return pa_fail(ctx, "pa_ssel_arclength: bad argument");
  if (ncompSel < 3) return pa_fail(ctx, "pa_ssel_arclength: the arc length needs selected components 0, 1 and 2");
  if (!ss_comp_ok(ncompSel, distComp)) return pa_fail(ctx, "pa_ssel_arclength: distComp " + std::to_string(distComp) + " out of range (" + std::to_string(ncompSel) + " are selected)");
  if (nSel == 0) return 0;
  if (!final) return pa_fail(ctx, "pa_ssel_arclength: null device array");
  hipLaunchKernelGGL(k_ssel_arc, ss_grid(nSel), dim3(SS_BLOCK), 0, ctx->stream, final, (int)ncompSel, (int)npts, (long long)nSel, (int)distComp, distVal);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_ssel_arclength: launch failed");
  return pa_sync(ctx);
}
