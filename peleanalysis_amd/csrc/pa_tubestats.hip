// pa_tubestats.hip -- stream tubes (PeleAnalysis Src/streamTubeStats.cpp) on gfx950: the wedge integrals of every surface triangle
// (wedge_volume_int / tetVol / wedge_surf_area with the element loop of :650-699), the per-line statistics (max_grad :876-952,
// peak_val :955-1001), the node-to-element means (:703-753), the element neighbours (buildNodeNeighbors :196-235) and the
// area-weighted smoothing (smoothVals :274-298).
// Layout: the Str FABs of all levels and boxes are flat -- box g holds ncomp components of ni * nj doubles at ncomp * off_g,
// component-major, i (line in box) fastest, then j -- the layout pa_streamsample_run takes for xyz.  A pa_tube holds the tables:
// per box (ni, nj, jlo, off), node id -> (box, i), the 1-based connectivity and, once asked for, the CSR of element neighbours.
// NUMERICS: every expression keeps the reference's association (-ffp-contract=off) and every sum over j its order; a thread owns a
// triangle (or a line) from the first point to the last, so there is no floating-point atomic and no reduction across threads: the
// results are bit-identical to the serial code for every launch shape and every grouping of the integrated components.  The twelve
// tetVol values of a wedge depend on coordinates only: they are formed once per wedge and shared by the volume and by all the
// components of the sweep (the reference recomputes them per component -- the same operations on the same operands).
#include "pa_internal.h"

#include <algorithm>

struct pa_tube {
  pa_ctx* ctx = nullptr;
  int nbt = 0;
  long long nNodes = 0, nElts = 0;
  std::vector<long long> box;  // [nbt][4]: ni, nj, jlo, off (points of the boxes before)
  std::vector<int> node;       // [nNodes][2]: box, i
  std::vector<char> has;       // [nbt]: some node lives in the box
  long long* d_box = nullptr;
  int* d_node = nullptr;
  int* d_face = nullptr;
  int* d_order = nullptr;      // node ids sorted by (box, i): consecutive threads of the line kernels read consecutive i of one box
  long long* d_rowptr = nullptr;  // CSR of the element neighbours, built on first use
  int* d_cols = nullptr;
  long long nnz = -1;
};

namespace {

struct TbTab {
  const long long* box;
  const int* node;
  const int* face;
  long long nNodes, nElts;
};

// where the line of node `id` lives in a buffer of ncomp components
struct TbLine {
  long long base;  // ncomp * off + i
  long long ni, np;
  int nj, jlo;
};
__device__ __forceinline__ TbLine tb_line(const TbTab& T, int id, int ncomp) {
  const int b = T.node[2 * id], i = T.node[2 * id + 1];
  const long long* B = T.box + 4 * (long long)b;
  TbLine L;
  L.ni = B[0];
  L.nj = (int)B[1];
  L.jlo = (int)B[2];
  L.np = B[0] * B[1];
  L.base = (long long)ncomp * B[3] + i;
  return L;
}
// index of (component c, point j) of the line
__device__ __forceinline__ long long tb_at(const TbLine& L, int c, int j) { return L.base + (long long)c * L.np + (long long)(j - L.jlo) * L.ni; }

struct P3 { double x[3]; };

// tetVol (:850-873): |R1 . (R2 x R3)| with R1 = D - A, R2 = B - A, R3 = C - A -- six times the volume
__device__ __forceinline__ double tb_tet(const P3& A, const P3& B, const P3& C, const P3& D) {
  double R1[3], R2[3], R3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    R1[i] = D.x[i] - A.x[i];
    R2[i] = B.x[i] - A.x[i];
    R3[i] = C.x[i] - A.x[i];
  }
  const double R40 = R2[1] * R3[2] - R3[1] * R2[2];
  const double R41 = R2[2] * R3[0] - R3[2] * R2[0];
  const double R42 = R2[0] * R3[1] - R3[0] * R2[1];
  return fabs((R1[0] * R40 + R1[1] * R41) + R1[2] * R42);
}

// wedge_surf_area (:1174-1254), three nodes
__device__ __forceinline__ double tb_area(const P3& A, const P3& B, const P3& C) {
  double R1[3], R2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    R1[i] = B.x[i] - A.x[i];
    R2[i] = C.x[i] - A.x[i];
  }
  const double R30 = R1[1] * R2[2] - R2[1] * R1[2];
  const double R31 = R1[2] * R2[0] - R2[2] * R1[0];
  const double R32 = R1[0] * R2[1] - R2[0] * R1[1];
  return 0.5 * sqrt((R30 * R30 + R31 * R31) + R32 * R32);
}

struct TbWedgeArgs {
  TbTab T;
  const double* xyz;
  const double* data;
  int ncomp, c0;  // data holds ncomp components; this sweep integrates c0 .. c0 + KC - 1
  int jlo, npts;
  int geom;       // write vol / area / wa (wa from component 0: only the sweep with c0 == 0 adds to it)
  double *vol, *area, *wa, *raw, *per_area;
};

// One thread per triangle, marching along j (:650-699).  The corners and values of point j stay in registers, point j + 1 is gathered.
template <int KC>
__global__ __launch_bounds__(256) void k_tube_wedges(TbWedgeArgs a) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= a.T.nElts) return;
  TbLine X[3], V[3];
#pragma unroll
  for (int n = 0; n < 3; ++n) {
    const int id = a.T.face[3 * e + n] - 1;
    X[n] = tb_line(a.T, id, 3);
    V[n] = tb_line(a.T, id, a.ncomp);
  }
  auto point = [&](int n, int j) {
    P3 p;
#pragma unroll
    for (int d = 0; d < 3; ++d) p.x[d] = a.xyz[tb_at(X[n], d, j)];
    return p;
  };
  const double area0 = tb_area(point(0, 0), point(1, 0), point(2, 0));
  double vol = 0.0, wa = 0.0, acc[KC > 0 ? KC : 1];
#pragma unroll
  for (int k = 0; k < KC; ++k) acc[k] = 0.0;
  if (a.npts >= 2) {
    P3 A = point(0, a.jlo), B = point(1, a.jlo), C = point(2, a.jlo);
    double vA[KC > 0 ? KC : 1], vB[KC > 0 ? KC : 1], vC[KC > 0 ? KC : 1];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      vA[k] = a.data[tb_at(V[0], a.c0 + k, a.jlo)];
      vB[k] = a.data[tb_at(V[1], a.c0 + k, a.jlo)];
      vC[k] = a.data[tb_at(V[2], a.c0 + k, a.jlo)];
    }
    const bool want_wa = a.geom && KC > 0 && a.c0 == 0;
    double areaLo = want_wa ? tb_area(A, B, C) : 0.0;
    for (int j = 0; j < a.npts - 1; ++j) {
      const int jn = a.jlo + j + 1;
      const P3 D = point(0, jn), E = point(1, jn), F = point(2, jn);
      // six times the tet volumes (:1113-1132)
      const double EABC = tb_tet(A, B, C, E), ADEF = tb_tet(A, D, E, F), ACEF = tb_tet(C, E, F, A);
      if (a.geom) vol += (EABC + ADEF + ACEF) / 6.;
      if (KC > 0) {
        const double DABC = tb_tet(A, B, C, D), FABC = tb_tet(A, B, C, F), BDEF = tb_tet(B, D, E, F), CDEF = tb_tet(C, D, E, F);
        const double ACED = tb_tet(C, E, D, A), BCDF = tb_tet(B, C, D, F), BCDE = tb_tet(B, C, D, E), ABDF = tb_tet(B, D, F, A);
        const double ABEF = tb_tet(B, E, F, A);
        const double areaHi = want_wa ? tb_area(D, E, F) : 0.0;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
          const double vD = a.data[tb_at(V[0], a.c0 + k, jn)], vE = a.data[tb_at(V[1], a.c0 + k, jn)], vF = a.data[tb_at(V[2], a.c0 + k, jn)];
          const double a_ = vA[k], b_ = vB[k], c_ = vC[k];
          // 24 times the integral over each of the six ways to cut the wedge into three tets (:1142-1164)
          const double int_1 = ((vD + a_ + b_ + c_) * DABC + (b_ + vD + vE + vF) * BDEF) + (b_ + c_ + vD + vF) * BCDF;
          const double int_2 = ((vD + a_ + b_ + c_) * DABC + (c_ + vD + vE + vF) * CDEF) + (b_ + c_ + vD + vE) * BCDE;
          const double int_3 = ((vE + a_ + b_ + c_) * EABC + (a_ + vD + vE + vF) * ADEF) + (a_ + c_ + vE + vF) * ACEF;
          const double int_4 = ((vE + a_ + b_ + c_) * EABC + (c_ + vD + vE + vF) * CDEF) + (a_ + c_ + vE + vD) * ACED;
          const double int_5 = ((vF + a_ + b_ + c_) * FABC + (a_ + vD + vE + vF) * ADEF) + (a_ + b_ + vE + vF) * ABEF;
          const double int_6 = ((vF + a_ + b_ + c_) * FABC + (b_ + vD + vE + vF) * BDEF) + (a_ + b_ + vD + vF) * ABDF;
          const double thisVolInt = (int_1 + int_2 + int_3 + int_4 + int_5 + int_6) / 144.;
          acc[k] += thisVolInt;
          if (want_wa && k == 0) wa += thisVolInt * (0.5 * (areaLo + areaHi));
          vA[k] = vD;
          vB[k] = vE;
          vC[k] = vF;
        }
        areaLo = areaHi;
      }
      A = D;
      B = E;
      C = F;
    }
  }
  if (a.geom) {
    a.vol[e] = vol;
    a.area[e] = area0;
    a.wa[e] = wa;
  }
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    a.raw[(long long)(a.c0 + k) * a.T.nElts + e] = acc[k];
    a.per_area[(long long)(a.c0 + k) * a.T.nElts + e] = acc[k] / area0;
  }
}

// max_grad (:876-952), one thread per line, two passes along j: the longest segment, then the gradients across the segments longer
// than the threshold -- maxs itself (the reference's test: no segment passes it) or, use_eps, 1.e-4 * maxs
__global__ __launch_bounds__(256) void k_tube_grad(TbTab T, const int* order, const double* xyz, const double* data, int ncomp, int comp, int use_eps,
                                                   double* gradmax) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= T.nNodes) return;
  const int id = order[t];
  const TbLine X = tb_line(T, id, 3), V = tb_line(T, id, ncomp);
  const int j0 = X.jlo;
  double hiX[3], loX[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) hiX[d] = xyz[tb_at(X, d, j0)];
  double maxs = 0;
  for (int i = 1; i < X.nj; ++i) {
    double tot = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      loX[d] = hiX[d];
      hiX[d] = xyz[tb_at(X, d, j0 + i)];
      const double dx = hiX[d] - loX[d];
      tot += dx * dx;
    }
    const double L = sqrt(tot);
    maxs = (i == 1 ? L : (maxs < L ? L : maxs));  // std::max(maxs, L)
  }
  const double thr = use_eps ? 1.e-4 * maxs : maxs;
#pragma unroll
  for (int d = 0; d < 3; ++d) hiX[d] = xyz[tb_at(X, d, j0)];
  double hiVal = data[tb_at(V, comp, j0)], gradMax = 0.;
  for (int i = 1; i < X.nj; ++i) {
    const double loVal = hiVal;
    hiVal = data[tb_at(V, comp, j0 + i)];
    double tot = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      loX[d] = hiX[d];
      hiX[d] = xyz[tb_at(X, d, j0 + i)];
      const double dx = hiX[d] - loX[d];
      tot += dx * dx;
    }
    const double L = sqrt(tot);
    if (L > thr) {
      const double grad = fabs((hiVal - loVal) / L);
      if (grad >= gradMax) gradMax = grad;
    }
  }
  gradmax[id] = gradMax;
}

// peak_val (:955-1001): the first maximum of component pcomp along the line (strict >), the sampled components there, and whether it
// sits inside the line (not at the first or last point of the box's j range)
#define PA_TUBE_MAXSAMPLE 32
struct TbSample { int n; int comp[PA_TUBE_MAXSAMPLE]; };
__global__ __launch_bounds__(256) void k_tube_peak(TbTab T, const int* order, const double* data, int ncomp, int pcomp, TbSample S, double* samples, int* ok) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= T.nNodes) return;
  const int id = order[t];
  const TbLine V = tb_line(T, id, ncomp);
  int loc = V.jlo;
  double peakVal = data[tb_at(V, pcomp, loc)];
  for (int i = 1; i < V.nj; ++i) {
    const double newVal = data[tb_at(V, pcomp, V.jlo + i)];
    if (newVal > peakVal) {
      peakVal = newVal;
      loc = V.jlo + i;
    }
  }
  for (int s = 0; s < S.n; ++s) samples[(long long)s * T.nNodes + id] = data[tb_at(V, S.comp[s], loc)];
  ok[id] = (loc == V.jlo || loc == V.jlo + V.nj - 1) ? 0 : 1;
}

// node values -> element values (:703-753)
__global__ __launch_bounds__(256) void k_tube_means(TbTab T, int nv, const double* vals, double* out) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= T.nElts) return;
  const int n0 = T.face[3 * e] - 1, n1 = T.face[3 * e + 1] - 1, n2 = T.face[3 * e + 2] - 1;
  for (int v = 0; v < nv; ++v) {
    const double* p = vals + (long long)v * T.nNodes;
    out[(long long)v * T.nElts + e] = (p[n0] + p[n1] + p[n2]) / 3.;
  }
}
__global__ __launch_bounds__(256) void k_tube_all(TbTab T, const int* ok, double* out) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= T.nElts) return;
  out[e] = (ok[T.face[3 * e] - 1] && ok[T.face[3 * e + 1] - 1] && ok[T.face[3 * e + 2] - 1]) ? 1.0 : 0.0;
}
// the values at the surface (j = 0), summed from 0 in node order, / nodesPerElt (:703-713)
__global__ __launch_bounds__(256) void k_tube_avg(TbTab T, const double* data, int ncomp, int comp, double* out) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= T.nElts) return;
  double s = 0;
  for (int n = 0; n < 3; ++n) s += data[tb_at(tb_line(T, T.face[3 * e + n] - 1, ncomp), comp, 0)];
  out[e] = s / 3;
}

// ---- element neighbours: node -> elements (count, scan, fill), then per element the union of its nodes' lists without itself
__global__ __launch_bounds__(256) void k_tube_count_inc(TbTab T, int* cnt) {
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= 3 * T.nElts) return;
  atomicAdd(&cnt[T.face[q] - 1], 1);
}
// exclusive scan of n counts by ONE workgroup (the node and element counts of a surface: a few passes over a few MB); out[n] = the total
#define PA_TUBE_SCAN_PER 16
__global__ __launch_bounds__(1024) void k_tube_scan(const int* cnt, long long* out, long long n) {
  __shared__ long long s[1024];
  __shared__ long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (long long base = 0; base < n; base += 1024 * PA_TUBE_SCAN_PER) {
    const long long q0 = base + (long long)tid * PA_TUBE_SCAN_PER;
    long long mine = 0;
    for (int k = 0; k < PA_TUBE_SCAN_PER; ++k)
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
    for (int k = 0; k < PA_TUBE_SCAN_PER; ++k)
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
__global__ __launch_bounds__(256) void k_tube_fill_inc(TbTab T, const long long* start, int* cursor, int* lists) {
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= 3 * T.nElts) return;
  const int nd = T.face[q] - 1;
  lists[start[nd] + atomicAdd(&cursor[nd], 1)] = (int)(q / 3);  // the order inside a list varies from run to run; the rows below are sorted
}
// entry q of the concatenation of the three nodes' lists of element e; -1 past the end
struct TbCat {
  const int* p[3];
  int n[3];
  __device__ __forceinline__ int total() const { return n[0] + n[1] + n[2]; }
  __device__ __forceinline__ int at(int q) const { return q < n[0] ? p[0][q] : (q < n[0] + n[1] ? p[1][q - n[0]] : p[2][q - n[0] - n[1]]); }
};
__device__ __forceinline__ TbCat tb_cat(const TbTab& T, const long long* start, const int* lists, long long e) {
  TbCat C;
  for (int k = 0; k < 3; ++k) {
    const int nd = T.face[3 * e + k] - 1;
    C.p[k] = lists + start[nd];
    C.n[k] = (int)(start[nd + 1] - start[nd]);
  }
  return C;
}
// a neighbour counts at its first occurrence
__device__ __forceinline__ bool tb_first(const TbCat& C, int q, int v, long long e) {
  if (v == (int)e) return false;
  for (int r = 0; r < q; ++r)
    if (C.at(r) == v) return false;
  return true;
}
__global__ __launch_bounds__(256) void k_tube_row_count(TbTab T, const long long* start, const int* lists, int* rowcnt) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= T.nElts) return;
  const TbCat C = tb_cat(T, start, lists, e);
  int c = 0;
  for (int q = 0; q < C.total(); ++q) c += tb_first(C, q, C.at(q), e) ? 1 : 0;
  rowcnt[e] = c;
}
__global__ __launch_bounds__(256) void k_tube_row_write(TbTab T, const long long* start, const int* lists, const long long* rowptr, int* cols) {
  const long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (e >= T.nElts) return;
  const TbCat C = tb_cat(T, start, lists, e);
  int* row = cols + rowptr[e];
  int m = 0;
  for (int q = 0; q < C.total(); ++q) {
    const int v = C.at(q);
    if (!tb_first(C, q, v, e)) continue;
    int k = m++;  // insertion into the ascending row (a std::set's order)
    for (; k > 0 && row[k - 1] > v; --k) row[k] = row[k - 1];
    row[k] = v;
  }
}
// smoothVals (:274-298): one pass
__global__ __launch_bounds__(256) void k_tube_smooth(long long nElts, const long long* rowptr, const int* cols, const double* vals, const double* area, double* out) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= nElts) return;
  const long long r0 = rowptr[i], r1 = rowptr[i + 1];
  double accumArea = area[i];
  for (long long q = r0; q < r1; ++q) accumArea += area[cols[q]];
  double accumWt = vals[i] * area[i];
  for (long long q = r0; q < r1; ++q) accumWt += vals[cols[q]] * area[cols[q]];
  out[i] = accumWt / accumArea;
}

inline dim3 tb_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }
inline TbTab tb_tab(const pa_tube* t) { return TbTab{t->d_box, t->d_node, t->d_face, t->nNodes, t->nElts}; }

template <int KC>
void tb_launch_wedges(pa_ctx* ctx, const TbWedgeArgs& a) {
  hipLaunchKernelGGL(k_tube_wedges<KC>, tb_grid(a.T.nElts), dim3(256), 0, ctx->stream, a);
}

int tb_build_csr(pa_ctx* ctx, pa_tube* t) {
  if (t->nnz >= 0) return 0;
  const long long nN = t->nNodes, nE = t->nElts;
  int *cnt = nullptr, *lists = nullptr, *rowcnt = nullptr;
  long long* start = nullptr;
  int rc = 0;
  do {
    if (hipMalloc(&cnt, sizeof(int) * (size_t)std::max<long long>(nN, 1)) != hipSuccess || hipMalloc(&start, sizeof(long long) * (size_t)(nN + 1)) != hipSuccess ||
        hipMalloc(&lists, sizeof(int) * (size_t)std::max<long long>(3 * nE, 1)) != hipSuccess || hipMalloc(&rowcnt, sizeof(int) * (size_t)std::max<long long>(nE, 1)) != hipSuccess ||
        hipMalloc(&t->d_rowptr, sizeof(long long) * (size_t)(nE + 1)) != hipSuccess) { rc = pa_fail(ctx, "pa_tube: device allocation failed (neighbours)"); break; }
    const TbTab T = tb_tab(t);
    if (hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)std::max<long long>(nN, 1), ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_tube: memset failed"); break; }
    if (nE > 0) hipLaunchKernelGGL(k_tube_count_inc, tb_grid(3 * nE), dim3(256), 0, ctx->stream, T, cnt);
    hipLaunchKernelGGL(k_tube_scan, dim3(1), dim3(1024), 0, ctx->stream, cnt, start, nN);
    if (hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)std::max<long long>(nN, 1), ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_tube: memset failed"); break; }
    if (nE > 0) {
      hipLaunchKernelGGL(k_tube_fill_inc, tb_grid(3 * nE), dim3(256), 0, ctx->stream, T, start, cnt, lists);
      hipLaunchKernelGGL(k_tube_row_count, tb_grid(nE), dim3(256), 0, ctx->stream, T, start, lists, rowcnt);
    }
    hipLaunchKernelGGL(k_tube_scan, dim3(1), dim3(1024), 0, ctx->stream, rowcnt, t->d_rowptr, nE);
    long long nnz = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&nnz, t->d_rowptr + nE, sizeof nnz, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_tube: neighbour count failed"); break; }
    if (hipMalloc(&t->d_cols, sizeof(int) * (size_t)std::max<long long>(nnz, 1)) != hipSuccess) { rc = pa_fail(ctx, "pa_tube: device allocation failed (neighbour columns)"); break; }
    if (nE > 0) hipLaunchKernelGGL(k_tube_row_write, tb_grid(nE), dim3(256), 0, ctx->stream, T, start, lists, t->d_rowptr, t->d_cols);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_tube: neighbour fill failed"); break; }
    t->nnz = nnz;
  } while (0);
  for (void* p : {(void*)cnt, (void*)lists, (void*)rowcnt, (void*)start})
    if (p) (void)hipFree(p);
  if (rc != 0) {
    if (t->d_rowptr) (void)hipFree(t->d_rowptr);
    if (t->d_cols) (void)hipFree(t->d_cols);
    t->d_rowptr = nullptr;
    t->d_cols = nullptr;
  }
  return rc;
}

bool tb_comp_ok(int ncomp, int comp) { return ncomp >= 1 && comp >= 0 && comp < ncomp; }

}  // namespace

extern "C" pa_tube* pa_tube_create(pa_ctx* ctx, int32_t nbt, const int64_t* box_desc, int64_t nNodes, const int32_t* node_table, int64_t nElts,
                                   const int32_t* faceData) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  auto fail = [&](const std::string& m) -> pa_tube* { pa_fail(ctx, "pa_tube_create: " + m); return nullptr; };
  if (nbt < 1 || !box_desc || nNodes < 0 || nElts < 0 || (nNodes > 0 && !node_table) || (nElts > 0 && !faceData)) return fail("bad argument");
  if (nNodes >= (1LL << 31) / 3 || nElts >= (1LL << 31) / 3) return fail("more than 2^31 / 3 nodes or elements");
  for (int g = 0; g < nbt; ++g) {
    const int64_t* B = box_desc + 4 * g;
    if (B[0] < 1 || B[1] < 1 || B[0] >= (1LL << 31) || B[1] >= (1LL << 31) || B[2] < -(1LL << 30) || B[2] > (1LL << 30) || B[3] < 0) return fail("box " + std::to_string(g) + ": bad (ni, nj, jlo, offset)");
  }
  std::unique_ptr<pa_tube> t(new pa_tube);
  t->ctx = ctx;
  t->nbt = nbt;
  t->nNodes = nNodes;
  t->nElts = nElts;
  t->box.assign(box_desc, box_desc + 4 * (size_t)nbt);
  t->node.assign(node_table, node_table + 2 * (size_t)nNodes);
  t->has.assign((size_t)nbt, 0);
  for (long long n = 0; n < nNodes; ++n) {
    const int b = t->node[2 * (size_t)n], i = t->node[2 * (size_t)n + 1];
    if (b < 0 || b >= nbt) return fail("node " + std::to_string(n + 1) + ": box " + std::to_string(b) + " out of range");
    if (i < 0 || i >= t->box[4 * (size_t)b]) return fail("node " + std::to_string(n + 1) + ": line " + std::to_string(i) + " outside its box");
    t->has[(size_t)b] = 1;
  }
  for (long long q = 0; q < 3 * nElts; ++q)
    if (faceData[q] < 1 || faceData[q] > nNodes)
      return fail("element " + std::to_string(q / 3) + ": node id " + std::to_string(faceData[q]) + " outside 1 .. " + std::to_string(nNodes));
  std::vector<int> order((size_t)nNodes);
  for (long long n = 0; n < nNodes; ++n) order[(size_t)n] = (int)n;
  std::sort(order.begin(), order.end(), [&](int p, int q) {
    const int *a = &t->node[2 * (size_t)p], *b = &t->node[2 * (size_t)q];
    return a[0] != b[0] ? a[0] < b[0] : (a[1] != b[1] ? a[1] < b[1] : p < q);
  });
  const size_t nb = sizeof(long long) * 4 * (size_t)nbt, nn = sizeof(int) * 2 * (size_t)std::max<long long>(nNodes, 1), nf = sizeof(int) * 3 * (size_t)std::max<long long>(nElts, 1),
               no = sizeof(int) * (size_t)std::max<long long>(nNodes, 1);
  bool ok = hipMalloc(&t->d_box, nb) == hipSuccess && hipMalloc(&t->d_node, nn) == hipSuccess && hipMalloc(&t->d_face, nf) == hipSuccess && hipMalloc(&t->d_order, no) == hipSuccess;
  ok = ok && hipMemcpy(t->d_box, t->box.data(), nb, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && nNodes > 0)
    ok = hipMemcpy(t->d_node, t->node.data(), sizeof(int) * 2 * (size_t)nNodes, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(t->d_order, order.data(), sizeof(int) * (size_t)nNodes, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && nElts > 0) ok = hipMemcpy(t->d_face, faceData, sizeof(int) * 3 * (size_t)nElts, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    pa_tube_destroy(t.release());
    return fail("device allocation or copy failed");
  }
  return t.release();
}

extern "C" void pa_tube_destroy(pa_tube* t) {
  if (!t) return;
  PaBind bind_(t->ctx);
  for (void* p : {(void*)t->d_box, (void*)t->d_node, (void*)t->d_face, (void*)t->d_order, (void*)t->d_rowptr, (void*)t->d_cols})
    if (p) (void)hipFree(p);
  delete t;
}

extern "C" int pa_tube_wedges(pa_ctx* ctx, pa_tube* t, const double* xyz, const double* data, int32_t K, int32_t jlo, int32_t nPtsOnStr, int32_t with_geom,
                              double* vol, double* area, double* wa, double* ints_raw, double* ints_per_area) {
  PaBind bind_(ctx);
  if (!ctx || !t || K < 0) return pa_fail(ctx, "pa_tube_wedges: bad argument");
  if (t->nElts == 0) return 0;
  if (!xyz || (K > 0 && (!data || !ints_raw || !ints_per_area)) || (with_geom && (!vol || !area || !wa))) return pa_fail(ctx, "pa_tube_wedges: null device array");
  for (int g = 0; g < t->nbt; ++g) {  // before any launch: every box with lines holds j = 0 and the swept range
    if (!t->has[(size_t)g]) continue;
    const long long bj = t->box[4 * (size_t)g + 2], bn = t->box[4 * (size_t)g + 1];
    const bool swept = nPtsOnStr >= 2;
    if (bj > 0 || bj + bn - 1 < 0 || (swept && (bj > jlo || bj + bn - 1 < (long long)jlo + nPtsOnStr - 1)))
      return pa_fail(ctx, "pa_tube_wedges: Str box " + std::to_string(g) + " (j = " + std::to_string(bj) + " .. " + std::to_string(bj + bn - 1) + ") does not hold j = 0 and j = " +
                              std::to_string(jlo) + " .. " + std::to_string((long long)jlo + nPtsOnStr - 1));
  }
  TbWedgeArgs a{tb_tab(t), xyz, data, (int)std::max(K, 1), 0, (int)jlo, (int)nPtsOnStr, with_geom ? 1 : 0, vol, area, wa, ints_raw, ints_per_area};
  if (K == 0) {
    if (with_geom) tb_launch_wedges<0>(ctx, a);
  } else {
    for (int c = 0; c < K;) {  // sweeps of 8, 4, 2, 1 components; the first one carries the geometry
      a.c0 = c;
      a.geom = (with_geom && c == 0) ? 1 : 0;
      const int left = K - c;
      if (left >= 8) { tb_launch_wedges<8>(ctx, a); c += 8; }
      else if (left >= 4) { tb_launch_wedges<4>(ctx, a); c += 4; }
      else if (left >= 2) { tb_launch_wedges<2>(ctx, a); c += 2; }
      else { tb_launch_wedges<1>(ctx, a); c += 1; }
    }
  }
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_tube_wedges: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_tube_lines(pa_ctx* ctx, pa_tube* t, const double* xyz, const double* data, int32_t ncomp, int32_t comp, int32_t use_eps, double* gradmax) {
  PaBind bind_(ctx);
  if (!ctx || !t || !tb_comp_ok(ncomp, comp)) return pa_fail(ctx, "pa_tube_lines: bad argument (component out of range)");
  if (t->nNodes == 0) return 0;
  if (!xyz || !data || !gradmax) return pa_fail(ctx, "pa_tube_lines: null device array");
  hipLaunchKernelGGL(k_tube_grad, tb_grid(t->nNodes), dim3(256), 0, ctx->stream, tb_tab(t), t->d_order, xyz, data, (int)ncomp, (int)comp, use_eps ? 1 : 0, gradmax);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_tube_lines: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_tube_peaks(pa_ctx* ctx, pa_tube* t, const double* data, int32_t ncomp, int32_t pcomp, int32_t nsample, const int32_t* sample_comps,
                             double* peak_samples, int32_t* ok) {
  PaBind bind_(ctx);
  if (!ctx || !t || !tb_comp_ok(ncomp, pcomp) || nsample < 0 || nsample > PA_TUBE_MAXSAMPLE || (nsample > 0 && !sample_comps))
    return pa_fail(ctx, "pa_tube_peaks: bad argument (component out of range, or more than 32 sampled components)");
  TbSample S{};
  S.n = nsample;
  for (int s = 0; s < nsample; ++s) {
    if (!tb_comp_ok(ncomp, sample_comps[s])) return pa_fail(ctx, "pa_tube_peaks: sampled component out of range");
    S.comp[s] = sample_comps[s];
  }
  if (t->nNodes == 0) return 0;
  if (!data || !ok || (nsample > 0 && !peak_samples)) return pa_fail(ctx, "pa_tube_peaks: null device array");
  hipLaunchKernelGGL(k_tube_peak, tb_grid(t->nNodes), dim3(256), 0, ctx->stream, tb_tab(t), t->d_order, data, (int)ncomp, (int)pcomp, S, peak_samples, ok);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_tube_peaks: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_tube_node_means(pa_ctx* ctx, pa_tube* t, int32_t nv, const double* vals, double* out) {
  PaBind bind_(ctx);
  if (!ctx || !t || nv < 0) return pa_fail(ctx, "pa_tube_node_means: bad argument");
  if (t->nElts == 0 || nv == 0) return 0;
  if (!vals || !out) return pa_fail(ctx, "pa_tube_node_means: null device array");
  hipLaunchKernelGGL(k_tube_means, tb_grid(t->nElts), dim3(256), 0, ctx->stream, tb_tab(t), (int)nv, vals, out);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_tube_node_means: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_tube_node_all(pa_ctx* ctx, pa_tube* t, const int32_t* ok, double* out) {
  PaBind bind_(ctx);
  if (!ctx || !t) return pa_fail(ctx, "pa_tube_node_all: bad argument");
  if (t->nElts == 0) return 0;
  if (!ok || !out) return pa_fail(ctx, "pa_tube_node_all: null device array");
  hipLaunchKernelGGL(k_tube_all, tb_grid(t->nElts), dim3(256), 0, ctx->stream, tb_tab(t), ok, out);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_tube_node_all: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_tube_node_avg(pa_ctx* ctx, pa_tube* t, const double* data, int32_t ncomp, int32_t comp, double* out) {
  PaBind bind_(ctx);
  if (!ctx || !t || !tb_comp_ok(ncomp, comp)) return pa_fail(ctx, "pa_tube_node_avg: bad argument (component out of range)");
  if (t->nElts == 0) return 0;
  if (!data || !out) return pa_fail(ctx, "pa_tube_node_avg: null device array");
  for (int g = 0; g < t->nbt; ++g)
    if (t->has[(size_t)g] && (t->box[4 * (size_t)g + 2] > 0 || t->box[4 * (size_t)g + 2] + t->box[4 * (size_t)g + 1] - 1 < 0))
      return pa_fail(ctx, "pa_tube_node_avg: Str box " + std::to_string(g) + " does not hold j = 0");
  hipLaunchKernelGGL(k_tube_avg, tb_grid(t->nElts), dim3(256), 0, ctx->stream, tb_tab(t), data, (int)ncomp, (int)comp, out);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_tube_node_avg: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_tube_smooth(pa_ctx* ctx, pa_tube* t, const double* vals, const double* area, int32_t nSmooth, double* out) {
  PaBind bind_(ctx);
  if (!ctx || !t) return pa_fail(ctx, "pa_tube_smooth: bad argument");
  if (t->nElts == 0) return 0;
  if (!vals || !area || !out) return pa_fail(ctx, "pa_tube_smooth: null device array");
  const size_t bytes = sizeof(double) * (size_t)t->nElts;
  if (nSmooth <= 0) {
    PA_HIP(hipMemcpyAsync(out, vals, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return pa_sync(ctx);
  }
  if (tb_build_csr(ctx, t) != 0) return 1;
  double* tmp = nullptr;  // ping-pong partner of out: pass p writes out when nSmooth - p is odd, so the last pass lands in out
  if (nSmooth > 1) PA_HIP(hipMalloc(&tmp, bytes));
  const double* src = vals;
  for (int p = 0; p < nSmooth; ++p) {
    double* dst = ((nSmooth - p) & 1) ? out : tmp;
    hipLaunchKernelGGL(k_tube_smooth, tb_grid(t->nElts), dim3(256), 0, ctx->stream, t->nElts, t->d_rowptr, t->d_cols, src, area, dst);
    src = dst;
  }
  int rc = hipGetLastError() != hipSuccess ? pa_fail(ctx, "pa_tube_smooth: launch failed") : pa_sync(ctx);
  if (tmp) (void)hipFree(tmp);
  return rc;
}

extern "C" int pa_tube_neighbors(pa_ctx* ctx, pa_tube* t, int64_t* nnz, int64_t* rowptr, int32_t* cols) {
  PaBind bind_(ctx);
  if (!ctx || !t || !nnz) return pa_fail(ctx, "pa_tube_neighbors: bad argument");
  if (tb_build_csr(ctx, t) != 0) return 1;
  *nnz = t->nnz;
  if (rowptr) PA_HIP(hipMemcpy(rowptr, t->d_rowptr, sizeof(long long) * (size_t)(t->nElts + 1), hipMemcpyDeviceToHost));
  if (cols && t->nnz > 0) PA_HIP(hipMemcpy(cols, t->d_cols, sizeof(int) * (size_t)t->nnz, hipMemcpyDeviceToHost));
  return 0;
}
