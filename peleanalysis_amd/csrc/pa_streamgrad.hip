// pa_streamgrad.hip -- the gradient streamlines of stream.cpp / stream_nd.f90 on gfx950 (the stream3d tool):
// lines of grad(progress) (or of the velocity, traceAlongV) seeded on isosurface nodes.  Unlike partStream (pa_stream.hip) a
// line never changes FAB: every seed belongs to one (level, file box) (stream.cpp:730-766) and vtrace runs inside that box's
// FAB, nGrow ghost layers included, until a step would leave it -- the position then stays put (RK4 returns before it moves
// x) and the line is "cut short".
//   k_sg_prep:  the ghost cells of one level as stream.cpp:796-884 leaves them (one launch per level, coarse to fine).
//   k_sg_trace: every line of the hierarchy in one launch, two threads per seed (backward, forward), written straight into
//               the Str FAB layout; the gradient g = T(i+1) - T(i-1) is formed at the 8 corners on the fly (one subtraction:
//               the same bits as the reference's materialised g, stream_nd.f90:33-44).
//   k_sg_grad + k_sg_fab: pa_vtrace_fab, one MFIter iteration of stream.cpp:920-925 (materialised g, as vtrace does).
// Gather- and latency-bound: per RK4 stage 8 corners x 3 components (x 2 loads on the fly), 4 stages per step.
#include "pa_internal.h"
#include <cmath>
#include <vector>

#define PA_SG_MAXLEV 8

// a FAB as vtrace sees it: box lo..hi (ghost cells included), x fastest, component stride cs
struct SgFab {
  const double* p;
  int lo[3], hi[3];
  long long cs;
  __device__ __forceinline__ long long sy() const { return hi[0] - lo[0] + 1; }
  __device__ __forceinline__ long long sz() const { return (long long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1); }
  __device__ __forceinline__ long long idx(int i, int j, int k) const { return ((long long)(k - lo[2]) * (hi[1] - lo[1] + 1) + (j - lo[1])) * (hi[0] - lo[0] + 1) + (i - lo[0]); }
};

struct SgGeom {
  double dx[3], plo[3], phi[3];
};

// ntrpv (stream_nd.f90:158-211) up to the sum: IsOK on the closed [plo, phi], the base cell b and the weights n, then b in
// [blo, bhi - 1] (blo / bhi: the bounds of the interpolated array)
__device__ __forceinline__ bool sg_locate(const SgGeom& G, const double x[3], const int blo[3], const int bhi[3], int b[3], double n[3]) {
#pragma unroll
  for (int d = 0; d < 3; ++d)
    if (x[d] < G.plo[d] || x[d] > G.phi[d]) return false;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double tmp = (x[d] - G.plo[d]) / G.dx[d] - 0.5;
    b[d] = (int)floor(tmp);
    double v = (x[d] - ((b[d] + 0.5) * G.dx[d] + G.plo[d])) / G.dx[d];
    v = (v < 1.0) ? v : 1.0;  // MIN(1.d0, n)
    n[d] = (0.0 < v) ? v : 0.0;  // MAX(0.d0, .)
  }
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d)
    if (b[d] < blo[d] || b[d] > bhi[d] - 1) ok = false;
  return ok;
}

// ntrpv of component m of F (bounds = F's box)
__device__ __forceinline__ bool sg_ntrp(const SgGeom& G, const SgFab& F, int m, const double x[3], double& u) {
  int b[3];
  double n[3];
  if (!sg_locate(G, x, F.lo, F.hi, b, n)) return false;
  const double* q = F.p + (long long)m * F.cs + F.idx(b[0], b[1], b[2]);
  const long long sy = F.sy(), sz = F.sz();
  u = sg_sum(n, [&](int di, int dj, int dk) { return q[di + dj * sy + dk * sz]; });
  return true;
}

// the vector field of RK4: mode 0 = g = centred differences of T component 0 on the fly, bounds T's box grown by -1 (the
// reference's g box, stream.cpp:910); mode 1 = components vc..vc+2 of V, bounds V's box (traceAlongV, and pa_vtrace_fab's g)
struct SgVec {
  SgFab F;
  int mode, vc;
};
__device__ __forceinline__ bool sg_vec(const SgGeom& G, const SgVec& V, const double x[3], double u[3]) {
  int b[3];
  double n[3];
  const SgFab& F = V.F;
  const long long sy = F.sy(), sz = F.sz();
  if (V.mode == 0) {
    const int glo[3] = {F.lo[0] + 1, F.lo[1] + 1, F.lo[2] + 1}, ghi[3] = {F.hi[0] - 1, F.hi[1] - 1, F.hi[2] - 1};
    if (!sg_locate(G, x, glo, ghi, b, n)) return false;
    const double* q = F.p + F.idx(b[0], b[1], b[2]);
    const long long s[3] = {1, sy, sz};
#pragma unroll
    for (int c = 0; c < 3; ++c)
      u[c] = sg_sum(n, [&](int di, int dj, int dk) {
        const double* r = q + di + dj * sy + dk * sz;
        return r[s[c]] - r[-s[c]];
      });
    return true;
  }
  if (!sg_locate(G, x, F.lo, F.hi, b, n)) return false;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double* q = F.p + (long long)(V.vc + c) * F.cs + F.idx(b[0], b[1], b[2]);
    u[c] = sg_sum(n, [&](int di, int dj, int dk) { return q[di + dj * sy + dk * sz]; });
  }
  return true;
}

// vnrml (stream_nd.f90:213-225): eps = 1.e-12 is a default-real literal
__device__ __forceinline__ void sg_vnrml(double v[3]) {
  const double eps = (double)1.e-12f;
  double sum = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) sum = sum + v[i] * v[i];
  if (sum > eps) {
    sum = sqrt(sum);
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = v[i] / sum;
  }
}

// RK4 (stream_nd.f90:122-156): x only moves when all four stages interpolate
__device__ __forceinline__ bool sg_rk4(const SgGeom& G, const SgVec& V, double x[3], double h) {
  double xx[3], vec[3], k1[3], k2[3], k3[3], k4[3];
  if (!sg_vec(G, V, x, vec)) return false;
  sg_vnrml(vec);
  for (int d = 0; d < 3; ++d) { k1[d] = vec[d] * h; xx[d] = x[d] + k1[d] * 0.5; }
  if (!sg_vec(G, V, xx, vec)) return false;
  sg_vnrml(vec);
  for (int d = 0; d < 3; ++d) { k2[d] = vec[d] * h; xx[d] = x[d] + k2[d] * 0.5; }
  if (!sg_vec(G, V, xx, vec)) return false;
  sg_vnrml(vec);
  for (int d = 0; d < 3; ++d) { k3[d] = vec[d] * h; xx[d] = x[d] + k3[d]; }
  if (!sg_vec(G, V, xx, vec)) return false;
  sg_vnrml(vec);
  for (int d = 0; d < 3; ++d) {
    k4[d] = vec[d] * h;
    x[d] = x[d] + (k1[d] + k4[d]) / 6.0 + (k2[d] + k3[d]) / 3.0;
  }
  return true;
}

// One half of vtrace's loop body for seed i of a box (stream_nd.f90:53-107): dir 1 writes n = 0 and the forward steps
// n = 1 .. nfwd, dir 0 the backward steps n = -1 .. -nRKh.  out(c, n) -> the Str FAB element.  Returns 0, 1 (a state component
// does not interpolate at the seed: "Problem with interpolation") or 2 / 4 (some step of this half was cut short).
template <typename O>
__device__ __forceinline__ int sg_line(const SgGeom& G, const SgFab& T, int nT, const SgVec& V, const double x0[3], int dir, int nRKh, int nfwd,
                                       double hRK, O out) {
  double x[3] = {x0[0], x0[1], x0[2]};
  if (dir) for (int d = 0; d < 3; ++d) out(d, 0) = x[d];
  for (int m = 0; m < nT; ++m) {
    double u;
    if (!sg_ntrp(G, T, m, x, u)) return 1;
    if (dir) out(3 + m, 0) = u;
  }
  const int nlen = dir ? nfwd : nRKh, sgn = dir ? 1 : -1;
  const double h = dir ? hRK : -hRK;
  int err = 0;
  for (int s = 1; s <= nlen; ++s) {
    const int n = sgn * s;
    if (!sg_rk4(G, V, x, h)) err = dir ? 4 : 2;
    for (int d = 0; d < 3; ++d) out(d, n) = x[d];
    for (int m = 0; m < nT; ++m) {
      double u;
      if (!sg_ntrp(G, T, m, x, u)) {
        // the neighbour one step nearer the seed; at |n| = 1 that is the seed's value (written by the other half: recomputed)
        if (s == 1) (void)sg_ntrp(G, T, m, x0, u);
        else u = out(3 + m, n - sgn);  // this thread's own store of the previous step
      }
      out(3 + m, n) = u;
    }
  }
  return err;
}

// ------------------------------------------------------------------------------------------------ the hierarchy trace
struct SgLevels {
  int nlev, ng, ncomp, vcomp, nRKsteps, nRKh;
  int boxcum[PA_SG_MAXLEV + 1];  // global box numbers of level l: boxcum[l] .. boxcum[l+1]-1
  const DBox* boxes[PA_SG_MAXLEV];
  DMFView V[PA_SG_MAXLEV];
  double dx[PA_SG_MAXLEV][3], plo[3], phi[3], hRK;
};

__global__ __launch_bounds__(256) void k_sg_trace(SgLevels S, long long nlines, int nbt, const long long* __restrict__ bstart, const int* __restrict__ ids,
                                                  long long nnodes, const double* __restrict__ nodes, double* strm, int* flags /* [nbt] keys, [nbt] errFlag 1 */) {
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= 2 * nlines) return;
  const long long line = q >> 1;
  const int dir = (int)(q & 1);
  int lo = 0, hi = nbt;  // box g with bstart[g] <= line < bstart[g+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (bstart[mid] <= line) lo = mid; else hi = mid;
  }
  const int g = lo;
  int l = 0;
  while (l + 1 < S.nlev && g >= S.boxcum[l + 1]) ++l;
  const int b = g - S.boxcum[l];
  const DBox B = S.boxes[l][b];
  SgFab T;
  T.p = S.V[l].data + S.V[l].off[b];
  for (int d = 0; d < 3; ++d) { T.lo[d] = B.lo[d] - S.ng; T.hi[d] = B.hi[d] + S.ng; }
  T.cs = pa_cstride((long long)(T.hi[0] - T.lo[0] + 1) * (T.hi[1] - T.lo[1] + 1) * (T.hi[2] - T.lo[2] + 1), S.ncomp);
  SgVec V{T, S.vcomp < 0 ? 0 : 1, S.vcomp < 0 ? 0 : S.vcomp};
  SgGeom G;
  for (int d = 0; d < 3; ++d) { G.dx[d] = S.dx[l][d]; G.plo[d] = S.plo[d]; G.phi[d] = S.phi[d]; }
  const long long i = line - bstart[g], nj = bstart[g + 1] - bstart[g];
  const long long node = ids[line] - 1;
  const double x0[3] = {nodes[node], nodes[nnodes + node], nodes[2 * nnodes + node]};
  double* seg = strm + bstart[g] * (long long)S.nRKsteps * (3 + S.ncomp);
  const long long plane = nj * S.nRKsteps;
  const int nRKh = S.nRKh;
  auto out = [=](int c, int n) -> double& { return seg[(long long)c * plane + (long long)(n + nRKh) * nj + i]; };
  const int e = sg_line(G, T, S.ncomp, V, x0, dir, nRKh, S.nRKsteps - 1 - nRKh, S.hRK, out);
  if (e == 1) atomicOr(&flags[nbt + g], 1);
  else if (e) atomicMax(&flags[g], (int)(2 * i + dir + 1));  // the LAST cut-short event of the box decides its errFlag
}

// ------------------------------------------------------------------------------------------------ state preparation
struct SgPrep {
  DLevelView L, LC;
  DMFView M, MC;
  int ncomp, ratio, level;
};

// one thread per cell of the FABs of box blockIdx.y (ghost cells included); valid cells are not touched
__global__ __launch_bounds__(256) void k_sg_prep(SgPrep P, int* bad) {
  const int b = blockIdx.y;
  const DBox B = P.L.boxes[b];
  const int ng = P.M.ng;
  const long long nx = B.hi[0] - B.lo[0] + 1 + 2 * ng, ny = B.hi[1] - B.lo[1] + 1 + 2 * ng, nz = B.hi[2] - B.lo[2] + 1 + 2 * ng;
  const long long ncell = nx * ny * nz, cs = pa_cstride(ncell, P.ncomp);
  double* f = P.M.data + P.M.off[b];
  for (long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x; c < ncell; c += (long long)gridDim.x * blockDim.x) {
    const int p[3] = {B.lo[0] - ng + (int)(c % nx), B.lo[1] - ng + (int)((c / nx) % ny), B.lo[2] - ng + (int)(c / (nx * ny))};
    bool valid = true, inside = true;
    for (int d = 0; d < 3; ++d) {
      valid = valid && p[d] >= B.lo[d] && p[d] <= B.hi[d];
      inside = inside && p[d] >= P.L.domlo[d] && p[d] <= P.L.domhi[d];
    }
    if (valid) continue;
    const double* src = nullptr;
    long long sstride = 0;
    if (inside) {
      const int o = owner_of(P.L, p);
      if (o >= 0) {  // FillBoundary: a valid cell of another box of the level
        src = P.M.data + P.M.off[o] + fab_index(P.L.boxes[o], ng, P.ncomp, 0, p[0], p[1], p[2]);
        sstride = pa_cstride((long long)(P.L.boxes[o].hi[0] - P.L.boxes[o].lo[0] + 1 + 2 * ng) * (P.L.boxes[o].hi[1] - P.L.boxes[o].lo[1] + 1 + 2 * ng) *
                             (P.L.boxes[o].hi[2] - P.L.boxes[o].lo[2] + 1 + 2 * ng), P.ncomp);
      } else if (P.level > 0) {  // FillCFgrowCells: the prepared coarse value of the parent cell
        const int r = P.ratio;
        int qc[3];
        for (int d = 0; d < 3; ++d) qc[d] = coarsen_idx(p[d], r);
        // a parent inside the coarsened fine BoxArray is not in GetBndryCells' coarse boxes: the reference copies an unset value
        bool partly = false;
        for (int dk = 0; dk < r && !partly; ++dk)
          for (int dj = 0; dj < r && !partly; ++dj)
            for (int di = 0; di < r && !partly; ++di) {
              const int s[3] = {qc[0] * r + di, qc[1] * r + dj, qc[2] * r + dk};
              partly = owner_of(P.L, s) >= 0;
            }
        const int ngc = P.MC.ng;
        int o2 = partly ? -1 : owner_of(P.LC, qc);
        if (!partly && o2 < 0)  // a ghost cell of some coarse FAB (they all hold the same value there)
          for (int bc = 0; bc < P.LC.nboxes && o2 < 0; ++bc) {
            const DBox& C = P.LC.boxes[bc];
            bool in = true;
            for (int d = 0; d < 3; ++d) in = in && qc[d] >= C.lo[d] - ngc && qc[d] <= C.hi[d] + ngc;
            if (in) o2 = bc;
          }
        if (o2 < 0) {
          atomicOr(bad, 1);
          continue;
        }
        const DBox& C = P.LC.boxes[o2];
        src = P.MC.data + P.MC.off[o2] + fab_index(C, ngc, P.ncomp, 0, qc[0], qc[1], qc[2]);
        sstride = pa_cstride((long long)(C.hi[0] - C.lo[0] + 1 + 2 * ngc) * (C.hi[1] - C.lo[1] + 1 + 2 * ngc) * (C.hi[2] - C.lo[2] + 1 + 2 * ngc), P.ncomp);
      }
    }
    for (int m = 0; m < P.ncomp; ++m) f[m * cs + c] = src ? src[m * sstride] : 0.0;  // FixOOB / uncovered level-0 cells: 0
  }
}

static int sg_ratio(const pa_level* F, const pa_level* C) {
  int r = 0;
  for (int d = 0; d < 3; ++d) {
    const int nf = F->domhi[d] - F->domlo[d] + 1, nc = C->domhi[d] - C->domlo[d] + 1;
    if (nc <= 0 || nf % nc != 0) return 0;
    if (d == 0) r = nf / nc;
    else if (nf / nc != r) return 0;
  }
  return r;
}

extern "C" int pa_streamgrad_prepare(pa_ctx* ctx, int nlev, pa_mf* const* state) {
  PaBind bind_(ctx);
  if (!ctx || !state || nlev <= 0) return pa_fail(ctx, "pa_streamgrad_prepare: bad argument");
  for (int l = 0; l < nlev; ++l) {
    const pa_mf* m = state[l];
    if (!m || m->ncomp != state[0]->ncomp || m->ng != state[0]->ng) return pa_fail(ctx, "pa_streamgrad_prepare: every level needs the same components and nGrow");
    if (m->lev->nremote > 0) return pa_fail(ctx, "pa_streamgrad_prepare: levels sharded across ranks are not supported");
  }
  int* dbad = nullptr;
  PA_HIP(hipMalloc(&dbad, sizeof(int)));
  PA_HIP(hipMemsetAsync(dbad, 0, sizeof(int), ctx->stream));
  int rc = 0;
  for (int l = 0; l < nlev && rc == 0; ++l) {
    SgPrep P{};
    P.L = state[l]->lev->view;
    P.M = state[l]->view;
    P.ncomp = state[l]->ncomp;
    P.level = l;
    if (l > 0) {
      P.LC = state[l - 1]->lev->view;
      P.MC = state[l - 1]->view;
      P.ratio = sg_ratio(state[l]->lev, state[l - 1]->lev);
      if (P.ratio < 2) { rc = pa_fail(ctx, "pa_streamgrad_prepare: the domains of levels " + std::to_string(l - 1) + " and " + std::to_string(l) + " are not related by one integer ratio >= 2"); break; }
    }
    const int nb = (int)state[l]->lev->boxes.size();
    if (nb == 0) continue;
    long long mx = 0;
    for (const DBox& B : state[l]->lev->boxes) {
      long long n = 1;
      for (int d = 0; d < 3; ++d) n *= B.hi[d] - B.lo[d] + 1 + 2 * state[l]->ng;
      mx = std::max(mx, n);
    }
    const unsigned gx = (unsigned)std::min<long long>((mx + 255) / 256, 1024);
    hipLaunchKernelGGL(k_sg_prep, dim3(gx, nb), dim3(256), 0, ctx->stream, P, dbad);
    if (hipGetLastError() != hipSuccess) rc = pa_fail(ctx, "pa_streamgrad_prepare: launch failed");
  }
  int hbad = 0;
  if (rc == 0 && (hipMemcpyAsync(&hbad, dbad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
    rc = pa_fail(ctx, "pa_streamgrad_prepare: synchronisation failed");
  (void)hipFree(dbad);
  if (rc == 0 && hbad)
    rc = pa_fail(ctx, "pa_streamgrad_prepare: a coarse-fine ghost cell has no coarse value (FillCFgrowCells would copy an unset one): the fine level is not "
                      "properly nested in the coarse one, or a fine box is not aligned to the refinement ratio");
  return rc;
}

static int sg_final_flag(int key, int f1) {
  if (f1) return 1;
  if (key == 0) return 0;
  return ((key - 1) & 1) ? 4 : 2;
}

extern "C" int pa_streamgrad_trace(pa_ctx* ctx, int nlev, pa_mf* const* state, int vcomp, int64_t nnodes, const double* nodes, const int64_t* box_start,
                                   const int32_t* ids, int nRKsteps, double hRK, double* strm, int32_t* box_flag) {
  PaBind bind_(ctx);
  if (!ctx || !state || nlev <= 0 || nlev > PA_SG_MAXLEV || !box_start) return pa_fail(ctx, "pa_streamgrad_trace: bad argument (1 <= nlev <= 8)");
  if (nRKsteps < 1) return pa_fail(ctx, "pa_streamgrad_trace: nRKsteps must be at least 1");
  SgLevels S{};
  S.nlev = nlev;
  S.ng = state[0] ? state[0]->ng : 0;
  S.ncomp = state[0] ? state[0]->ncomp : 0;
  S.vcomp = vcomp;
  S.nRKsteps = nRKsteps;
  S.nRKh = (nRKsteps - 1) / 2;
  S.hRK = hRK;
  S.boxcum[0] = 0;
  for (int l = 0; l < nlev; ++l) {
    const pa_mf* m = state[l];
    if (!m || m->ng != S.ng || m->ncomp != S.ncomp) return pa_fail(ctx, "pa_streamgrad_trace: every level needs the same components and nGrow");
    if (m->ng < 1) return pa_fail(ctx, "pa_streamgrad_trace: nGrow must be at least 1");
    if (vcomp >= 0 && vcomp + 3 > m->ncomp) return pa_fail(ctx, "pa_streamgrad_trace: velocity components out of range");
    if (m->lev->nremote > 0) return pa_fail(ctx, "pa_streamgrad_trace: levels sharded across ranks are not supported");
    S.boxes[l] = m->lev->view.boxes;
    S.V[l] = m->view;
    S.boxcum[l + 1] = S.boxcum[l] + (int)m->lev->boxes.size();
    for (int d = 0; d < 3; ++d) S.dx[l][d] = (m->lev->prob_hi[d] - m->lev->prob_lo[d]) / (double)(m->lev->domhi[d] - m->lev->domlo[d] + 1);
  }
  for (int d = 0; d < 3; ++d) { S.plo[d] = state[0]->lev->prob_lo[d]; S.phi[d] = state[0]->lev->prob_hi[d]; }
  const int nbt = S.boxcum[nlev];
  if (box_start[0] != 0) return pa_fail(ctx, "pa_streamgrad_trace: box_start[0] must be 0");
  for (int g = 0; g < nbt; ++g)
    if (box_start[g + 1] < box_start[g]) return pa_fail(ctx, "pa_streamgrad_trace: box_start is not ascending");
  const long long nlines = box_start[nbt];
  if (nlines > 0 && (!nodes || !ids || !strm)) return pa_fail(ctx, "pa_streamgrad_trace: null device array");
  if (box_flag) for (int g = 0; g < nbt; ++g) box_flag[g] = 0;
  if (nlines == 0) return 0;
  long long* dstart = nullptr;
  int* dflags = nullptr;
  PA_HIP(hipMalloc(&dstart, sizeof(long long) * (size_t)(nbt + 1)));
  if (hipMalloc(&dflags, sizeof(int) * 2 * (size_t)nbt) != hipSuccess) { (void)hipFree(dstart); return pa_fail(ctx, "pa_streamgrad_trace: device allocation failed"); }
  int rc = 0;
  std::vector<int> hf(2 * (size_t)nbt);
  do {
    if (hipMemcpyAsync(dstart, box_start, sizeof(long long) * (size_t)(nbt + 1), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemsetAsync(dflags, 0, sizeof(int) * 2 * (size_t)nbt, ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_streamgrad_trace: copy failed"); break; }
    const unsigned gx = (unsigned)((2 * nlines + 255) / 256);
    hipLaunchKernelGGL(k_sg_trace, dim3(gx), dim3(256), 0, ctx->stream, S, nlines, nbt, dstart, ids, (long long)nnodes, nodes, strm, dflags);
    if (hipGetLastError() != hipSuccess) { rc = pa_fail(ctx, "pa_streamgrad_trace: launch failed"); break; }
    if (hipMemcpyAsync(hf.data(), dflags, sizeof(int) * hf.size(), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_streamgrad_trace: synchronisation failed"); break; }
    if (box_flag) for (int g = 0; g < nbt; ++g) box_flag[g] = sg_final_flag(hf[(size_t)g], hf[(size_t)(nbt + g)]);
  } while (0);
  (void)hipFree(dstart);
  (void)hipFree(dflags);
  return rc;
}

// ------------------------------------------------------------------------------------------------ pa_vtrace_fab
// g(i,j,k,:) = centred differences of T component 0 over g's box (stream_nd.f90:33-44)
__global__ __launch_bounds__(256) void k_sg_grad(SgFab T, SgFab g, double* gp) {
  const long long nx = g.hi[0] - g.lo[0] + 1, ny = g.hi[1] - g.lo[1] + 1, nz = g.hi[2] - g.lo[2] + 1;
  const long long c = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (c >= nx * ny * nz) return;
  const int i = g.lo[0] + (int)(c % nx), j = g.lo[1] + (int)((c / nx) % ny), k = g.lo[2] + (int)(c / (nx * ny));
  const double* t = T.p + T.idx(i, j, k);
  const long long sy = T.sy(), sz = T.sz();
  gp[c] = t[1] - t[-1];
  gp[g.cs + c] = t[sy] - t[-sy];
  gp[2 * g.cs + c] = t[sz] - t[-sz];
}

struct SgFabArgs {
  SgFab T, strm;
  SgVec V;
  SgGeom G;
  int nT, n_ids, nRKh, nfwd;
  double hRK;
};

__global__ __launch_bounds__(256) void k_sg_fab(SgFabArgs A, const int* __restrict__ ids, long long nloc, const double* __restrict__ loc, int* flags /* [0] key, [1] first seed with errFlag 1 */) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 2 * A.n_ids) return;
  const int i = q >> 1, dir = q & 1;
  const long long j = ids[i] - 1;
  const double x0[3] = {loc[j], loc[nloc + j], loc[2 * nloc + j]};
  double* sp = const_cast<double*>(A.strm.p);
  const SgFab& S = A.strm;
  auto out = [=](int c, int n) -> double& { return sp[(long long)c * S.cs + S.idx(i, n, S.lo[2])]; };
  const int e = sg_line(A.G, A.T, A.nT, A.V, x0, dir, A.nRKh, A.nfwd, A.hRK, out);
  if (e == 1) atomicMin(&flags[1], i);
  else if (e) atomicMax(&flags[0], 2 * i + dir + 1);
}

static bool sg_fab_of(const pa_fab* f, SgFab& s) {
  if (!f || !f->p) return false;
  s.p = f->p;
  for (int d = 0; d < 3; ++d) { s.lo[d] = f->lo[d]; s.hi[d] = f->hi[d]; if (s.hi[d] < s.lo[d]) return false; }
  s.cs = f->nstride;
  return true;
}

extern "C" int pa_vtrace_fab(pa_ctx* ctx, const pa_fab* T, int32_t nT, const double* loc, int64_t nloc, const int32_t* ids, int32_t n_ids, pa_fab* g,
                             int32_t computeVec, pa_fab* strm, int32_t ncs, const double dx[3], const double plo[3], const double phi[3], double hRK,
                             int32_t* errFlag) {
  PaBind bind_(ctx);
  SgFabArgs A{};
  if (!ctx || !dx || !plo || !phi || !errFlag || !sg_fab_of(T, A.T) || !sg_fab_of(g, A.V.F) || !sg_fab_of(strm, A.strm)) return pa_fail(ctx, "pa_vtrace_fab: bad argument");
  if (nT < 1 || nT > T->ncomp || ncs != 3 + nT || strm->ncomp < ncs || g->ncomp < 3) return pa_fail(ctx, "pa_vtrace_fab: component counts (ncs = 3 + nT)");
  if (n_ids > 0 && (!loc || !ids || nloc < 1)) return pa_fail(ctx, "pa_vtrace_fab: null node array");
  const int nRKh = -strm->lo[1], nsteps = strm->hi[1] - strm->lo[1] + 1;
  if (nRKh < 0 || strm->lo[0] != 0 || strm->hi[0] != n_ids - 1 || strm->hi[2] != strm->lo[2] || nRKh != (nsteps - 1) / 2)
    return pa_fail(ctx, "pa_vtrace_fab: strm must be the box (0, -nRKh, 0)..(n_ids-1, nRKsteps-1-nRKh, 0)");
  if (computeVec) {  // the centred differences read g's box grown by one from T
    for (int d = 0; d < 3; ++d)
      if (g->lo[d] - 1 < T->lo[d] || g->hi[d] + 1 > T->hi[d]) return pa_fail(ctx, "pa_vtrace_fab: g's box grown by one must lie inside T's box");
  }
  A.nT = nT; A.n_ids = n_ids; A.nRKh = nRKh; A.nfwd = nsteps - 1 - nRKh; A.hRK = hRK;
  A.V.mode = 1; A.V.vc = 0;
  for (int d = 0; d < 3; ++d) { A.G.dx[d] = dx[d]; A.G.plo[d] = plo[d]; A.G.phi[d] = phi[d]; }
  *errFlag = 0;
  if (computeVec) {
    const long long n = (long long)(g->hi[0] - g->lo[0] + 1) * (g->hi[1] - g->lo[1] + 1) * (g->hi[2] - g->lo[2] + 1);
    hipLaunchKernelGGL(k_sg_grad, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, A.T, A.V.F, g->p);
  }
  if (n_ids <= 0) return pa_sync(ctx);
  int* df = nullptr;
  PA_HIP(hipMalloc(&df, 2 * sizeof(int)));
  const int init[2] = {0, 0x7fffffff};
  int hf[2] = {0, 0}, rc = 0;
  if (hipMemcpyAsync(df, init, sizeof init, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = pa_fail(ctx, "pa_vtrace_fab: copy failed");
  if (rc == 0) {
    hipLaunchKernelGGL(k_sg_fab, dim3((unsigned)((2LL * n_ids + 255) / 256)), dim3(256), 0, ctx->stream, A, ids, (long long)nloc, loc, df);
    if (hipGetLastError() != hipSuccess) rc = pa_fail(ctx, "pa_vtrace_fab: launch failed");
  }
  if (rc == 0 && (hipMemcpyAsync(hf, df, sizeof hf, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
    rc = pa_fail(ctx, "pa_vtrace_fab: synchronisation failed");
  (void)hipFree(df);
  if (rc == 0) *errFlag = hf[1] != 0x7fffffff ? 1 : sg_final_flag(hf[0], 0);
  return rc;
}
