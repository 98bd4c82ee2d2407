// pa_streamsample.hip -- sampleStreamlines.cpp / sampleStreamlines_nd.f90 on gfx950 (the sampleStreamlines3d tool): plotfile
// components interpolated at every point of the lines of a streamFile, the points' signed arc length from the seed, X / Y / Z.
//   k_ss_sample:  every point of every (level, Str box) with lines in ONE launch, a thread per point (i fastest, then j: the
//                 stores into the Str layout are coalesced).  ntrpv's b / n (sampleStreamlines_nd.f90:67-72) -- no [plo, phi]
//                 test, unlike stream_nd.f90 -- then the box test against the grown seed box, then the 8 corner cells resolved
//                 ONCE (the per-cell rule below) and reused for the K components.
//   k_ss_xyzd:    X / Y / Z copied fab by fab (set_sample_location, sampleStreamlines.cpp:779-785) and set_distance
//                 (sampleStreamlines_nd.f90:106-146), a thread per line.
//   pa_interpstream_fab / pa_set_distance_fab: one MFIter iteration of sampleStreamlines.cpp:745-748 / :772 on a staged FAB.
// The per-cell rule replaces the staged FAB of sample_pathlines (:671-734): a cell of the level's index domain takes the value of
// the finest level <= lev whose grids hold it (FillVar, piecewise-constant injection); a cell outside it takes its periodic image's
// value when a shift of at most one domain length per periodic direction brings it inside (Geometry::periodicShift), else -20000.
// Gather-bound on reads that mostly hit L2; store-bound at large K.
#include "pa_internal.h"
#include <cmath>
#include <vector>

#define PA_SS_MAXLEV 8

struct SsLevels {
  int nlev, K;
  int is_per[3];
  int boxcum[PA_SS_MAXLEV + 1];  // global Str box numbers of level l: boxcum[l] .. boxcum[l+1]-1
  int ratio[PA_SS_MAXLEV];       // ratio[l]: level l to level l - 1 (l >= 1)
  DLevelView L[PA_SS_MAXLEV];
  DMFView M[PA_SS_MAXLEV];
  double dx[PA_SS_MAXLEV][3], plo[3];
};

// ntrpv up to the sum (sampleStreamlines_nd.f90:67-83): b = FLOOR((x-plo)/dx - 0.5), n clamped to [0, 1]; b in [blo, bhi - 1]
// (the Fortran tests b <= bhi and then reads b + 1: at b == bhi that is outside the FAB -- a failure here)
__device__ __forceinline__ bool ss_locate(const double dx[3], const double plo[3], const double x[3], const int blo[3], const int bhi[3], int b[3],
                                          double n[3]) {
  bool ok = true;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double tmp = (x[d] - plo[d]) / dx[d] - 0.5;
    b[d] = (int)floor(tmp);
    double v = (x[d] - ((b[d] + 0.5) * dx[d] + plo[d])) / dx[d];
    v = (v < 1.0) ? v : 1.0;    // MIN(1.d0, n)
    n[d] = (0.0 < v) ? v : 0.0;  // MAX(0.d0, .)
    ok = ok && b[d] >= blo[d] && b[d] <= bhi[d] - 1;
  }
  return ok;
}

// order of a point in interpstream's loops (:26-53): k outermost, then j = 0, -1, .., lo, then j = 1 .. hi, i innermost
__device__ __forceinline__ unsigned long long ss_rank(int i, int j, int k, const int lo[3], const int hi[3]) {
  const long long ni = hi[0] - lo[0] + 1, nj = hi[1] - lo[1] + 1;
  const long long jr = j <= 0 ? -j : (long long)(-lo[1]) + j;
  return (unsigned long long)((((long long)(k - lo[2]) * nj + jr) * ni) + (i - lo[0]));
}

// the value source of cell p of level lev: base pointer of component 0 and the component stride; null: -20000
__device__ __forceinline__ const double* ss_cell(const SsLevels& S, int lev, const int p0[3], long long& cs) {
  int p[3] = {p0[0], p0[1], p0[2]};
  const DLevelView& L = S.L[lev];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int len = L.domhi[d] - L.domlo[d] + 1;
    if (p[d] < L.domlo[d]) {
      if (!S.is_per[d]) return nullptr;
      p[d] += len;
    } else if (p[d] > L.domhi[d]) {
      if (!S.is_per[d]) return nullptr;
      p[d] -= len;
    }
    if (p[d] < L.domlo[d] || p[d] > L.domhi[d]) return nullptr;  // more than one domain length outside
  }
  for (int l = lev; l >= 0; --l) {
    const int o = owner_of(S.L[l], p);
    if (o >= 0) {
      const DBox& B = S.L[l].boxes[o];
      const DMFView& M = S.M[l];
      cs = pa_cstride((long long)(B.hi[0] - B.lo[0] + 1 + 2 * M.ng) * (B.hi[1] - B.lo[1] + 1 + 2 * M.ng) * (B.hi[2] - B.lo[2] + 1 + 2 * M.ng), M.ncomp);
      return M.data + M.off[o] + fab_index(B, M.ng, M.ncomp, 0, p[0], p[1], p[2]);
    }
    if (l > 0)
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] = coarsen_idx(p[d], S.ratio[l]);
  }
  return nullptr;  // no level holds the cell: FillVar sets nothing, the staged -20000 stays
}

// one thread per point of the boxes with lines; pstart: CSR of those points over the global Str boxes (0 for boxes without lines)
__global__ __launch_bounds__(256) void k_ss_sample(SsLevels S, int nbt, const long long* __restrict__ pstart, const long long* __restrict__ ostart,
                                                   const int* __restrict__ sbox /* [nbt][6] Str boxes */, const int* __restrict__ bbox /* [nbt][6] */,
                                                   const double* __restrict__ xyz, double* __restrict__ out, int ncout, int dcomp,
                                                   unsigned long long* fail) {
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= pstart[nbt]) return;
  int lo = 0, hi = nbt;  // box g with pstart[g] <= q < pstart[g+1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pstart[mid] <= q) lo = mid; else hi = mid;
  }
  const int g = lo;
  int l = 0;
  while (l + 1 < S.nlev && g >= S.boxcum[l + 1]) ++l;
  const long long t = q - pstart[g], np = pstart[g + 1] - pstart[g];
  const double* xs = xyz + 3 * ostart[g];
  const double x[3] = {xs[t], xs[np + t], xs[2 * np + t]};
  const int blo[3] = {bbox[6 * g], bbox[6 * g + 1], bbox[6 * g + 2]}, bhi[3] = {bbox[6 * g + 3], bbox[6 * g + 4], bbox[6 * g + 5]};
  int b[3];
  double n[3];
  if (!ss_locate(S.dx[l], S.plo, x, blo, bhi, b, n)) {
    const int slo[3] = {sbox[6 * g], sbox[6 * g + 1], sbox[6 * g + 2]}, shi[3] = {sbox[6 * g + 3], sbox[6 * g + 4], sbox[6 * g + 5]};
    const long long ni = shi[0] - slo[0] + 1, nj = shi[1] - slo[1] + 1;
    atomicMin(&fail[g], ss_rank(slo[0] + (int)(t % ni), slo[1] + (int)((t / ni) % nj), slo[2] + (int)(t / (ni * nj)), slo, shi));
    return;
  }
  const double* c8[8];
  long long s8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int p[3] = {b[0] + (e & 1), b[1] + ((e >> 1) & 1), b[2] + (e >> 2)};
    s8[e] = 0;
    c8[e] = ss_cell(S, l, p, s8[e]);
  }
  double* o = out + ncout * ostart[g] + (long long)dcomp * np + t;
  for (int m = 0; m < S.K; ++m) {
    o[(long long)m * np] = sg_sum(n, [&](int di, int dj, int dk) {
      const int e = di | (dj << 1) | (dk << 2);
      return c8[e] ? c8[e][(long long)m * s8[e]] : -20000.0;
    });
  }
}

// boxes WITHOUT lines: the sampled components stay 0 (sampledata->setVal(0.), :151); a thread per point of those boxes
__global__ __launch_bounds__(256) void k_ss_zero(int nbt, const long long* __restrict__ zstart, const long long* __restrict__ ostart, double* out, int ncout,
                                                 int dcomp, int K) {
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= zstart[nbt]) return;
  int lo = 0, hi = nbt;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (zstart[mid] <= q) lo = mid; else hi = mid;
  }
  const int g = lo;
  const long long t = q - zstart[g], np = zstart[g + 1] - zstart[g];
  double* o = out + ncout * ostart[g] + (long long)dcomp * np + t;
  for (int m = 0; m < K; ++m) o[(long long)m * np] = 0.0;
}

// set_distance (sampleStreamlines_nd.f90:106-146) for line (i, k) of a FAB of nj x ni points per k (j lo..hi, j = 0 the seed):
// loc(c) / res: element (i, j, k) at [c * cstride] + ((k - klo) * nj + (j - jlo)) * ni + (i - ilo).  res(i, 0, 0) is set to 0
// (k = 0 hard-coded, as the Fortran)
__device__ __forceinline__ void ss_distance(const double* loc, long long lcs, double* res, const int lo[3], const int hi[3], int i, int k) {
  const long long ni = hi[0] - lo[0] + 1, nj = hi[1] - lo[1] + 1;
  auto at = [&](int j, int kk) { return ((long long)(kk - lo[2]) * nj + (j - lo[1])) * ni + (i - lo[0]); };
  double d = 0.0;
  res[at(0, 0)] = d;
  for (int j = -1; j >= lo[1]; --j) {
    const long long a = at(j, k), p = at(j + 1, k);
    const double dx = loc[a] - loc[p], dy = loc[lcs + a] - loc[lcs + p], dz = loc[2 * lcs + a] - loc[2 * lcs + p];
    d = d + sqrt(dx * dx + dy * dy + dz * dz);
    res[a] = -d;
  }
  d = 0.0;
  for (int j = 1; j <= hi[1]; ++j) {
    const long long a = at(j, k), p = at(j - 1, k);
    const double dx = loc[a] - loc[p], dy = loc[lcs + a] - loc[lcs + p], dz = loc[2 * lcs + a] - loc[2 * lcs + p];
    d = d + sqrt(dx * dx + dy * dy + dz * dz);
    res[a] = d;
  }
}

// every Str box (with lines or not): components 0..2 = the path's X / Y / Z, component 3 = distance_from_seed; a thread per (i, k)
__global__ __launch_bounds__(256) void k_ss_xyzd(int nbt, const long long* __restrict__ lstart, const long long* __restrict__ ostart, const int* __restrict__ sbox,
                                                 const double* __restrict__ xyz, double* __restrict__ out, int ncout) {
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= lstart[nbt]) return;
  int lo = 0, hi = nbt;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (lstart[mid] <= q) lo = mid; else hi = mid;
  }
  const int g = lo;
  const int slo[3] = {sbox[6 * g], sbox[6 * g + 1], sbox[6 * g + 2]}, shi[3] = {sbox[6 * g + 3], sbox[6 * g + 4], sbox[6 * g + 5]};
  const long long ni = shi[0] - slo[0] + 1, nj = shi[1] - slo[1] + 1, np = ni * nj * (shi[2] - slo[2] + 1);
  const long long t = q - lstart[g];
  const int i = slo[0] + (int)(t % ni), k = slo[2] + (int)(t / ni);
  const double* xs = xyz + 3 * ostart[g];
  double* o = out + ncout * ostart[g];
  const long long r0 = (long long)(k - slo[2]) * nj * ni + (i - slo[0]);
  for (int c = 0; c < 3; ++c)
    for (long long j = 0; j < nj; ++j) o[c * np + r0 + j * ni] = xs[c * np + r0 + j * ni];
  ss_distance(xs, np, o + 3 * np, slo, shi, i, k);
}

static bool ss_str_box_ok(const int* b) { return b[0] <= b[3] && b[1] <= 0 && 0 <= b[4] && b[2] == 0 && b[5] == 0; }

extern "C" int pa_streamsample_run(pa_ctx* ctx, int nlev, pa_mf* const* data, int32_t K, const double* file_dx, const double plo[3], const int32_t is_per[3],
                                   const int32_t* nbox, const int32_t* str_boxes, const int32_t* has_lines, const int32_t* bbox, const double* xyz, double* out,
                                   int32_t ncout, int32_t dcomp, int32_t with_xyzd, int32_t* box_fail) {
  PaBind bind_(ctx);
  if (!ctx || !data || nlev <= 0 || nlev > PA_SS_MAXLEV || !file_dx || !plo || !is_per || !nbox || !str_boxes || !has_lines || !bbox || !box_fail)
    return pa_fail(ctx, "pa_streamsample_run: bad argument (1 <= nlev <= 8)");
  if (K < 0 || dcomp < 4 || dcomp + K > ncout) return pa_fail(ctx, "pa_streamsample_run: components out of range (4 <= dcomp, dcomp + K <= ncout)");
  SsLevels S{};
  S.nlev = nlev;
  S.K = K;
  for (int d = 0; d < 3; ++d) { S.is_per[d] = is_per[d] ? 1 : 0; S.plo[d] = plo[d]; }
  S.boxcum[0] = 0;
  for (int l = 0; l < nlev; ++l) {
    const pa_mf* m = data[l];
    if (!m || (K > 0 && m->ncomp < K)) return pa_fail(ctx, "pa_streamsample_run: every level needs the K components");
    if (m->lev->nremote > 0) return pa_fail(ctx, "pa_streamsample_run: levels sharded across ranks are not supported");
    if (nbox[l] < 0) return pa_fail(ctx, "pa_streamsample_run: negative box count");
    S.L[l] = m->lev->view;
    S.M[l] = m->view;
    S.boxcum[l + 1] = S.boxcum[l] + nbox[l];
    for (int d = 0; d < 3; ++d) S.dx[l][d] = file_dx[3 * l + d];
    S.ratio[l] = 1;
    if (l > 0) {
      const pa_level *F = m->lev, *C = data[l - 1]->lev;
      for (int d = 0; d < 3; ++d) {
        const int nf = F->domhi[d] - F->domlo[d] + 1, nc = C->domhi[d] - C->domlo[d] + 1;
        const int r = (nc > 0 && nf % nc == 0) ? nf / nc : 0;
        if (r < 2 || (d > 0 && r != S.ratio[l]))
          return pa_fail(ctx, "pa_streamsample_run: the domains of levels " + std::to_string(l - 1) + " and " + std::to_string(l) + " are not related by one integer ratio >= 2");
        S.ratio[l] = r;
      }
    }
  }
  const int nbt = S.boxcum[nlev];
  std::vector<long long> ostart(nbt + 1, 0), pstart(nbt + 1, 0), zstart(nbt + 1, 0), lstart(nbt + 1, 0);
  for (int g = 0; g < nbt; ++g) {
    const int* b = str_boxes + 6 * g;
    if (!ss_str_box_ok(b)) return pa_fail(ctx, "pa_streamsample_run: a Str box is not (ilo, jlo, 0)..(ihi, jhi, 0) with jlo <= 0 <= jhi");
    const long long np = (long long)(b[3] - b[0] + 1) * (b[4] - b[1] + 1);
    ostart[g + 1] = ostart[g] + np;
    pstart[g + 1] = pstart[g] + (has_lines[g] ? np : 0);
    zstart[g + 1] = zstart[g] + (has_lines[g] ? 0 : np);
    lstart[g + 1] = lstart[g] + (b[3] - b[0] + 1);
    box_fail[g] = 0;
  }
  if (ostart[nbt] > 0 && (!xyz || !out)) return pa_fail(ctx, "pa_streamsample_run: null device array");
  if (ostart[nbt] == 0) return 0;
  long long* dst = nullptr;
  int* dbox = nullptr;
  unsigned long long* dfail = nullptr;
  PA_HIP(hipMalloc(&dst, sizeof(long long) * 4 * (size_t)(nbt + 1)));
  if (hipMalloc(&dbox, sizeof(int) * 12 * (size_t)nbt) != hipSuccess || hipMalloc(&dfail, sizeof(unsigned long long) * (size_t)nbt) != hipSuccess) {
    (void)hipFree(dst);
    if (dbox) (void)hipFree(dbox);
    return pa_fail(ctx, "pa_streamsample_run: device allocation failed");
  }
  std::vector<long long> hst;
  for (auto* v : {&ostart, &pstart, &zstart, &lstart}) hst.insert(hst.end(), v->begin(), v->end());
  std::vector<int> hbox(12 * (size_t)nbt);
  std::copy(str_boxes, str_boxes + 6 * (size_t)nbt, hbox.begin());
  std::copy(bbox, bbox + 6 * (size_t)nbt, hbox.begin() + 6 * (size_t)nbt);
  std::vector<unsigned long long> hfail(nbt, ~0ull);
  const long long *d_o = dst, *d_p = dst + (nbt + 1), *d_z = dst + 2 * (nbt + 1), *d_l = dst + 3 * (nbt + 1);
  int rc = 0;
  do {
    if (hipMemcpyAsync(dst, hst.data(), sizeof(long long) * hst.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(dbox, hbox.data(), sizeof(int) * hbox.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(dfail, hfail.data(), sizeof(unsigned long long) * (size_t)nbt, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
      rc = pa_fail(ctx, "pa_streamsample_run: copy failed");
      break;
    }
    if (K > 0 && pstart[nbt] > 0)
      hipLaunchKernelGGL(k_ss_sample, dim3((unsigned)((pstart[nbt] + 255) / 256)), dim3(256), 0, ctx->stream, S, nbt, d_p, d_o, dbox, dbox + 6 * nbt, xyz, out,
                         (int)ncout, (int)dcomp, dfail);
    if (K > 0 && zstart[nbt] > 0)
      hipLaunchKernelGGL(k_ss_zero, dim3((unsigned)((zstart[nbt] + 255) / 256)), dim3(256), 0, ctx->stream, nbt, d_z, d_o, out, (int)ncout, (int)dcomp, (int)K);
    if (with_xyzd)
      hipLaunchKernelGGL(k_ss_xyzd, dim3((unsigned)((lstart[nbt] + 255) / 256)), dim3(256), 0, ctx->stream, nbt, d_l, d_o, dbox, xyz, out, (int)ncout);
    if (hipGetLastError() != hipSuccess) { rc = pa_fail(ctx, "pa_streamsample_run: launch failed"); break; }
    if (hipMemcpyAsync(hfail.data(), dfail, sizeof(unsigned long long) * (size_t)nbt, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_streamsample_run: synchronisation failed"); break; }
    for (int g = 0; g < nbt; ++g) {
      if (hfail[g] == ~0ull) continue;
      const int* b = str_boxes + 6 * g;
      const long long ni = b[3] - b[0] + 1, jr = (long long)(hfail[g] / (unsigned long long)ni) % (b[4] - b[1] + 1);
      box_fail[g] = jr == 0 ? 1 : 2;  // j = 0 first in the Fortran's order: the seed
    }
  } while (0);
  (void)hipFree(dst);
  (void)hipFree(dbox);
  (void)hipFree(dfail);
  return rc;
}

// ------------------------------------------------------------------------------------------------ one FAB (:745-748, :772)
struct SsFab {
  const double* p;
  int lo[3], hi[3];
  long long cs;
};

static bool ss_fab_of(const pa_fab* f, SsFab& s) {
  if (!f || !f->p) return false;
  s.p = f->p;
  for (int d = 0; d < 3; ++d) { s.lo[d] = f->lo[d]; s.hi[d] = f->hi[d]; if (s.hi[d] < s.lo[d]) return false; }
  s.cs = f->nstride;
  return true;
}

// interpstream: a thread per point of loc's box; fab: the staged data (np components), strm: np components on loc's box
__global__ __launch_bounds__(256) void k_ss_fab(SsFab loc, SsFab fab, SsFab strm, int np, SsLevels G, unsigned long long* fail) {
  const long long ni = loc.hi[0] - loc.lo[0] + 1, nj = loc.hi[1] - loc.lo[1] + 1, nk = loc.hi[2] - loc.lo[2] + 1;
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= ni * nj * nk) return;
  const int i = loc.lo[0] + (int)(q % ni), j = loc.lo[1] + (int)((q / ni) % nj), k = loc.lo[2] + (int)(q / (ni * nj));
  const double x[3] = {loc.p[q], loc.p[loc.cs + q], loc.p[2 * loc.cs + q]};
  int b[3];
  double n[3];
  if (!ss_locate(G.dx[0], G.plo, x, fab.lo, fab.hi, b, n)) {
    atomicMin(fail, ss_rank(i, j, k, loc.lo, loc.hi));
    return;
  }
  const long long fx = fab.hi[0] - fab.lo[0] + 1, fxy = fx * (fab.hi[1] - fab.lo[1] + 1);
  const double* base = fab.p + (long long)(b[2] - fab.lo[2]) * fxy + (long long)(b[1] - fab.lo[1]) * fx + (b[0] - fab.lo[0]);
  double* o = const_cast<double*>(strm.p) + q;
  for (int m = 0; m < np; ++m) {
    const double* c = base + (long long)m * fab.cs;
    o[(long long)m * strm.cs] = sg_sum(n, [&](int di, int dj, int dk) { return c[di + dj * fx + dk * fxy]; });
  }
}

extern "C" int pa_interpstream_fab(pa_ctx* ctx, const pa_fab* loc, int32_t nl, const pa_fab* fab, int32_t np, pa_fab* strm, const double dx[3],
                                   const double plo[3], int32_t* status) {
  PaBind bind_(ctx);
  SsFab L{}, F{}, O{};
  if (!ctx || !dx || !plo || !status || !ss_fab_of(loc, L) || !ss_fab_of(fab, F) || !ss_fab_of(strm, O)) return pa_fail(ctx, "pa_interpstream_fab: bad argument");
  if (nl < 3 || nl > loc->ncomp || np < 1 || np > fab->ncomp || np > strm->ncomp) return pa_fail(ctx, "pa_interpstream_fab: component counts (nl >= 3)");
  for (int d = 0; d < 3; ++d)
    if (L.lo[d] != O.lo[d] || L.hi[d] != O.hi[d]) return pa_fail(ctx, "pa_interpstream_fab: strm must be on loc's box");
  if (L.lo[1] > 0 || L.hi[1] < 0) return pa_fail(ctx, "pa_interpstream_fab: loc's box must hold j = 0 (the seeds)");
  const long long n = (long long)(L.hi[0] - L.lo[0] + 1) * (L.hi[1] - L.lo[1] + 1) * (L.hi[2] - L.lo[2] + 1);
  if (L.cs < n || O.cs < n) return pa_fail(ctx, "pa_interpstream_fab: loc / strm component strides must hold the box (dense FABs)");
  SsLevels G{};
  for (int d = 0; d < 3; ++d) { G.dx[0][d] = dx[d]; G.plo[d] = plo[d]; }
  *status = 0;
  unsigned long long* df = nullptr;
  PA_HIP(hipMalloc(&df, sizeof(unsigned long long)));
  unsigned long long hf = ~0ull;
  int rc = 0;
  if (hipMemcpyAsync(df, &hf, sizeof hf, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = pa_fail(ctx, "pa_interpstream_fab: copy failed");
  if (rc == 0) {
    hipLaunchKernelGGL(k_ss_fab, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, L, F, O, (int)np, G, df);
    if (hipGetLastError() != hipSuccess) rc = pa_fail(ctx, "pa_interpstream_fab: launch failed");
  }
  if (rc == 0 && (hipMemcpyAsync(&hf, df, sizeof hf, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess))
    rc = pa_fail(ctx, "pa_interpstream_fab: synchronisation failed");
  (void)hipFree(df);
  if (rc == 0 && hf != ~0ull) {
    const long long ni = L.hi[0] - L.lo[0] + 1, nj = L.hi[1] - L.lo[1] + 1;
    *status = ((long long)(hf / (unsigned long long)ni) % nj) == 0 ? 1 : 2;
  }
  (void)nl;
  return rc;
}

__global__ __launch_bounds__(256) void k_ss_dist_fab(SsFab loc, SsFab res) {
  const long long ni = loc.hi[0] - loc.lo[0] + 1, nk = loc.hi[2] - loc.lo[2] + 1;
  const long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (q >= ni * nk) return;
  ss_distance(loc.p, loc.cs, const_cast<double*>(res.p), loc.lo, loc.hi, loc.lo[0] + (int)(q % ni), loc.lo[2] + (int)(q / ni));
}

extern "C" int pa_set_distance_fab(pa_ctx* ctx, const pa_fab* loc, pa_fab* res) {
  PaBind bind_(ctx);
  SsFab L{}, R{};
  if (!ctx || !ss_fab_of(loc, L) || !ss_fab_of(res, R) || loc->ncomp < 3) return pa_fail(ctx, "pa_set_distance_fab: bad argument");
  for (int d = 0; d < 3; ++d)
    if (L.lo[d] != R.lo[d] || L.hi[d] != R.hi[d]) return pa_fail(ctx, "pa_set_distance_fab: res must be on loc's box");
  if (L.lo[1] > 0 || L.hi[1] < 0 || L.lo[2] > 0 || L.hi[2] < 0) return pa_fail(ctx, "pa_set_distance_fab: the box must hold j = 0 and k = 0 (res(i,0,0) is set)");
  const long long n = (long long)(L.hi[0] - L.lo[0] + 1) * (L.hi[1] - L.lo[1] + 1) * (L.hi[2] - L.lo[2] + 1);
  if (L.cs < n) return pa_fail(ctx, "pa_set_distance_fab: loc's component stride must hold the box (dense FAB)");
  const long long nl = (long long)(L.hi[0] - L.lo[0] + 1) * (L.hi[2] - L.lo[2] + 1);
  hipLaunchKernelGGL(k_ss_dist_fab, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, ctx->stream, L, R);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_set_distance_fab: launch failed");
  return pa_sync(ctx);
}

extern "C" int pa_device_mem_info(pa_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes) {
  PaBind bind_(ctx);
  size_t f = 0, t = 0;
  if (!ctx || !free_bytes || !total_bytes) return pa_fail(ctx, "pa_device_mem_info: bad argument");
  PA_HIP(hipMemGetInfo(&f, &t));
  *free_bytes = (int64_t)f;
  *total_bytes = (int64_t)t;
  return 0;
}
