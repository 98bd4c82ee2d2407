// pa_streamalt.hip -- the alternate surface of PeleAnalysis Src/stream.cpp (buildAltSurf) on gfx950: where every traced line meets a
// second value of the progress variable (build_surface_at_isoVal :1841-2074), the distance along the line to it, the thermal
// thickness (add_thermal_thickness_to_surf :1554-1838), the cold-side strain (add_cold_strain_to_surf :1369-1552) and the cosine
// of the line's angle to the vertical (add_angle_to_surf :1211-1367; the caller takes the acos).
// Layout: the trace's own buffer -- box g of all levels at box_start[g] * nRKsteps * ncs doubles, component outermost, then j, the
// line in the box fastest (pa_streamgrad_trace) -- and the 1-based node id of every line.  One launch for all boxes, a thread per
// line: adjacent lanes are adjacent lines of a box, so every (component, j) load of a wavefront is one contiguous run.
// Two marches in increasing j.  The first locates every query (alt, thickLo, thickHi, T): the reference's scan
//     for (j = lo; j < hi && !found; ++j) { rIdx = lIdx + 1; rVal = v(rIdx); if (val >= lVal && val < rVal) found; else lIdx = rIdx, lVal = rVal; }
// runs behind a `found` flag for all lanes (they differ anyway), each distinct query component is read once, and the three-way
// choice around it (val > v(hi); val > v(lo); neither) is taken after the march, when v(hi) has been read.  The second forms each
// segment length once and adds it to every query's distance with that query's weight; both of the reference's distance loops run
// in increasing j from 0.0, so the sums keep their serial order.  The carried components are read at the two located points only.
// NUMERICS: every expression keeps the reference's association (-ffp-contract=off) and every comparison its form, so that a NaN
// makes each one false as it does there; add, multiply, divide and sqrt are IEEE: the results are the serial code's bits.  A thread
// owns a line and a node: no atomics on the results.
#include "pa_internal.h"

#define PA_SA_MAXQ 4      // alt, thickLo, thickHi, T
#define PA_SA_MAXU 3      // distinct components among them
#define PA_SA_MAXCARRY 8  // components carried to the located point of the alt query

namespace {

struct SaArgs {
  const long long* bstart;  // device CSR [nbox + 1]
  const int* ids;
  const double* strm;
  long long nlines, nNodes;
  int nbox, ncs, nRKsteps;
  int nq, nu;
  int ucomp[PA_SA_MAXU];  // the distinct query components
  int qu[PA_SA_MAXQ];     // query -> index in ucomp
  double qval[PA_SA_MAXQ];
  int ncarry, carry[PA_SA_MAXCARRY];
  int strainComp, angle;
  double* out;          // [nout][nNodes]
  signed char* branch;  // [nq][nNodes] or null
};

__global__ __launch_bounds__(256) void k_sa_check_ids(const int* __restrict__ ids, long long nlines, long long nNodes, int* bad) {
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= nlines) return;
  const int id = ids[t];
  if (id < 1 || id > nNodes) atomicOr(bad, 1);
}

template <int NU>
__device__ __forceinline__ double sa_pick(const double (&v)[NU], int u) {
  double r = v[0];
#pragma unroll
  for (int k = 1; k < NU; ++k) r = (u == k ? v[k] : r);
  return r;
}

// NU distinct query components, NQ queries: 1 alt; 2 alt, T; 3 alt, thickLo, thickHi; 4 alt, thickLo, thickHi, T.  Compile-time counts
// leave the marches without a branch, so that the loads of several points are in flight at once (a line is a chain of 2 * nRKsteps
// dependent-looking steps otherwise, and a surface has too few lines to hide that behind other waves).
template <int NU, int NQ>
__global__ __launch_bounds__(256) void k_sa_lines(SaArgs a) {
  constexpr bool THICK = NQ >= 3, HAS_T = NQ == 2 || NQ == 4;
  const long long line = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (line >= a.nlines) return;
  int blo = 0, bhi = a.nbox;  // box g with bstart[g] <= line < bstart[g+1]
  while (bhi - blo > 1) {
    const int mid = (blo + bhi) >> 1;
    if (a.bstart[mid] <= line) blo = mid; else bhi = mid;
  }
  const long long b0 = a.bstart[blo], nj = a.bstart[blo + 1] - b0, i = line - b0;
  const int nRKh = (a.nRKsteps - 1) / 2, lo = -nRKh, hi = a.nRKsteps - 1 - nRKh;
  const double* __restrict__ seg = a.strm + b0 * (long long)a.nRKsteps * a.ncs + i;
  const long long plane = nj * a.nRKsteps;
  auto at = [=](int c, int j) -> double { return seg[(long long)c * plane + (long long)(j + nRKh) * nj]; };

  // ---- first march: locate (:1894-1927)
  double vlo[NU], vj[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) vlo[u] = vj[u] = at(a.ucomp[u], lo);
  int lIdx[NQ], rIdx[NQ];
  double lVal[NQ], rVal[NQ], frac[NQ];
  bool found[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    lIdx[q] = lo;
    rIdx[q] = lo + 1;
    lVal[q] = rVal[q] = sa_pick<NU>(vlo, a.qu[q]);
    found[q] = false;
  }
#pragma unroll 4
  for (int j = lo; j < hi; ++j) {
#pragma unroll
    for (int u = 0; u < NU; ++u) vj[u] = at(a.ucomp[u], j + 1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const double val = a.qval[q], v = sa_pick<NU>(vj, a.qu[q]);
      const bool act = !found[q];
      rIdx[q] = act ? j + 1 : rIdx[q];
      rVal[q] = act ? v : rVal[q];
      const bool hit = act && (val >= lVal[q]) && (val < rVal[q]);
      const bool mv = act && !hit;
      found[q] = found[q] || hit;
      lIdx[q] = mv ? j + 1 : lIdx[q];
      lVal[q] = mv ? v : lVal[q];
    }
  }
  // vj holds v(hi) now
  const long long idx = a.ids[line] - 1;
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double val = a.qval[q];
    int code;
    if (val > sa_pick<NU>(vj, a.qu[q])) {
      lIdx[q] = hi - 1;
      rIdx[q] = hi;
      frac[q] = 1.0;
      code = 3;
    } else if (val > sa_pick<NU>(vlo, a.qu[q])) {
      frac[q] = (rVal[q] == lVal[q] ? 0.0 : (val - lVal[q]) / (rVal[q] - lVal[q]));
      code = found[q] ? 1 : 2;
    } else {
      lIdx[q] = lo;
      rIdx[q] = lo + 1;
      frac[q] = 0.0;
      code = 0;
    }
    if (a.branch) a.branch[(long long)q * a.nNodes + idx] = (signed char)code;
  }

  // ---- second march: the distance from j = 0 to every located point (:1944-1972)
  double dist[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) dist[q] = 0;
  double xL[3], xR[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) xR[d] = at(d, lo);
#pragma unroll 4
  for (int j = lo; j < hi; ++j) {
    double dd = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      xL[d] = xR[d];
      xR[d] = at(d, j + 1);
      dd += (xR[d] - xL[d]) * (xR[d] - xL[d]);
    }
    const double s = sqrt(dd);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      if (lIdx[q] < 0) {
        if (j >= lIdx[q] && j < 0) dist[q] -= (j == lIdx[q] ? (1. - frac[q]) : 1.0) * s;
      } else {
        if (j >= 0 && j < rIdx[q]) dist[q] += (j == rIdx[q] - 1 ? frac[q] : 1.0) * s;
      }
    }
  }

  // ---- the node's components (:1929-1942, :1973, :1737, :1448-1451, :1255-1265)
  auto lerp = [&](int c, int l, int r, double f) -> double {
    const double L = at(c, l), R = at(c, r);
    return L + (R - L) * f;
  };
  int oc = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) a.out[(long long)(oc++) * a.nNodes + idx] = lerp(d, lIdx[0], rIdx[0], frac[0]);
  for (int k = 0; k < a.ncarry; ++k) a.out[(long long)(oc++) * a.nNodes + idx] = lerp(a.carry[k], lIdx[0], rIdx[0], frac[0]);
  a.out[(long long)(oc++) * a.nNodes + idx] = dist[0];
  if constexpr (THICK) a.out[(long long)(oc++) * a.nNodes + idx] = dist[2] - dist[1];  // hiLoc - loLoc
  if constexpr (HAS_T) a.out[(long long)(oc++) * a.nNodes + idx] = lerp(a.strainComp, lIdx[NQ - 1], rIdx[NQ - 1], frac[NQ - 1]);
  if (a.angle) {
    const int h = (int)(0.5 * (lo + hi));
    double mag = 0, dx[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      dx[d] = at(d, h - 1) - at(d, h + 1);
      mag += dx[d] * dx[d];
    }
    mag = sqrt(mag);
    a.out[(long long)(oc++) * a.nNodes + idx] = dx[2] / mag;
  }
}

template <int NU, int NQ>
void sa_launch(pa_ctx* ctx, unsigned gx, const SaArgs& a) {
  hipLaunchKernelGGL((k_sa_lines<NU, NQ>), dim3(gx), dim3(256), 0, ctx->stream, a);
}

}  // namespace

extern "C" int pa_streamalt_run(pa_ctx* ctx, int32_t nbox, const int64_t* box_start, const int32_t* ids, const double* strm, int32_t ncs, int32_t nRKsteps,
                                int64_t nNodes, const pa_streamalt_params* p, double* out, int8_t* branch) {
  PaBind bind_(ctx);
  if (!ctx || nbox < 1 || !box_start || !p || nNodes < 0) return pa_fail(ctx, "pa_streamalt_run: bad argument");
  if (nRKsteps < 3) return pa_fail(ctx, "pa_streamalt_run: nRKsteps must be at least 3 (the search and the angle index j = -1 .. 1)");
  auto comp_ok = [ncs](int c) { return c >= 0 && c < ncs; };
  if (ncs < 4 || !comp_ok(p->isoComp)) return pa_fail(ctx, "pa_streamalt_run: progress component out of range");
  if (p->ncarry < 0 || p->ncarry > PA_SA_MAXCARRY) return pa_fail(ctx, "pa_streamalt_run: more than 8 carried components");
  for (int k = 0; k < p->ncarry; ++k)
    if (!comp_ok(p->carry[k])) return pa_fail(ctx, "pa_streamalt_run: carried component out of range");
  if (p->thickComp >= ncs) return pa_fail(ctx, "pa_streamalt_run: thickness component out of range");
  if (p->TComp >= ncs) return pa_fail(ctx, "pa_streamalt_run: T component out of range");
  if (p->TComp >= 0 && !comp_ok(p->strainComp)) return pa_fail(ctx, "pa_streamalt_run: strain component out of range");
  if (box_start[0] != 0) return pa_fail(ctx, "pa_streamalt_run: box_start[0] must be 0");
  for (int g = 0; g < nbox; ++g)
    if (box_start[g + 1] < box_start[g]) return pa_fail(ctx, "pa_streamalt_run: box_start is not ascending");
  const long long nlines = box_start[nbox];
  if (nlines == 0) return 0;
  if (!ids || !strm || !out) return pa_fail(ctx, "pa_streamalt_run: null device array");

  SaArgs a{};
  a.ids = ids;
  a.strm = strm;
  a.nlines = nlines;
  a.nNodes = nNodes;
  a.nbox = nbox;
  a.ncs = ncs;
  a.nRKsteps = nRKsteps;
  auto add_query = [&a](int comp, double val) {
    int u = 0;
    while (u < a.nu && a.ucomp[u] != comp) ++u;
    if (u == a.nu) a.ucomp[a.nu++] = comp;
    a.qu[a.nq] = u;
    a.qval[a.nq] = val;
    return a.nq++;
  };
  add_query(p->isoComp, p->altVal);
  if (p->thickComp >= 0) {
    add_query(p->thickComp, p->thickLo);
    add_query(p->thickComp, p->thickHi);
  }
  if (p->TComp >= 0) add_query(p->TComp, p->TVal);
  a.ncarry = p->ncarry;
  for (int k = 0; k < p->ncarry; ++k) a.carry[k] = p->carry[k];
  a.strainComp = p->TComp >= 0 ? p->strainComp : 0;
  a.angle = p->addAngle ? 1 : 0;
  a.out = out;
  a.branch = (signed char*)branch;

  long long* dstart = nullptr;
  int* dbad = nullptr;
  PA_HIP(hipMalloc(&dstart, sizeof(long long) * (size_t)(nbox + 1)));
  if (hipMalloc(&dbad, sizeof(int)) != hipSuccess) { (void)hipFree(dstart); return pa_fail(ctx, "pa_streamalt_run: device allocation failed"); }
  int rc = 0;
  do {
    int bad = 0;
    const unsigned gx = (unsigned)((nlines + 255) / 256);
    if (hipMemcpyAsync(dstart, box_start, sizeof(long long) * (size_t)(nbox + 1), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemsetAsync(dbad, 0, sizeof(int), ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_streamalt_run: copy failed"); break; }
    hipLaunchKernelGGL(k_sa_check_ids, dim3(gx), dim3(256), 0, ctx->stream, ids, nlines, (long long)nNodes, dbad);
    if (hipGetLastError() != hipSuccess) { rc = pa_fail(ctx, "pa_streamalt_run: launch failed"); break; }
    if (hipMemcpyAsync(&bad, dbad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_streamalt_run: synchronisation failed"); break; }
    if (bad) { rc = pa_fail(ctx, "pa_streamalt_run: a node id outside 1 .. " + std::to_string((long long)nNodes)); break; }  // before any scatter
    a.bstart = dstart;
    switch (10 * a.nq + a.nu) {  // the queries are alt [, thickLo, thickHi] [, T]
      case 11: sa_launch<1, 1>(ctx, gx, a); break;
      case 21: sa_launch<1, 2>(ctx, gx, a); break;
      case 22: sa_launch<2, 2>(ctx, gx, a); break;
      case 31: sa_launch<1, 3>(ctx, gx, a); break;
      case 32: sa_launch<2, 3>(ctx, gx, a); break;
      case 41: sa_launch<1, 4>(ctx, gx, a); break;
      case 42: sa_launch<2, 4>(ctx, gx, a); break;
      default: sa_launch<3, 4>(ctx, gx, a); break;
    }
    if (hipGetLastError() != hipSuccess) { rc = pa_fail(ctx, "pa_streamalt_run: launch failed"); break; }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { rc = pa_fail(ctx, "pa_streamalt_run: synchronisation failed"); break; }
  } while (0);
  (void)hipFree(dstart);
  (void)hipFree(dbad);
  return rc;
}
