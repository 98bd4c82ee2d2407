// pa_filter.hip -- filterPlt hot path on gfx950: PelePhysics Filter (box) applied per FAB
// (filterPlt.cpp:206-219) and the ghost-cell fill around it (filterPlt.cpp:174-203:
// FillPatchSingleLevel / FillPatchTwoLevels + first-order extrapolation at walls).
//
// apply_filter keeps the reference's summation order (n = z outermost, l = x innermost,
// ((w_l*w_m)*w_n)*q added term by term) so results are bit-identical to the oracle; the
// (2ng+1)^3 taps are served from an LDS tile with an ng-deep halo.
#include "pa_internal.h"
#include "pa_dist.h"
#include "pa_fabview.h"
#include "pa_cclin.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <type_traits>

extern "C" int pa_box_filter_weights(int fgr, double* w) {
  // PelePhysics Filter::set_box_weights restated
  if (fgr < 1 || !w) return -1;
  const int ng = fgr / 2, nw = 2 * ng + 1;
  for (int i = 0; i < nw; ++i) w[i] = 1.0 / (double)fgr;
  if (nw > 1) { w[0] = 0.5 * w[0]; w[nw - 1] = w[0]; }
  return ng;
}

// The other PelePhysics filter types whose weights are closed-form polynomials of the filter-to-grid ratio (filterPlt.cpp:80
// `filter_type`, PelePhysics Filter.H).  [RECALLED / re-derived -- the PelePhysics source is not in the reference
// tree: parity unpinned.]  0 none; 1 box; 3 and 7: the 3-point approximation of the box / Gaussian filter (the same weights:
// both match the second moment fgr^2/12, Sagaut & Grohens 1999); 4 and 8: the 5-point approximations (second moment fgr^2/12
// and fourth moment fgr^4/80 (box) or fgr^4/48 (Gaussian of the same variance)).  Every weight is ONE division of an
// exactly representable integer expression, so any algebraically equal way of writing it gives the same double.  2: the
// Gaussian from its textbook kernel (unverified, see below).  The "optimized" variants (5, 6, 9, 10: tabulated coefficients)
// are not restated: -1.  w must hold 2 * ngrow + 1 doubles: up to 33 (Gaussian, ngrow = ceil(4 fgr / sqrt 12) <= 16).
extern "C" int pa_filter_weights(int type, int fgr, double* w) {
  if (!w || fgr < 1) return -1;
  const double f2 = (double)fgr * (double)fgr, f4 = f2 * f2;
  switch (type) {
    case 0: w[0] = 1.0; return 0;
    case 1: return pa_box_filter_weights(fgr, w);
    case 2: {
      // REFUSED unless the caller opts in (PA_ALLOW_UNVERIFIED_GAUSSIAN=1 in the environment, read per call; filterPlt:
      // allow_unverified_gaussian=1): these weights are a guess at PelePhysics' and a plotfile filtered with them may differ from
      // the reference's at 1e-6 .. 1e-5 without any other sign (advisor finding, round 4).
      {
        if (!pa_opt().allow_unverified_gaussian) return -1;
      }
      // Gaussian (PelePhysics filter_type 2) [UNVERIFIED against PelePhysics: its source is not in the reference tree].  The textbook
      // LES Gaussian of width Delta = fgr dx, G(r) = sqrt(6 / (pi Delta^2)) exp(-6 r^2 / Delta^2) (variance Delta^2 / 12, the box
      // filter's), sampled at the cell centres, cut at 4 standard deviations and normalised so that the weights sum to one
      const int ng = std::max(1, (int)std::ceil(4.0 * (double)fgr / std::sqrt(12.0)));
      if (ng > 16) return -1;
      double sum = 0.0;
      for (int i = -ng; i <= ng; ++i) { w[i + ng] = std::exp(-6.0 * (double)(i * i) / f2); sum += w[i + ng]; }
      for (int i = 0; i <= 2 * ng; ++i) w[i] = w[i] / sum;
      return ng;
    }
    case 3: case 7:
      w[0] = f2 / 24.0; w[1] = (12.0 - f2) / 12.0; w[2] = w[0];
      return 1;
    case 4:
      w[0] = (3.0 * f4 - 20.0 * f2) / 5760.0; w[1] = (80.0 * f2 - 3.0 * f4) / 1440.0; w[2] = (3.0 * f4 - 100.0 * f2 + 960.0) / 960.0;
      w[3] = w[1]; w[4] = w[0];
      return 2;
    case 8:
      w[0] = (f4 - 4.0 * f2) / 1152.0; w[1] = (16.0 * f2 - f4) / 288.0; w[2] = (f4 - 20.0 * f2 + 192.0) / 192.0;
      w[3] = w[1]; w[4] = w[0];
      return 2;
    default: return -1;
  }
}

struct FilterW { double w[33]; };  // up to ng = 16

// tile of TX x TY x TZ outputs per 256-thread workgroup; thread = (x, y) column, loops over z
template <typename BP, int NG, int TX, int TY, int TZ>
__global__ __launch_bounds__(256) void k_boxfilter(BP bp, int scomp, int ncomp, FilterW W) {
  constexpr int LX = TX + 2 * NG, LY = TY + 2 * NG, LZ = TZ + 2 * NG, NW = 2 * NG + 1;
  static_assert(TX * TY == 256, "one thread per (x,y) column");
  __shared__ double s_in[LZ][LY][LX];
  __shared__ double s_wlm[NW][NW];  // w[l]*w[m], index [m][l]
  FabView I, O;
  DBox V;
  double dxinv[3];
  if (!bp.get(blockIdx.y, I, O, V, dxinv)) return;
  const int nx = V.hi[0] - V.lo[0] + 1, ny = V.hi[1] - V.lo[1] + 1, nz = V.hi[2] - V.lo[2] + 1;
  const int tx = (nx + TX - 1) / TX, ty = (ny + TY - 1) / TY, tz = (nz + TZ - 1) / TZ;
  const unsigned bid = blockIdx.x;
  if (bid >= (unsigned)tx * ty * tz) return;
  const int i0 = V.lo[0] + (bid % tx) * TX, j0 = V.lo[1] + ((bid / tx) % ty) * TY, k0 = V.lo[2] + (bid / (tx * ty)) * TZ;
  const int t = threadIdx.x;
  if (t < NW * NW) s_wlm[t / NW][t % NW] = W.w[t % NW] * W.w[t / NW];
  const int li = t % TX, lj = t / TX;
  for (int c = scomp; c < scomp + ncomp; ++c) {
    __syncthreads();
    // stage the tile + halo; positions past the box + ng are clamped (their values are never used)
    for (int q = t; q < LZ * LY * LX; q += 256) {
      const int x = q % LX, y = (q / LX) % LY, z = q / (LX * LY);
      const int gi = min(i0 - NG + x, V.hi[0] + NG), gj = min(j0 - NG + y, V.hi[1] + NG), gk = min(k0 - NG + z, V.hi[2] + NG);
      s_in[z][y][x] = I(gi, gj, gk, c);
    }
    __syncthreads();
    const int i = i0 + li, j = j0 + lj;
    if (i <= V.hi[0] && j <= V.hi[1]) {
      for (int kk = 0; kk < TZ && k0 + kk <= V.hi[2]; ++kk) {
        double acc = 0.0;
        for (int n = 0; n < NW; ++n) {
          const double wn = W.w[n];
          for (int m = 0; m < NW; ++m)
#pragma unroll
            for (int l = 0; l < NW; ++l) acc += (s_wlm[m][l] * wn) * s_in[kk + n][lj + m][li + l];
        }
        O(i, j, k0 + kk, c) = acc;
      }
    }
  }
}

// Box weights, streaming form.  PelePhysics' box filter has w = (f/2, f, ..., f, f/2) with f = 1/fgr, so every
// tap weight ((w_l*w_m)*w_n) is c3 = (f*f)*f times an exact power of two 2^-e (e = how many of l, m, n are end
// indices), and the tap ((w_l*w_m)*w_n)*q = 2^-e * RN(c3*q) exactly: scaling by a power of two commutes with
// rounding.  The reference's accumulation order of ONE output is n (z) outermost, then m (y), then l (x); an
// output therefore consumes the input planes in ascending order, and the outputs k-NG..k+NG that share input
// plane k can be advanced together without changing any output's own order.  Thread = (x,y) column with a
// window of 2NG+1 running sums (output planes in flight, slot = plane mod (2NG+1), compile-time after unrolling
// the plane loop by the window length); each input plane is staged ONCE in LDS (double-buffered, prefetched
// through registers) and each staged value is read once per row and reused for the 2NG+1 outputs of the
// window: 1/(2NG+1) LDS reads and 1 + 3/(2NG+1) fp64 instructions per tap instead of 2 and 2.  Bit-identical
// to k_boxfilter / the oracle (except where c3*q is denormal, < 1e-307).
template <typename BP, int NG>
__global__ __launch_bounds__(256) void k_boxfilter_stream(BP bp, int scomp, int ncomp, double f, int kseg) {
  constexpr int TX = 32, TY = 8, LX = TX + 2 * NG, LY = TY + 2 * NG, NW = 2 * NG + 1, NLD = (LX * LY + 255) / 256;
  __shared__ double s_in[2][LY][LX];
  FabView I, O;
  DBox V;
  double dxinv[3];
  if (!bp.get(blockIdx.y, I, O, V, dxinv)) return;
  const int nx = V.hi[0] - V.lo[0] + 1, ny = V.hi[1] - V.lo[1] + 1, nz = V.hi[2] - V.lo[2] + 1;
  const int tx = (nx + TX - 1) / TX, ty = (ny + TY - 1) / TY, tz = (nz + kseg - 1) / kseg;
  const unsigned bid = blockIdx.x;
  if (bid >= (unsigned)tx * ty * tz) return;
  const int i0 = V.lo[0] + (bid % tx) * TX, j0 = V.lo[1] + ((bid / tx) % ty) * TY, k0 = V.lo[2] + (bid / (tx * ty)) * kseg;
  const int k1 = min(k0 + kseg - 1, V.hi[2]);
  const int t = threadIdx.x, li = t % TX, lj = t / TX;
  const int i = i0 + li, j = j0 + lj;
  const bool live = i <= V.hi[0] && j <= V.hi[1];
  const double c3 = (f * f) * f;
  const int nq = k1 - k0 + 1 + 2 * NG;  // input planes k0-NG .. k1+NG
  for (int c = scomp; c < scomp + ncomp; ++c) {
    double acc[NW], pre[NLD];
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[q] = 0.0;
    auto fetch = [&](int q) {  // plane q of the segment into registers (positions past the box + NG are clamped, never used)
      const int gk = k0 - NG + q;
#pragma unroll
      for (int r = 0; r < NLD; ++r) {
        const int e = min(t + 256 * r, LX * LY - 1);
        const int x = e % LX, y = e / LX;
        pre[r] = I(min(i0 - NG + x, V.hi[0] + NG), min(j0 - NG + y, V.hi[1] + NG), gk, c);
      }
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int r = 0; r < NLD; ++r) {
        const int e = t + 256 * r;
        if (e < LX * LY) s_in[buf][e / LX][e % LX] = pre[r];
      }
    };
    __syncthreads();  // the previous component's readers are done with both buffers
    fetch(0);
    stage(0);
    __syncthreads();
    auto step = [&](auto zzc, int q) __attribute__((always_inline)) {
      constexpr int ZZ = decltype(zzc)::value;
      const int buf = q & 1;
      if (q + 1 < nq) fetch(q + 1);
#pragma unroll 1
      for (int m = 0; m < NW; ++m) {
        const double c3m = (m == 0 || m == NW - 1) ? c3 * 0.5 : c3;  // exact scaling
        double p[NW], h[NW];
#pragma unroll
        for (int l = 0; l < NW; ++l) {
          p[l] = c3m * s_in[buf][lj + m][li + l];
          if (l == 0 || l == NW - 1) p[l] = p[l] * 0.5;
          h[l] = p[l] * 0.5;
        }
#pragma unroll
        for (int d = 0; d < NW; ++d) {  // output a = q - d sees this plane as its n = d
          constexpr int dummy = 0;
          (void)dummy;
          const int slot = ((ZZ - d) % NW + NW) % NW;
#pragma unroll
          for (int l = 0; l < NW; ++l) acc[slot] += (d == 0 || d == NW - 1) ? h[l] : p[l];
        }
      }
      {  // the output whose last plane (n = 2NG) this was
        constexpr int slot = ((ZZ - 2 * NG) % NW + NW) % NW;
        const int a = q - 2 * NG;
        if (a >= 0 && live) O(i, j, k0 + a, c) = acc[slot];
        acc[slot] = 0.0;
      }
      if (q + 1 < nq) stage(buf ^ 1);
      __syncthreads();
    };
    int q = 0;
    // unrolled by the window length so that the slots are compile-time registers
#define PA_FS(z) if (q < nq) { step(std::integral_constant<int, (z)>{}, q); ++q; }
    while (q < nq) {
      PA_FS(0) PA_FS(1) PA_FS(2)
      if (NW > 3) { PA_FS(3 % NW) PA_FS(4 % NW) }
      if (NW > 5) { PA_FS(5 % NW) PA_FS(6 % NW) PA_FS(7 % NW) PA_FS(8 % NW) }
    }
#undef PA_FS
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Separable form (the default; PA_FILTER_EXACT=1 keeps the tap-order kernels above).  The filter is a tensor product,
// out = W_z (W_x (W_y in)), and SURVEY 7.3 / north_star grant 1e-12 relative: three 1-D passes of 2NG+1 taps instead of
// (2NG+1)^3 taps in the reference's order -- the result differs from the tap-order sum by a few ulp (tested to
// 1e-12 * Linf against the oracle; cell by cell within gamma_(4NG+6) * sum |w w w| |q| of the exact sum, and bit for bit equal
// to the operation order written out below: tests/filter_ref.py sep_bound / sep_model, which must change with it), and the
// kernel is bound by HBM (16 B/cell) instead of fp64 issue.
// One z-marching kernel, 512 or 1024 threads: a workgroup owns a strip of TY whole rows of a box (rows of a FAB are contiguous
// in memory, so a strip + halo is read as one flat, fully coalesced piece; the only re-read is the 2NG halo rows shared
// with the neighbouring strip, which runs on the same XCD at the same time) and walks kseg + 2NG input planes:
//   stage   plane q+1 is requested into registers before the passes of plane q and parked in LDS A[(q+1)&1] after them
//   y-pass  LDS A -> LDS B: a thread makes 4 consecutive rows of one column from 2NG+4 reads (lanes along x: no conflicts)
//   x-pass  LDS B -> registers: a thread owns pairs of x-adjacent columns, NG+1 16-byte reads for both
//   z-pass  a register window of 2NG+1 running sums per column (slot = output plane mod window, compile-time after
//           unrolling the plane loop by the window length); the output whose last plane this was leaves as a 16-byte store
// Two barriers per plane.  Block numbering keeps all tiles of a box on one XCD (L = 8 (T g + t) + q <-> tile t of box 8g+q).
template <typename BP, int NG, int NT, int NIT>
__global__ __launch_bounds__(NT) void k_filter_sep(BP bp, int scomp, FilterW W, int TY, int kseg, int nys, int T, int nboxes, int ld_max) {
  constexpr int NW = 2 * NG + 1, NLD = NT == 512 ? 7 : 5;  // staging loads per thread: (TY + 2NG) * nxg <= NLD * NT
  extern __shared__ double s_dyn[];
  const unsigned Lb = blockIdx.x, qx = Lb & 7u, rx = Lb >> 3;
  const int tile = (int)(rx % (unsigned)T), b = (int)(8u * (rx / (unsigned)T) + qx);
  if (b >= nboxes) return;
  FabView I, O;
  DBox V;
  double dxinv[3];
  if (!bp.get(b, I, O, V, dxinv)) return;
  const int c = scomp + (int)blockIdx.y;
  const int nx = V.hi[0] - V.lo[0] + 1, ny = V.hi[1] - V.lo[1] + 1, nz = V.hi[2] - V.lo[2] + 1;
  const int ys = tile % nys, zs = tile / nys;
  if (ys * TY >= ny || zs * kseg >= nz) return;
  const int j0 = V.lo[1] + ys * TY, k0 = V.lo[2] + zs * kseg, k1 = min(k0 + kseg - 1, V.hi[2]);
  const int rows = min(TY, V.hi[1] - j0 + 1);
  const int nxg = nx + 2 * NG, ld = nxg + (nxg & 1), nxh = (nx + 1) >> 1;
  const bool padded = (nxg & 1) != 0;
  double* const A0 = s_dyn;
  double* const Bs = s_dyn + 2 * (TY + 2 * NG) * ld_max;
  const int asz = (TY + 2 * NG) * ld_max;
  const int t = threadIdx.x;
  // staging elements of this thread: e = t + NT r over the (TY + 2NG) x nxg piece, rows clamped into the FAB
  const int nA = (TY + 2 * NG) * nxg;
  int goff[NLD];
#pragma unroll
  for (int r = 0; r < NLD; ++r) {
    const int e = min(t + NT * r, nA - 1);
    const int ry = e / nxg, x = e - ry * nxg;
    const int gj = min(j0 - NG + ry, V.hi[1] + NG);
    goff[r] = (gj - I.lo[1]) * I.nx + (V.lo[0] - NG + x - I.lo[0]);
  }
  const long long pstride = (long long)I.nx * I.ny;
  const double* const ibase = I.p + (long long)c * I.sc + (long long)(k0 - NG - I.lo[2]) * pstride;
  // y-pass items (group of 4 rows, column of the ghosted row), at most 2 per thread
  const int nyi = (TY >> 2) * nxg;
  int yoff[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int e = t + NT * it;
    const int g = e / nxg, xg = e - g * nxg;
    yoff[it] = e < nyi ? (4 * g) * ld + xg : -1;
  }
  // x-pass / z-window items: (row, pair of columns), NIT per thread
  int xoff[NIT], ooff[NIT];
  bool second[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int e = t + NT * it;
    const int y = e / nxh, xp = e - y * nxh;
    const bool ok = y < rows;
    xoff[it] = ok ? y * ld + 2 * xp : -1;
    ooff[it] = (j0 + y - O.lo[1]) * O.nx + (V.lo[0] + 2 * xp - O.lo[0]);
    second[it] = 2 * xp + 1 < nx;
  }
  const long long opstride = (long long)O.nx * O.ny;
  double* const obase = O.p + (long long)c * O.sc + (long long)(k0 - O.lo[2]) * opstride;
  const bool al16 = !(O.nx & 1) && !((V.lo[0] - O.lo[0]) & 1) && !(O.sc & 1) && !((unsigned long long)O.p & 15ull) && !(opstride & 1);
  typedef double d2 __attribute__((ext_vector_type(2)));
  double acc[NIT][2][NW];
#pragma unroll
  for (int it = 0; it < NIT; ++it)
#pragma unroll
    for (int q = 0; q < NW; ++q) acc[it][0][q] = acc[it][1][q] = 0.0;
  double pre[NLD];
  const int nq = k1 - k0 + 1 + 2 * NG;  // input planes k0-NG .. k1+NG
  auto fetch = [&](int q) {
    const double* pl = ibase + (long long)q * pstride;
#pragma unroll
    for (int r = 0; r < NLD; ++r)
      if (NT * r < nA) pre[r] = pl[goff[r]];
  };
  auto stage = [&](double* Ab) {
#pragma unroll
    for (int r = 0; r < NLD; ++r) {
      const int e = t + NT * r;
      if (e < nA) Ab[padded ? e + e / nxg : e] = pre[r];
    }
  };
  fetch(0);
  stage(A0);
  __syncthreads();
  auto step = [&](auto zzc, int q) __attribute__((always_inline)) {
    constexpr int ZZ = decltype(zzc)::value;
    const double* Ab = A0 + (q & 1) * asz;
    if (q + 1 < nq) fetch(q + 1);
    // y-pass
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      if (yoff[it] < 0) continue;
      const double* a = Ab + yoff[it];
      double in[NW + 3];
#pragma unroll
      for (int m = 0; m < NW + 3; ++m) in[m] = a[m * ld];
      double* o = Bs + yoff[it];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        // symmetric weights (every filter type of the library): w_m (in[m] + in[2NG-m]), centre tap last
        double y = W.w[0] * (in[s4] + in[s4 + 2 * NG]);
#pragma unroll
        for (int m = 1; m < NG; ++m) y += W.w[m] * (in[s4 + m] + in[s4 + 2 * NG - m]);
        y += W.w[NG] * in[s4 + NG];
        o[s4 * ld] = y;
      }
    }
    __syncthreads();
    // x-pass + z-window
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      if (xoff[it] < 0) continue;
      const d2* bp2 = (const d2*)(Bs + xoff[it]);
      double v[2 * NG + 2];
#pragma unroll
      for (int s2 = 0; s2 <= NG; ++s2) { const d2 u = bp2[s2]; v[2 * s2] = u.x; v[2 * s2 + 1] = u.y; }
      double x0 = W.w[0] * (v[0] + v[2 * NG]), x1 = W.w[0] * (v[1] + v[2 * NG + 1]);
#pragma unroll
      for (int l = 1; l < NG; ++l) { x0 += W.w[l] * (v[l] + v[2 * NG - l]); x1 += W.w[l] * (v[l + 1] + v[2 * NG + 1 - l]); }
      x0 += W.w[NG] * v[NG];
      x1 += W.w[NG] * v[NG + 1];
#pragma unroll
      for (int d = 0; d < NW; ++d) {  // output a = q - d sees this plane as its n = d
        constexpr int dummy = 0;
        (void)dummy;
        const int slot = ((ZZ - d) % NW + NW) % NW;
        acc[it][0][slot] += W.w[d] * x0;
        acc[it][1][slot] += W.w[d] * x1;
      }
      constexpr int done = ((ZZ - 2 * NG) % NW + NW) % NW;  // the output whose last plane (n = 2NG) this was
      const int aq = q - 2 * NG;
      if (aq >= 0) {
        double* op = obase + (long long)aq * opstride + ooff[it];
        if (al16 && second[it]) *(d2*)op = d2{acc[it][0][done], acc[it][1][done]};
        else { op[0] = acc[it][0][done]; if (second[it]) op[1] = acc[it][1][done]; }
      }
      acc[it][0][done] = 0.0;
      acc[it][1][done] = 0.0;
    }
    if (q + 1 < nq) stage(A0 + ((q + 1) & 1) * asz);
    __syncthreads();
  };
  int q = 0;
#define PA_SS(z) if (q < nq) { step(std::integral_constant<int, (z) % NW>{}, q); ++q; }
  while (q < nq) {
    PA_SS(0) PA_SS(1) PA_SS(2)
    if (NW > 3) { PA_SS(3) PA_SS(4) }
    if (NW > 5) { PA_SS(5) PA_SS(6) }
    if (NW > 7) { PA_SS(7) PA_SS(8) }
    if (NW > 9) { PA_SS(9) PA_SS(10) PA_SS(11) PA_SS(12) }
    if (NW > 13) { PA_SS(13) PA_SS(14) PA_SS(15) PA_SS(16) }
  }
#undef PA_SS
}

// shape of a separable launch for a level / FAB whose largest box is nx x ny x nz; false: use the tap-order kernels.
// NG <= 2: 512 threads, two column pairs per thread (<= 114 VGPRs: two workgroups per CU).  Wider windows keep one pair
// per thread (the window of 2NG+1 sums per column is the register budget): 512 threads where a strip of a narrow box
// has no more pairs than that, else 1024 threads (one workgroup per CU, 16 waves).
struct SepShape { int TY, kseg, nys, T, ld_max, nt, nit; size_t lds; };
static bool sep_shape(int nx, int ny, int nz, int ng, unsigned nboxes, int ncomp, SepShape& S) {
  if (!(ng == 1 || ng == 2 || ng == 3 || ng == 4 || ng == 6 || ng == 8)) return false;
  const int nxg = nx + 2 * ng, ld = nxg + (nxg & 1), nxh = (nx + 1) / 2;
  const int ty0 = std::min(32, (ny + 3) / 4 * 4);
  auto fit = [&](int nt, int nit) {
    const int nld = nt == 512 ? 7 : 5;
    int TY = ty0;
    while (TY >= 4 && ((TY + 2 * ng) * nxg > nld * nt || TY * nxh > nt * nit || (TY / 4) * nxg > 2 * nt)) TY -= 4;
    return TY;
  };
  if (ng <= 2) { S.nt = 512; S.nit = 2; }
  else { S.nit = 1; S.nt = fit(512, 1) >= std::min(ty0, 16) ? 512 : 1024; }
  const int TY = fit(S.nt, S.nit);
  if (TY < 4) return false;
  // planes per workgroup: a segment re-reads 2 ng planes, so wide windows take long segments (measured on a 512^3 level of
  // 128^3 boxes, fgr 8: 32 / 64 / 128 planes 0.595 / 0.531 / 0.500 ms; fgr 2 and 4 are flat); shorter while a launch would
  // leave CUs without a workgroup
  S.TY = TY;
  S.nys = (ny + TY - 1) / TY;
  int kseg = std::min(ng > 2 ? 128 : 64, nz);
  while (kseg > 8 * ng && kseg > 16 && (long long)nboxes * ncomp * S.nys * ((nz + kseg - 1) / kseg) < 512) kseg = (kseg + 1) / 2;
  S.kseg = std::max(1, kseg);
  S.T = S.nys * ((nz + S.kseg - 1) / S.kseg);
  S.ld_max = ld;
  S.lds = sizeof(double) * (size_t)(2 * (TY + 2 * ng) + TY) * ld;
  return S.lds <= 150 * 1024;
}
template <typename BP, int NG, int NT, int NIT>
static void sep_launch(hipStream_t st, const BP& bp, const SepShape& S, unsigned nboxes, int scomp, int ncomp, const FilterW& W) {
  // more than 64 KiB of dynamic LDS needs the attribute, and function attributes are per DEVICE: one flag per device and
  // instantiation (ngpus > 1 in one process: pa::Team runs one host thread per GPU; advisor finding, round 3)
  static std::atomic<unsigned long long> done{0};
  int dev = 0;
  (void)hipGetDevice(&dev);
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(done.load(std::memory_order_acquire) & bit)) {
    if (hipFuncSetAttribute((const void*)k_filter_sep<BP, NG, NT, NIT>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) == hipSuccess)
      done.fetch_or(bit, std::memory_order_release);
    else
      (void)hipGetLastError();  // the launch below then fails on its own if the LDS request is refused; pa_boxfilter_level reports it
  }
  const dim3 g(8u * (unsigned)S.T * ((nboxes + 7u) / 8u), (unsigned)ncomp);
  hipLaunchKernelGGL((k_filter_sep<BP, NG, NT, NIT>), g, dim3(NT), S.lds, st, bp, scomp, W, S.TY, S.kseg, S.nys, S.T, (int)nboxes, S.ld_max);
}
template <typename BP, int NG>
static void sep_dispatch(hipStream_t st, const BP& bp, const SepShape& S, unsigned nboxes, int scomp, int ncomp, const FilterW& W) {
  if constexpr (NG <= 2) sep_launch<BP, NG, 512, 2>(st, bp, S, nboxes, scomp, ncomp, W);
  else if (S.nt == 512) sep_launch<BP, NG, 512, 1>(st, bp, S, nboxes, scomp, ncomp, W);
  else sep_launch<BP, NG, 1024, 1>(st, bp, S, nboxes, scomp, ncomp, W);
}

// any filter width: taps straight from global memory (L1/L2), same summation order
template <typename BP>
__global__ __launch_bounds__(256) void k_boxfilter_generic(BP bp, int scomp, int ncomp, int ng, FilterW W) {
  FabView I, O;
  DBox V;
  double dxinv[3];
  if (!bp.get(blockIdx.y, I, O, V, dxinv)) return;
  int i, j, k0, k1;
  if (!tile_cell(V, i, j, k0, k1)) return;
  const int nw = 2 * ng + 1;
  for (int c = scomp; c < scomp + ncomp; ++c)
    for (int k = k0; k <= k1; ++k) {
      double acc = 0.0;
      for (int n = 0; n < nw; ++n)
        for (int m = 0; m < nw; ++m)
          for (int l = 0; l < nw; ++l) acc += ((W.w[l] * W.w[m]) * W.w[n]) * I(i + l - ng, j + m - ng, k + n - ng, c);
      O(i, j, k, c) = acc;
    }
}

// what pa_filter_last_launch reports: {kind, ng, threads, TY, y strips, kseg, z segments, refused}, all for the LARGEST box of
// the launch (the one the launch was shaped for); written on the host, next to the launch it describes
enum { PA_FK_NONE = 0, PA_FK_SEP = 1, PA_FK_STREAM = 2, PA_FK_TILE = 3, PA_FK_GENERIC = 4, PA_FK_2D = 5 };
static void filter_note(pa_ctx* ctx, int kind, int ng, int nt, int TY, int nys, int kseg, int nzs, int refused) {
  const int32_t v[8] = {kind, ng, nt, TY, nys, kseg, nzs, refused};
  for (int q = 0; q < 8; ++q) ctx->filter_info[q] = v[q];
}
static void filter_note_cells(pa_ctx* ctx, int kind, int ng, int nx, int ny, int nz, int refused) {  // the thread-per-cell tiling of tile_grid_dims
  const int TY = nx <= 32 ? 8 : PA_TY;
  filter_note(ctx, kind, ng, 256, TY, (ny + TY - 1) / TY, PA_TZ, (nz + PA_TZ - 1) / PA_TZ, refused);
}

template <typename BP>
static void filter_launch(pa_ctx* ctx, const BP& bp, int nx, int ny, int nz, unsigned nboxes, int scomp, int ncomp, int ng, const FilterW& W) {
  const hipStream_t st = ctx->stream;
  auto grid = [&](int TX, int TY, int TZ) { return dim3(((nx + TX - 1) / TX) * ((ny + TY - 1) / TY) * ((nz + TZ - 1) / TZ), nboxes); };
  // default: the separable form (1e-12 relative); PA_FILTER_EXACT=1: the reference's tap order, bit for bit (read per launch)
  const bool exact = pa_opt().filter_exact != 0;
  SepShape S;
  bool sym = true;  // the separable kernel pairs the taps w_m (a[m] + a[2ng - m]); every filter type of the library is symmetric
  for (int q = 0; q < ng; ++q) sym = sym && W.w[q] == W.w[2 * ng - q];
  const bool asked = !exact && ng >= 1 && sym, sep = asked && sep_shape(nx, ny, nz, ng, nboxes, ncomp, S);
  const int refused = asked && !sep;  // the separable form was asked for and the shape rule said no: the tap-order kernels below
  if (sep) {
    filter_note(ctx, PA_FK_SEP, ng, S.nt, S.TY, S.nys, S.kseg, (nz + S.kseg - 1) / S.kseg, 0);
    switch (ng) {
      case 1: sep_dispatch<BP, 1>(st, bp, S, nboxes, scomp, ncomp, W); return;
      case 2: sep_dispatch<BP, 2>(st, bp, S, nboxes, scomp, ncomp, W); return;
      case 3: sep_dispatch<BP, 3>(st, bp, S, nboxes, scomp, ncomp, W); return;
      case 4: sep_dispatch<BP, 4>(st, bp, S, nboxes, scomp, ncomp, W); return;
      case 6: sep_dispatch<BP, 6>(st, bp, S, nboxes, scomp, ncomp, W); return;
      case 8: sep_dispatch<BP, 8>(st, bp, S, nboxes, scomp, ncomp, W); return;
      default: break;
    }
  }
  // box weights (w0/2, w0, ..., w0, w0/2): the streaming kernel
  const int nw = 2 * ng + 1;
  bool box = ng >= 1 && W.w[0] == 0.5 * W.w[1] && W.w[nw - 1] == W.w[0];
  for (int q = 2; q < nw - 1 && box; ++q) box = W.w[q] == W.w[1];
  if (box && (ng == 1 || ng == 2 || ng == 4)) {
    const int kseg = std::max(1, std::min(32, nz));
    const dim3 g = grid(32, 8, kseg);
    filter_note(ctx, PA_FK_STREAM, ng, 256, 8, (ny + 7) / 8, kseg, (nz + kseg - 1) / kseg, refused);
    if (ng == 1) hipLaunchKernelGGL((k_boxfilter_stream<BP, 1>), g, dim3(256), 0, st, bp, scomp, ncomp, W.w[1], kseg);
    else if (ng == 2) hipLaunchKernelGGL((k_boxfilter_stream<BP, 2>), g, dim3(256), 0, st, bp, scomp, ncomp, W.w[1], kseg);
    else hipLaunchKernelGGL((k_boxfilter_stream<BP, 4>), g, dim3(256), 0, st, bp, scomp, ncomp, W.w[1], kseg);
    return;
  }
  if (ng == 1 || ng == 2 || ng == 4) filter_note(ctx, PA_FK_TILE, ng, 256, 8, (ny + 7) / 8, ng == 4 ? 4 : 8, (nz + (ng == 4 ? 4 : 8) - 1) / (ng == 4 ? 4 : 8), refused);
  else filter_note_cells(ctx, PA_FK_GENERIC, ng, nx, ny, nz, refused);
  if (ng == 1) hipLaunchKernelGGL((k_boxfilter<BP, 1, 32, 8, 8>), grid(32, 8, 8), dim3(256), 0, st, bp, scomp, ncomp, W);
  else if (ng == 2) hipLaunchKernelGGL((k_boxfilter<BP, 2, 32, 8, 8>), grid(32, 8, 8), dim3(256), 0, st, bp, scomp, ncomp, W);
  else if (ng == 4) hipLaunchKernelGGL((k_boxfilter<BP, 4, 32, 8, 4>), grid(32, 8, 4), dim3(256), 0, st, bp, scomp, ncomp, W);
  else hipLaunchKernelGGL(k_boxfilter_generic<BP>, tile_grid_dims(nx, ny, nz, nboxes), dim3(256), 0, st, bp, scomp, ncomp, ng, W);
}

extern "C" int pa_boxfilter_level(pa_ctx* ctx, const pa_mf* in, pa_mf* out, int scomp, int ncomp, int ng, const double* w) {
  PaBind bind_(ctx);
  if (!ctx || !in || !out || !w) return pa_fail(ctx, "pa_boxfilter_level: null argument");
  if (in->lev != out->lev) return pa_fail(ctx, "pa_boxfilter_level: different levels");
  if (ng < 0 || ng > 16 || ng > in->ng) return pa_fail(ctx, "pa_boxfilter_level: input has fewer ghost cells than the filter half-width");
  if (scomp < 0 || ncomp < 1 || scomp + ncomp > in->ncomp || scomp + ncomp > out->ncomp) return pa_fail(ctx, "pa_boxfilter_level: component range");
  FilterW W;
  for (int q = 0; q < 2 * ng + 1; ++q) W.w[q] = w[q];
  const pa_level* L = in->lev;
  if (in->lev->boxes.empty()) return 0;  // a rank that owns no box of this level
  LevelBP2 bp{L->view, in->view, out->view};
  ProfScope prof(ctx, PA_TAG_FILTER);
  filter_launch(ctx, bp, L->maxn[0], L->maxn[1], L->maxn[2], (unsigned)L->boxes.size(), scomp, ncomp, ng, W);
  PA_HIP(hipGetLastError());
  return 0;
}

// Filter::apply_filter on EVERY level of a hierarchy (the level loop of filterPlt.cpp:206-219).  The levels do not depend on each
// other and a level of a few 10^7 cells does not fill the chip (config 3: 16.8 M cells per level at 0.37-0.49 of HBM), so
// (Each level's launch on a stream of its own between a fork and a join was MEASURED slower -- config 3's three levels 0.304 ms side
// by side against 0.248 ms one after the other: the fork / join events cost more than the tails they fill,
// profiles/r04_small_experiments.txt -- and went with its switch in round 6.)
extern "C" int pa_boxfilter_hierarchy(pa_ctx* ctx, int nlev, const pa_mf* const* in, pa_mf* const* out, int scomp, int ncomp, const int32_t* ngs,
                                      const double* const* ws) {
  PaBind bind_(ctx);
  if (!ctx || nlev <= 0 || !in || !out || !ngs || !ws) return pa_fail(ctx, "pa_boxfilter_hierarchy: null argument");
  // (the levels on one stream each was measured slower than one after the other on one stream: DESIGN_HISTORY.md R4)
  for (int l = 0; l < nlev; ++l)
    if (pa_boxfilter_level(ctx, in[l], out[l], scomp, ncomp, ngs[l], ws[l])) return 1;
  return 0;
}

// 2-D build of Filter::apply_filter: out(i,j,c) = sum_m sum_l (w_l w_m) in(i+l, j+m, c) on a level stored as one plane
// of cells (the z index is carried along untouched); thread per cell -- 2-D data is small next to the 3-D levels
template <typename BP>
__global__ __launch_bounds__(256) void k_boxfilter2d(BP bp, int scomp, int ncomp, int ng, FilterW W) {
  FabView I, O;
  DBox V;
  double dxinv[3];
  if (!bp.get(blockIdx.y, I, O, V, dxinv)) return;
  int i, j, k0, k1;
  if (!tile_cell(V, i, j, k0, k1)) return;
  const int nw = 2 * ng + 1;
  for (int c = scomp; c < scomp + ncomp; ++c)
    for (int k = k0; k <= k1; ++k) {
      double acc = 0.0;
      for (int m = 0; m < nw; ++m)
        for (int l = 0; l < nw; ++l) acc += (W.w[l] * W.w[m]) * I(i + l - ng, j + m - ng, k, c);
      O(i, j, k, c) = acc;
    }
}

extern "C" int pa_boxfilter_level2d(pa_ctx* ctx, const pa_mf* in, pa_mf* out, int scomp, int ncomp, int ng, const double* w) {
  PaBind bind_(ctx);
  if (!ctx || !in || !out || !w) return pa_fail(ctx, "pa_boxfilter_level2d: null argument");
  if (in->lev != out->lev) return pa_fail(ctx, "pa_boxfilter_level2d: different levels");
  if (ng < 0 || ng > 16 || ng > in->ng) return pa_fail(ctx, "pa_boxfilter_level2d: input has fewer ghost cells than the filter half-width");
  if (scomp < 0 || ncomp < 1 || scomp + ncomp > in->ncomp || scomp + ncomp > out->ncomp) return pa_fail(ctx, "pa_boxfilter_level2d: component range");
  FilterW W;
  for (int q = 0; q < 2 * ng + 1; ++q) W.w[q] = w[q];
  const pa_level* L = in->lev;
  if (in->lev->boxes.empty()) return 0;  // a rank that owns no box of this level
  LevelBP2 bp{L->view, in->view, out->view};
  ProfScope prof(ctx, PA_TAG_FILTER);
  filter_note_cells(ctx, PA_FK_2D, ng, L->maxn[0], L->maxn[1], L->maxn[2], 0);
  hipLaunchKernelGGL(k_boxfilter2d<LevelBP2>, tile_grid_dims(L->maxn[0], L->maxn[1], L->maxn[2], (unsigned)L->boxes.size()), dim3(256), 0, ctx->stream, bp, scomp,
                     ncomp, ng, W);
  PA_HIP(hipGetLastError());
  return 0;
}

extern "C" int pa_filter_last_launch(const pa_ctx* ctx, int32_t info[8]) {
  if (!ctx || !info) return 1;
  for (int q = 0; q < 8; ++q) info[q] = ctx->filter_info[q];
  return 0;
}

extern "C" int pa_boxfilter_fab(pa_ctx* ctx, pa_box valid, const pa_fab* in, pa_fab* out, int scomp, int ncomp, int ng, const double* w) {
  PaBind bind_(ctx);
  if (!ctx || !in || !out || !w) return pa_fail(ctx, "pa_boxfilter_fab: null argument");
  if (ng < 0 || ng > 16) return pa_fail(ctx, "pa_boxfilter_fab: filter half-width out of range");
  std::string why;
  if (!fab_covers(*in, valid, ng, scomp, ncomp, why) || !fab_covers(*out, valid, 0, scomp, ncomp, why)) return pa_fail(ctx, "pa_boxfilter_fab: " + why);
  FilterW W;
  for (int q = 0; q < 2 * ng + 1; ++q) W.w[q] = w[q];
  FabBP2 bp{fab_view(*in), fab_view(*out), to_dbox(valid), {1, 1, 1}};
  filter_launch(ctx, bp, valid.hi[0] - valid.lo[0] + 1, valid.hi[1] - valid.lo[1] + 1, valid.hi[2] - valid.lo[2] + 1, 1, scomp, ncomp, ng, W);
  PA_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ ghost cells for filterPlt
// shell enumeration shared with FillBoundary (pa_core.hip)
__device__ __forceinline__ bool shell_cell2(const DBox& B, int ng, long long t, int& i, int& j, int& k) {
  const int nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const int gx = nx + 2 * ng, gy = ny + 2 * ng;
  const long long nzs = (long long)ng * gy * gx, nys = (long long)nz * ng * gx, nxs = (long long)nz * ny * ng;
  if (t < 2 * nzs) {
    const int s = t >= nzs;
    if (s) t -= nzs;
    i = B.lo[0] - ng + (int)(t % gx);
    j = B.lo[1] - ng + (int)((t / gx) % gy);
    k = (int)(t / ((long long)gx * gy));
    k = s ? B.hi[2] + 1 + k : B.lo[2] - ng + k;
    return true;
  }
  t -= 2 * nzs;
  if (t < 2 * nys) {
    const int s = t >= nys;
    if (s) t -= nys;
    i = B.lo[0] - ng + (int)(t % gx);
    j = (int)((t / gx) % ng);
    k = B.lo[2] + (int)(t / ((long long)gx * ng));
    j = s ? B.hi[1] + 1 + j : B.lo[1] - ng + j;
    return true;
  }
  t -= 2 * nys;
  if (t < 2 * nxs) {
    const int s = t >= nxs;
    if (s) t -= nxs;
    i = (int)(t % ng);
    j = B.lo[1] + (int)((t / ng) % ny);
    k = B.lo[2] + (int)(t / ((long long)ng * ny));
    i = s ? B.hi[0] + 1 + i : B.lo[0] - ng + i;
    return true;
  }
  return false;
}

static long long min_shell2(const pa_level* L, int ng) {  // workgroups per box of the grid-stride shell kernels: enough for the smallest box
  long long m = 1LL << 50;
  for (const DBox& B : L->boxes) {
    const long long nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
    m = std::min(m, (nx + 2 * ng) * (ny + 2 * ng) * (nz + 2 * ng) - nx * ny * nz);
  }
  return std::max<long long>(m, 1);
}
// first-order extrapolation: a ghost cell outside a non-periodic wall takes the value of the
// nearest cell inside the domain (which lies in the same grown FAB and is already filled)
__global__ void k_foextrap(DLevelView L, DMFView M, int comp, int ncomp, int ngf) {
  const int b = blockIdx.y;
  const DBox B = L.boxes[b];
  const long long nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const long long nsh = (nx + 2 * ngf) * (ny + 2 * ngf) * (nz + 2 * ngf) - nx * ny * nz;
  double* f = M.data + M.off[b];
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nsh; t += (long long)gridDim.x * blockDim.x) {  // grid-stride (min_shell2)
    int q[3];
    if (!shell_cell2(B, ngf, t, q[0], q[1], q[2])) continue;
    int p[3] = {q[0], q[1], q[2]};
    bool out = false;
    for (int d = 0; d < 3; ++d)
      if (!L.is_per[d]) {
        if (p[d] < L.domlo[d]) { p[d] = L.domlo[d]; out = true; }
        if (p[d] > L.domhi[d]) { p[d] = L.domhi[d]; out = true; }
      }
    if (!out) continue;
    for (int c = comp; c < comp + ncomp; ++c) f[fab_index(B, M.ng, M.ncomp, c, q[0], q[1], q[2])] = f[fab_index(B, M.ng, M.ncomp, c, p[0], p[1], p[2])];
  }
}

extern "C" int pa_foextrap(pa_ctx* ctx, pa_mf* M, int comp, int ncomp, int ng) {
  PaBind bind_(ctx);
  if (!ctx || !M) return pa_fail(ctx, "pa_foextrap: null argument");
  if (ng > M->ng || ng < 0 || comp < 0 || comp + ncomp > M->ncomp) return pa_fail(ctx, "pa_foextrap: ng/component range");
  if (ng == 0) return 0;
  if (M->lev->boxes.empty()) return 0;  // a rank that owns no box of this level
  dim3 grid((unsigned)((min_shell2(M->lev, ng) + 255) / 256), (unsigned)M->lev->boxes.size());
  hipLaunchKernelGGL(k_foextrap, grid, dim3(256), 0, ctx->stream, M->lev->view, M->view, comp, ncomp, ng);
  PA_HIP(hipGetLastError());
  return 0;
}

// FillPatchTwoLevels for the ghost cells that no fine box covers: piecewise constant or
// cell-conservative linear interpolation of the coarse level (see oracle/pa_oracle.c
// orc_fillpatch_two_levels for the restated limiter)
__device__ __forceinline__ void fillpatch2_cell(const DLevelView& L, const DMFView& M, const DLevelView& LC, const DMFView& MC, int comp, int cshift, int ncomp, int ngf, int r,
                                                int interp, int* nbad, int b, const DBox& B, long long t) {
  int q[3];
  if (!shell_cell2(B, ngf, t, q[0], q[1], q[2])) return;
  if (classify(L, q[0], q[1], q[2]) != 1) return;  // covered: FillBoundary; outside a wall: foextrap afterwards
  const int qc[3] = {coarsen_idx(q[0], r), coarsen_idx(q[1], r), coarsen_idx(q[2], r)};
  double* f = M.data + M.off[b];
  for (int c = comp; c < comp + ncomp; ++c) {
    bool ok = true;
    const double u0 = crse_val(LC, MC, c + cshift, qc[0], qc[1], qc[2], ok);
    double val = u0;
    if (interp == 1) {
      // mf_cell_cons_lin_interp_mcslope + mf_cell_cons_lin_interp (AMReX, recalled; oracle/pa_oracle.c
      // orc_fillpatch_two_levels): central slopes limited by df/db, one common factor alpha with
      // dumax = sum |s_d| (r-1)/(2r); coarse neighbours beyond a non-periodic wall are the foextrap-filled
      // coarse ghost cells = the nearest cell inside the domain (filterPlt.cpp:164-173)
      auto cu = [&](int n) -> double {  // neighbour n = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
        int p[3] = {qc[0] + n % 3 - 1, qc[1] + (n / 3) % 3 - 1, qc[2] + n / 9 - 1};
        for (int d = 0; d < 3; ++d)
          if (!LC.is_per[d]) { p[d] = max(p[d], LC.domlo[d]); p[d] = min(p[d], LC.domhi[d]); }
        return crse_val(LC, MC, c + cshift, p[0], p[1], p[2], ok);
      };
      double sl[3], alpha;
      ccl_slopes<false>(cu, u0, r, sl, alpha);
      const int rem[3] = {q[0] - qc[0] * r, q[1] - qc[1] * r, q[2] - qc[2] * r};
      const double acc = ccl_child(u0, sl, alpha, rem, r);
      val = acc;
    }
    if (!ok) atomicAdd(nbad, 1);
    f[fab_index(B, M.ng, M.ncomp, c, q[0], q[1], q[2])] = val;
  }
}
// thread per ghost-shell cell, grid-stride: gridDim.x is sized by the SMALLEST shell of the level (min_shell2), larger boxes take more trips
__global__ void k_fillpatch2(DLevelView L, DMFView M, DLevelView LC, DMFView MC, int comp, int cshift /* coarse component = fine component + cshift */, int ncomp, int ngf, int r,
                             int interp, int* nbad) {
  const int b = blockIdx.y;
  const DBox B = L.boxes[b];
  const long long nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const long long nsh = (nx + 2 * ngf) * (ny + 2 * ngf) * (nz + 2 * ngf) - nx * ny * nz;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nsh; t += (long long)gridDim.x * blockDim.x)
    fillpatch2_cell(L, M, LC, MC, comp, cshift, ncomp, ngf, r, interp, nbad, b, B, t);
}

// The same for interp_type 1 with one thread per COARSE parent cell of the ghost shell: the 8 children of a parent share
// its limited slopes and common factor (27 coarse values through the owner map, min / max, two divisions), which the
// per-ghost-cell kernel recomputed for each of them.  Same operations on the same operands per child, so the ghost cells
// are bit-identical (the filter tests compare the shell with the oracle).  Parents whose children are all valid cells of
// the box leave at once.
// interp_type 1 in two steps.  (1) k_fp_find, ONCE per (fine level, coarse level, ghost width): thread per coarse parent of
// every box's ghost shell; the parents with at least one child that is a coarse-fine ghost cell go to a list {box, children
// mask, parent cell} kept with the fine level (FpPlan) -- the geometry of a hierarchy does not change between calls, and of
// the 3 M parents of config 3's finest level pair only a few hundred thousand qualify.  (2) k_fp_do, every call: thread per
// list entry, dense wavefronts: the 8 children of a parent share its limited slopes and common factor (27 coarse values, min /
// max, two divisions), which the per-ghost-cell kernel recomputed for each of them.  Same operations on the same operands
// per child, so the ghost cells are bit-identical (the filter tests compare the shell with the oracle).
// uniform: every coarse parent's 8 children share one owner-grid cell and one side of every wall (even owner-grid cells and
// domain bounds: checked on the host), so ONE classification per parent stands for all of them.
__global__ __launch_bounds__(256) void k_fp_find(DLevelView L, int ngf, int uniform, int4* items, int* count, int cap) {
  const int b = blockIdx.y, r = 2;
  const DBox B = L.boxes[b];
  int clo[3], cn[3];
  for (int d = 0; d < 3; ++d) {
    clo[d] = coarsen_idx(B.lo[d] - ngf, r);
    cn[d] = coarsen_idx(B.hi[d] + ngf, r) - clo[d] + 1;
  }
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (t >= (long long)cn[0] * cn[1] * cn[2]) return;
  const unsigned u = (unsigned)t, rr = u / (unsigned)cn[0];
  const int qc[3] = {clo[0] + (int)(u - rr * (unsigned)cn[0]), clo[1] + (int)(rr % (unsigned)cn[1]), clo[2] + (int)(rr / (unsigned)cn[1])};
  bool interior = true;
  for (int d = 0; d < 3; ++d) interior = interior && (r * qc[d] >= B.lo[d] && r * qc[d] + r - 1 <= B.hi[d]);
  if (interior) return;
  unsigned geo = 0;  // children inside the grown box and outside the valid box
  for (int c8 = 0; c8 < 8; ++c8) {
    const int q[3] = {r * qc[0] + (c8 & 1), r * qc[1] + ((c8 >> 1) & 1), r * qc[2] + (c8 >> 2)};
    bool in = true, valid = true;
    for (int d = 0; d < 3; ++d) {
      in = in && q[d] >= B.lo[d] - ngf && q[d] <= B.hi[d] + ngf;
      valid = valid && q[d] >= B.lo[d] && q[d] <= B.hi[d];
    }
    if (in && !valid) geo |= 1u << c8;
  }
  if (!geo) return;
  unsigned mask = 0;  // children that are coarse-fine ghost cells of this FAB
  if (uniform) {
    if (classify(L, r * qc[0], r * qc[1], r * qc[2]) == 1) mask = geo;
  } else {
    for (int c8 = 0; c8 < 8; ++c8)
      if (((geo >> c8) & 1u) && classify(L, r * qc[0] + (c8 & 1), r * qc[1] + ((c8 >> 1) & 1), r * qc[2] + (c8 >> 2)) == 1) mask |= 1u << c8;
  }
  if (!mask) return;
  const int i = atomicAdd(count, 1);
  if (i < cap) items[i] = make_int4(b | (int)(mask << 24), qc[0], qc[1], qc[2]);
}

__device__ __forceinline__ void fp_do_item(const DLevelView& L, const DMFView& M, const DLevelView& LC, const DMFView& MC, int comp, int cshift, int ncomp, const int4* items, int n,
                                           int* nbad, const int t) {
  const int r = 2;
  if (t >= n) return;
  const int4 it = items[t];
  const int b = it.x & 0xffffff;
  const unsigned mask = (unsigned)it.x >> 24;
  const int qc[3] = {it.y, it.z, it.w};
  const DBox B = L.boxes[b];
  double* f = M.data + M.off[b];
  // the coarse box that holds the parent (through a periodic image if need be): its neighbours inside the same box are plain
  // loads at fixed offsets, issued together; only the ones beyond it (a parent on the box's surface) walk the owner map
  int pw[3] = {qc[0], qc[1], qc[2]};
  const int cb = wrap_cell(LC, pw) ? owner_of(LC, pw) : -1;
  const DBox CB = LC.boxes[cb >= 0 ? cb : 0];
  const int sy = CB.hi[0] - CB.lo[0] + 1 + 2 * MC.ng, sz = sy * (CB.hi[1] - CB.lo[1] + 1 + 2 * MC.ng);  // a coarse FAB is far below 2^31 cells
  for (int c = comp; c < comp + ncomp; ++c) {
    bool ok = true;
    double v[27];  // coarse values, index (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
    // a parent without an owning coarse box (fine level not properly nested): every neighbour is `far`, the 27 predicated
    // loads below read element 0 of the coarse multifab (in bounds) and crse_val counts the ghost cells in nbad
    const double* p0 = cb >= 0 ? MC.data + MC.off[cb] + fab_index(CB, MC.ng, MC.ncomp, c + cshift, pw[0], pw[1], pw[2]) : MC.data;
    unsigned far = 0;  // neighbours that are not cells of CB
#pragma unroll
    for (int n = 0; n < 27; ++n) {
      // coarse neighbours beyond a non-periodic wall are the nearest cell inside the domain (filterPlt.cpp:164-173)
      int p[3] = {qc[0] + n % 3 - 1, qc[1] + (n / 3) % 3 - 1, qc[2] + n / 9 - 1};
      bool in = cb >= 0;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        if (!LC.is_per[d]) { p[d] = max(p[d], LC.domlo[d]); p[d] = min(p[d], LC.domhi[d]); }
        const int len = LC.domhi[d] - LC.domlo[d] + 1;
        if (p[d] < LC.domlo[d]) p[d] += len;  // one period is enough where it matters: further out the cell is not in CB either
        if (p[d] > LC.domhi[d]) p[d] -= len;
        in = in && p[d] >= CB.lo[d] && p[d] <= CB.hi[d];
      }
      const int o = in ? (p[2] - pw[2]) * sz + (p[1] - pw[1]) * sy + (p[0] - pw[0]) : 0;
      double x = p0[o];
      if (MC.xform) x = (x - MC.xa) * MC.xb;
      v[n] = x;
      far |= in ? 0u : 1u << n;
    }
    if (far) {
#pragma unroll
      for (int n = 0; n < 27; ++n) {
        if (!((far >> n) & 1u)) continue;
        int p[3] = {qc[0] + n % 3 - 1, qc[1] + (n / 3) % 3 - 1, qc[2] + n / 9 - 1};
#pragma unroll
        for (int d = 0; d < 3; ++d)
          if (!LC.is_per[d]) { p[d] = max(p[d], LC.domlo[d]); p[d] = min(p[d], LC.domhi[d]); }
        v[n] = crse_val(LC, MC, c + cshift, p[0], p[1], p[2], ok);
      }
    }
    const double u0 = v[13];
    double sl[3], alpha;
    ccl_slopes<true>([&](int n) { return v[n]; }, u0, r, sl, alpha);  // (pa_cclin.h: unrolled, so v[] stays in registers)
    if (!ok) atomicAdd(nbad, __popc(mask));
    for (int c8 = 0; c8 < 8; ++c8) {
      if (!((mask >> c8) & 1u)) continue;
      const int q[3] = {r * qc[0] + (c8 & 1), r * qc[1] + ((c8 >> 1) & 1), r * qc[2] + (c8 >> 2)};
      const int rem[3] = {q[0] - qc[0] * r, q[1] - qc[1] * r, q[2] - qc[2] * r};
      f[fab_index(B, M.ng, M.ncomp, c, q[0], q[1], q[2])] = ccl_child(u0, sl, alpha, rem, r);
    }
  }
}

__global__ __launch_bounds__(256, 2) void k_fp_do(DLevelView L, DMFView M, DLevelView LC, DMFView MC, int comp, int cshift, int ncomp, const int4* items, int n, int* nbad) {
  fp_do_item(L, M, LC, MC, comp, cshift, ncomp, items, n, nbad, blockIdx.x * 256 + threadIdx.x);
}
// the level pairs of a hierarchy in ONE launch (pa_fill_ghosts_hierarchy): FillPatchTwoLevels reads VALID coarse cells only (through
// the owner map; beyond a wall the nearest cell inside), so the pairs do not depend on each other
struct FpdLev { DLevelView L; DMFView M; DLevelView LC; DMFView MC; int comp, cshift, ncomp; const int4* items; int n; };
struct FpdBatch { int n; unsigned wg0[PA_MAXB + 1]; FpdLev a[PA_MAXB]; };
__global__ __launch_bounds__(256, 2) void k_fp_do_levels(FpdBatch Bt, int* nbad) {
  int l = 0;
  while (l + 1 < Bt.n && blockIdx.x >= Bt.wg0[l + 1]) ++l;
  const int t = (int)(blockIdx.x - Bt.wg0[l]) * 256 + (int)threadIdx.x;
  // a constant index per case: the level's arguments stay in the kernel-argument segment (a run-time index into the by-value
  // array sends the whole batch through scratch memory: 191 us for two level pairs against 2 x 70 us for two k_fp_do launches)
  static_assert(PA_MAXB == 4, "one case per batch row");
  switch (l) {
    case 0: fp_do_item(Bt.a[0].L, Bt.a[0].M, Bt.a[0].LC, Bt.a[0].MC, Bt.a[0].comp, Bt.a[0].cshift, Bt.a[0].ncomp, Bt.a[0].items, Bt.a[0].n, nbad, t); break;
    case 1: fp_do_item(Bt.a[1].L, Bt.a[1].M, Bt.a[1].LC, Bt.a[1].MC, Bt.a[1].comp, Bt.a[1].cshift, Bt.a[1].ncomp, Bt.a[1].items, Bt.a[1].n, nbad, t); break;
    case 2: fp_do_item(Bt.a[2].L, Bt.a[2].M, Bt.a[2].LC, Bt.a[2].MC, Bt.a[2].comp, Bt.a[2].cshift, Bt.a[2].ncomp, Bt.a[2].items, Bt.a[2].n, nbad, t); break;
    default: fp_do_item(Bt.a[3].L, Bt.a[3].M, Bt.a[3].LC, Bt.a[3].MC, Bt.a[3].comp, Bt.a[3].cshift, Bt.a[3].ncomp, Bt.a[3].items, Bt.a[3].n, nbad, t); break;
  }
}
struct Fp2Args { DLevelView L; DMFView M; DLevelView LC; DMFView MC; int comp, cshift, ncomp, ngf, r, interp; };
__global__ void k_fillpatch2_levels(LevBatch<Fp2Args> Bt, int* nbad) {
  unsigned b;
  const Fp2Args& A = Bt.a[Bt.find(blockIdx.y, b)];
  const DBox B = A.L.boxes[b];
  const long long nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const long long nsh = (nx + 2 * A.ngf) * (ny + 2 * A.ngf) * (nz + 2 * A.ngf) - nx * ny * nz;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nsh; t += (long long)gridDim.x * blockDim.x)
    fillpatch2_cell(A.L, A.M, A.LC, A.MC, A.comp, A.cshift, A.ncomp, A.ngf, A.r, A.interp, nbad, (int)b, B, t);
}
struct FoArgs { DLevelView L; DMFView M; int comp, ncomp, ngf; };
__global__ void k_foextrap_levels(LevBatch<FoArgs> Bt) {
  unsigned b;
  const FoArgs& A = Bt.a[Bt.find(blockIdx.y, b)];
  const DBox B = A.L.boxes[b];
  const long long nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1, nz = B.hi[2] - B.lo[2] + 1;
  const long long nsh = (nx + 2 * A.ngf) * (ny + 2 * A.ngf) * (nz + 2 * A.ngf) - nx * ny * nz;
  double* f = A.M.data + A.M.off[b];
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nsh; t += (long long)gridDim.x * blockDim.x) {
    int q[3];
    if (!shell_cell2(B, A.ngf, t, q[0], q[1], q[2])) continue;
    int p[3] = {q[0], q[1], q[2]};
    bool out = false;
    for (int d = 0; d < 3; ++d)
      if (!A.L.is_per[d]) {
        if (p[d] < A.L.domlo[d]) { p[d] = A.L.domlo[d]; out = true; }
        if (p[d] > A.L.domhi[d]) { p[d] = A.L.domhi[d]; out = true; }
      }
    if (!out) continue;
    for (int c = A.comp; c < A.comp + A.ncomp; ++c) f[fab_index(B, A.M.ng, A.M.ncomp, c, q[0], q[1], q[2])] = f[fab_index(B, A.M.ng, A.M.ncomp, c, p[0], p[1], p[2])];
  }
}

FpPlan::~FpPlan() {
  if (d_items) (void)hipFree(d_items);
}

#define PA_HIPN(call)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                       \
      return nullptr;                                                                     \
    }                                                                                     \
  } while (0)
// the parent list of a (fine level, coarse level, ghost width) triple, built on first use (k_fp_find) and kept with the fine level
static const FpPlan* fp_parent_plan(pa_ctx* ctx, const pa_level* F, const pa_level* C, int ng) {
  long long mp = 0;
  for (const DBox& B : F->boxes) {
    long long n = 1;
    for (int d = 0; d < 3; ++d) n *= coarsen_idx(B.hi[d] + ng, 2) - coarsen_idx(B.lo[d] - ng, 2) + 1;
    mp = std::max(mp, n);
  }
  auto fail = [&](const char* m) -> const FpPlan* { pa_fail(ctx, m); return nullptr; };
  const auto key = std::make_pair(C->serial, ng);
  auto itp = F->fp_plans.find(key);
    if (itp == F->fp_plans.end()) {  // the list of parents, once
      if (F->boxes.size() >= (1u << 24)) return fail("pa_fillpatch_two_levels: too many boxes");
      bool uniform = F->g % 2 == 0;  // one classification per parent (see k_fp_find)
      for (int d = 0; d < 3; ++d) uniform = uniform && F->mlo[d] % 2 == 0 && F->domlo[d] % 2 == 0 && (F->domhi[d] + 1) % 2 == 0;
      long long cap = 0;  // parents of the shells
      for (const DBox& B : F->boxes) {
        long long all = 1, in = 1;
        for (int d = 0; d < 3; ++d) {
          all *= coarsen_idx(B.hi[d] + ng, 2) - coarsen_idx(B.lo[d] - ng, 2) + 1;
          in *= std::max(0, coarsen_idx(B.hi[d] - 1, 2) - coarsen_idx(B.lo[d] + 1, 2) + 1);  // parents whose 2 cells per direction are all valid (>=: a lower bound)
        }
        cap += all - in;
      }
      if (cap >= (1LL << 31)) return fail("pa_fillpatch_two_levels: ghost shell too large");
      std::unique_ptr<FpPlan> P(new FpPlan());
      PA_HIPN(hipMalloc(&P->d_items, sizeof(int4) * (size_t)std::max<long long>(cap, 1)));
      int* d_count = nullptr;
      PA_HIPN(hipMalloc(&d_count, sizeof(int)));
      PA_HIPN(hipMemsetAsync(d_count, 0, sizeof(int), ctx->stream));
      hipLaunchKernelGGL(k_fp_find, dim3((unsigned)((mp + 255) / 256), (unsigned)F->boxes.size()), dim3(256), 0, ctx->stream, F->view, ng, uniform ? 1 : 0,
                         (int4*)P->d_items, d_count, (int)cap);
      int n = 0;
      PA_HIPN(hipMemcpyAsync(&n, d_count, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
      PA_HIPN(hipStreamSynchronize(ctx->stream));
      (void)hipFree(d_count);
      if (n > cap) return fail("pa_fillpatch_two_levels: parent list overflow");
      P->n = n;
      itp = F->fp_plans.emplace(key, std::move(P)).first;
    }
  return itp->second.get();
}

extern "C" int pa_fillpatch_two_levels(pa_ctx* ctx, pa_mf* fine, const pa_mf* crse, int comp, int ncomp, int ng, int ratio, int interp_type) {
  PaBind bind_(ctx);
  if (!ctx || !fine || !crse) return pa_fail(ctx, "pa_fillpatch_two_levels: null argument");
  if (ng > fine->ng || ng < 0 || comp < 0 || comp + ncomp > fine->ncomp || comp + ncomp > crse->ncomp) return pa_fail(ctx, "pa_fillpatch_two_levels: ng/component range");
  // any integer refinement ratio (isosurface.cpp:1472,1518 and filterPlt.cpp:133,200 take the plotfile's); the cached parent
  // lists of interp_type 1 (k_fp_find / k_fp_do) are the ratio-2 form, other ratios take the per-ghost-cell kernel
  if (ratio < 2 || ratio > 16) return pa_fail(ctx, "pa_fillpatch_two_levels: refinement ratio must be 2 .. 16");
  if (interp_type != 0 && interp_type != 1) return pa_fail(ctx, "pa_fillpatch_two_levels: interp_type must be 0 (pc) or 1 (cell-conservative linear)");
  if (ng == 0) return 0;
  // sharded coarse level: the parents of the ghost layers (+ 1 coarse cell for slopes / min-max) from this rank's coarse-source copy
  int ccomp = comp;
  if (pa_coarse_source(ctx, fine->lev, crse, comp, ncomp, 1, ng, 1, &crse, &ccomp, ratio)) return 1;
  if (fine->lev->boxes.empty() || !crse) return 0;
  if (interp_type == 1 && ratio == 2 && !pa_opt().force_fallbacks) {
    const FpPlan* Pp = fp_parent_plan(ctx, fine->lev, crse->lev, ng);
    if (!Pp) return 1;
    const FpPlan& P = *Pp;
    const pa_level* F = fine->lev;
    if (P.n > 0)
      hipLaunchKernelGGL(k_fp_do, dim3((unsigned)((P.n + 255) / 256)), dim3(256), 0, ctx->stream, F->view, fine->view, crse->lev->view, crse->view, comp, ccomp - comp,
                         ncomp, (const int4*)P.d_items, P.n, ctx->d_flags);
    PA_HIP(hipGetLastError());
    return 0;
  }
  dim3 grid((unsigned)((min_shell2(fine->lev, ng) + 255) / 256), (unsigned)fine->lev->boxes.size());
  hipLaunchKernelGGL(k_fillpatch2, grid, dim3(256), 0, ctx->stream, fine->lev->view, fine->view, crse->lev->view, crse->view, comp, ccomp - comp, ncomp, ng, ratio,
                     interp_type, ctx->d_flags);
  PA_HIP(hipGetLastError());
  return 0;
}

// The ghost fill of a whole hierarchy -- filterPlt.cpp:159-203 (FillBoundary, FillPatchTwoLevels, foextrap per level) and
// isosurface.cpp:1468-1524 (FillBoundary + FillPatchTwoLevels with PCInterp) -- in THREE launches instead of three per level:
// FillBoundary of every level, FillPatchTwoLevels of every level pair, foextrap of every level.  Legal because no step of a
// level reads what another level's step writes: FillBoundary and FillPatchTwoLevels read VALID cells only (the coarse values
// through the owner map, the nearest cell inside the domain beyond a wall) and write disjoint ghost cells; foextrap reads the
// ghost cells of its own FAB that the two earlier launches filled.  Results identical to the per-level calls.  Levels sharded
// over ranks take the per-level calls (their cross-rank halves are exchanges of their own).
extern "C" int pa_fill_ghosts_hierarchy(pa_ctx* ctx, int nlev, pa_mf* const* mfs, int comp, int ncomp, const int32_t* ngs, int ratio, int interp_type, int foextrap) {
  PaBind bind_(ctx);
  if (!ctx || nlev <= 0 || !mfs || !ngs) return pa_fail(ctx, "pa_fill_ghosts_hierarchy: null argument");
  if (ratio < 2 || ratio > 16) return pa_fail(ctx, "pa_fill_ghosts_hierarchy: refinement ratio must be 2 .. 16");
  if (interp_type != 0 && interp_type != 1) return pa_fail(ctx, "pa_fill_ghosts_hierarchy: interp_type must be 0 (pc) or 1 (cell-conservative linear)");
  bool sharded = false;
  for (int l = 0; l < nlev; ++l) {
    if (!mfs[l]) return pa_fail(ctx, "pa_fill_ghosts_hierarchy: null multifab");
    if (ngs[l] > mfs[l]->ng || ngs[l] < 0 || comp < 0 || comp + ncomp > mfs[l]->ncomp) return pa_fail(ctx, "pa_fill_ghosts_hierarchy: ng/component range");
    for (int d = 0; d < 3; ++d)
      if (mfs[l]->lev->is_per[d] && ngs[l] > mfs[l]->lev->domhi[d] - mfs[l]->lev->domlo[d] + 1) return pa_fail(ctx, "pa_fill_ghosts_hierarchy: ng larger than the periodic domain");
    sharded = sharded || mfs[l]->lev->nranks > 1;
  }
  if (sharded || pa_opt().force_fallbacks) {
    for (int l = 0; l < nlev; ++l) {
      if (pa_fill_boundary(ctx, mfs[l], comp, ncomp, ngs[l])) return 1;
      if (l > 0 && pa_fillpatch_two_levels(ctx, mfs[l], mfs[l - 1], comp, ncomp, ngs[l], ratio, interp_type)) return 1;
      if (foextrap && pa_foextrap(ctx, mfs[l], comp, ncomp, ngs[l])) return 1;
    }
    return 0;
  }
  {
    ProfScope prof(ctx, PA_TAG_FILL);
    std::vector<int> g(ngs, ngs + nlev);
    if (pa_fill_boundary_local_batch_ngs(ctx, nlev, mfs, comp, ncomp, g.data())) return 1;
  }
  if (interp_type == 1 && ratio == 2 && !pa_opt().force_fallbacks) {
    for (int l0 = 1; l0 < nlev; l0 += PA_MAXB) {
      FpdBatch Bt;
      Bt.n = 0;
      Bt.wg0[0] = 0;
      for (int l = l0; l < nlev && l < l0 + PA_MAXB; ++l) {
        if (ngs[l] == 0 || mfs[l]->lev->boxes.empty()) continue;
        const FpPlan* P = fp_parent_plan(ctx, mfs[l]->lev, mfs[l - 1]->lev, ngs[l]);
        if (!P) return 1;
        if (P->n <= 0) continue;
        Bt.a[Bt.n] = FpdLev{mfs[l]->lev->view, mfs[l]->view, mfs[l - 1]->lev->view, mfs[l - 1]->view, comp, 0, ncomp, (const int4*)P->d_items, P->n};
        Bt.wg0[Bt.n + 1] = Bt.wg0[Bt.n] + (unsigned)((P->n + 255) / 256);
        ++Bt.n;
      }
      if (Bt.n) hipLaunchKernelGGL(k_fp_do_levels, dim3(Bt.wg0[Bt.n]), dim3(256), 0, ctx->stream, Bt, ctx->d_flags);
    }
  } else {
    for (int l0 = 1; l0 < nlev; l0 += PA_MAXB) {
      LevBatch<Fp2Args> Bt;
      long long ms = 0;
      for (int l = l0; l < nlev && l < l0 + PA_MAXB; ++l) {
        if (ngs[l] == 0 || mfs[l]->lev->boxes.empty()) continue;
        Bt.a[Bt.n] = Fp2Args{mfs[l]->lev->view, mfs[l]->view, mfs[l - 1]->lev->view, mfs[l - 1]->view, comp, 0, ncomp, ngs[l], ratio, interp_type};
        Bt.ycum[Bt.n + 1] = Bt.ycum[Bt.n] + (int)mfs[l]->lev->boxes.size();
        ++Bt.n;
        ms = std::max(ms, min_shell2(mfs[l]->lev, ngs[l]));
      }
      if (Bt.n) hipLaunchKernelGGL(k_fillpatch2_levels, dim3((unsigned)((ms + 255) / 256), (unsigned)Bt.ycum[Bt.n]), dim3(256), 0, ctx->stream, Bt, ctx->d_flags);
    }
  }
  PA_HIP(hipGetLastError());
  if (foextrap) {
    for (int l0 = 0; l0 < nlev; l0 += PA_MAXB) {
      LevBatch<FoArgs> Bt;
      long long ms = 0;
      for (int l = l0; l < nlev && l < l0 + PA_MAXB; ++l) {
        if (ngs[l] == 0 || mfs[l]->lev->boxes.empty()) continue;
        bool wall = false;  // a level without a non-periodic direction has nothing to extrapolate
        for (int d = 0; d < 3; ++d) wall = wall || !mfs[l]->lev->is_per[d];
        if (!wall) continue;
        Bt.a[Bt.n] = FoArgs{mfs[l]->lev->view, mfs[l]->view, comp, ncomp, ngs[l]};
        Bt.ycum[Bt.n + 1] = Bt.ycum[Bt.n] + (int)mfs[l]->lev->boxes.size();
        ++Bt.n;
        ms = std::max(ms, min_shell2(mfs[l]->lev, ngs[l]));
      }
      if (Bt.n) hipLaunchKernelGGL(k_foextrap_levels, dim3((unsigned)((ms + 255) / 256), (unsigned)Bt.ycum[Bt.n]), dim3(256), 0, ctx->stream, Bt);
    }
    PA_HIP(hipGetLastError());
  }
  return 0;
}


