// pa_resample.h -- the per-parent device code that pa_resample.hip (running sum of avgPlotfiles) and pa_flatten.hip (the general
// route of pa_flatten_level) share: ONE copy of "the file's value where it holds the cell, else the interpolant of the coarser work
// multifab", so that the two produce the same bits.
#pragma once
#include "pa_internal.h"
#include "pa_cclin.h"
#include <limits>

#define PA_RS_MAXV 16  // variables per launch (the component map travels in the kernel arguments)


struct RsArgs {
  DLevelView U;   // target level: boxes of the running sum and of T
  DMFView S, T;   // running sum; this level's work multifab (has_t)
  DLevelView F;   // the file's level (has_f)
  DMFView FM;
  DLevelView UC;  // coarser target level and its work multifab (has_c)
  DMFView TC;
  int has_t, has_f, has_c, gt, interp, nvar;
  int comp[PA_RS_MAXV];  // file component of variable v
};

// One coarse parent (thread t of box b) of the target level.  SUM: the valid cells are added to the running sum A.S (pa_resample.hip);
// without it only A.T is written -- V(f, l) itself, the flatten of pa_flatten.hip's general route -- and A.S is not touched.
template <int R, bool SUM>
__device__ __forceinline__ void rs_parent(const RsArgs& A, const int b, const unsigned t, unsigned long long* nosrc) {
  constexpr int NCH = R * R * R;
  const DBox B = A.U.boxes[b];
  const int g = A.gt;
  int clo[3], cn[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    clo[d] = coarsen_idx(B.lo[d] - g, R);
    cn[d] = coarsen_idx(B.hi[d] + g, R) - clo[d] + 1;
  }
  if (t >= (unsigned)cn[0] * (unsigned)cn[1] * (unsigned)cn[2]) return;  // (a grown box is far below 2^32 parents)
  const unsigned row = t / (unsigned)cn[0];
  const int qc[3] = {clo[0] + (int)(t - row * (unsigned)cn[0]), clo[1] + (int)(row % (unsigned)cn[1]), clo[2] + (int)(row / (unsigned)cn[1])};

  // the children inside the grown box / inside the valid box, and which of them the file holds (at their canonical cells)
  unsigned long long in = 0, valid = 0, have = 0;
  for (int c = 0; c < NCH; ++c) {
    const int q[3] = {R * qc[0] + c % R, R * qc[1] + (c / R) % R, R * qc[2] + c / (R * R)};
    bool i_ = true, v_ = true;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      i_ = i_ && q[d] >= B.lo[d] - g && q[d] <= B.hi[d] + g;
      v_ = v_ && q[d] >= B.lo[d] && q[d] <= B.hi[d];
    }
    if (!i_) continue;
    in |= 1ull << c;
    if (v_) valid |= 1ull << c;
    if (A.has_f) {
      int p[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] = A.U.is_per[d] ? q[d] : min(max(q[d], A.U.domlo[d]), A.U.domhi[d]);
      wrap_cell(A.U, p);
      if (owner_of(A.F, p) >= 0) have |= 1ull << c;
    }
  }
  if (!in) return;

  // the parent in T_{l-1}: the coarse box under the valid cell of B nearest to the children; the parent (clamped into the
  // domain across a wall) and its neighbours lie in that box grown by its ghost layers (checked: pa_resample_add_file_level)
  const unsigned long long miss = in & ~have;
  bool src = miss == 0;
  const double* p0 = nullptr;
  int sy = 0, sz = 0, qcc[3] = {qc[0], qc[1], qc[2]};
  long long cstride = 0;
  if (miss && R > 1 && A.has_c) {
    int ca[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      ca[d] = coarsen_idx(min(max(R * qc[d], B.lo[d]), B.hi[d]), R);
      if (!A.UC.is_per[d]) qcc[d] = min(max(qc[d], A.UC.domlo[d]), A.UC.domhi[d]);
    }
    const int cb = owner_of(A.UC, ca);
    if (cb >= 0) {
      const DBox CB = A.UC.boxes[cb];
      const int need = A.interp == 1 ? 1 : 0;
      bool ok = true;
#pragma unroll
      for (int d = 0; d < 3; ++d) ok = ok && qcc[d] - need >= CB.lo[d] - A.TC.ng && qcc[d] + need <= CB.hi[d] + A.TC.ng;
      if (ok) {
        src = true;
        sy = CB.hi[0] - CB.lo[0] + 1 + 2 * A.TC.ng;
        sz = sy * (CB.hi[1] - CB.lo[1] + 1 + 2 * A.TC.ng);  // a coarse FAB is far below 2^31 cells
        p0 = A.TC.data + A.TC.off[cb] + fab_index(CB, A.TC.ng, A.TC.ncomp, 0, qcc[0], qcc[1], qcc[2]);
        cstride = fab_index(CB, A.TC.ng, A.TC.ncomp, 1, qcc[0], qcc[1], qcc[2]) - fab_index(CB, A.TC.ng, A.TC.ncomp, 0, qcc[0], qcc[1], qcc[2]);
      }
    }
  }
  if (!src) atomicAdd(nosrc, (unsigned long long)__popcll(miss));  // cells without source data: they get a NaN

  double* const sb = SUM ? A.S.data + A.S.off[b] : nullptr;
  double* const tb = A.has_t ? A.T.data + A.T.off[b] : nullptr;
  for (int v = 0; v < A.nvar; ++v) {
    double u0 = 0.0, sl[3] = {0.0, 0.0, 0.0}, alpha = 1.0;
    if (miss && p0) {
      const double* pv = p0 + (long long)v * cstride;
      u0 = pv[0];
      if (A.interp == 1) {
        double w[27];  // index (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
#pragma unroll
        for (int n = 0; n < 27; ++n) w[n] = pv[(n / 9 - 1) * sz + ((n / 3) % 3 - 1) * sy + (n % 3 - 1)];
        ccl_slopes<true>([&](int n) { return w[n]; }, u0, R, sl, alpha);
      }
    }
    for (int c = 0; c < NCH; ++c) {
      if (!((in >> c) & 1ull)) continue;
      const int q[3] = {R * qc[0] + c % R, R * qc[1] + (c / R) % R, R * qc[2] + c / (R * R)};
      int pu[3], p[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) p[d] = pu[d] = A.U.is_per[d] ? q[d] : min(max(q[d], A.U.domlo[d]), A.U.domhi[d]);
      double val;
      if ((have >> c) & 1ull) {
        wrap_cell(A.U, p);
        const int fb = owner_of(A.F, p);
        val = A.FM.data[A.FM.off[fb] + fab_index(A.F.boxes[fb], A.FM.ng, A.FM.ncomp, A.comp[v], p[0], p[1], p[2])];
      } else if (!p0) {
        val = std::numeric_limits<double>::quiet_NaN();
      } else if (A.interp == 1) {
        const int rem[3] = {pu[0] - R * qcc[0], pu[1] - R * qcc[1], pu[2] - R * qcc[2]};
        val = ccl_child(u0, sl, alpha, rem, R);
      } else {
        val = u0;
      }
      if (tb) tb[fab_index(B, A.T.ng, A.T.ncomp, v, q[0], q[1], q[2])] = val;
      if constexpr (SUM) {
        if ((valid >> c) & 1ull) {
          double* s = sb + fab_index(B, A.S.ng, A.S.ncomp, v, q[0], q[1], q[2]);
          *s = *s + val;
        }
      }
    }
  }
}
