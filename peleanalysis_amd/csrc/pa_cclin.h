// pa_cclin.h -- the cell-conservative linear interpolant of FillPatchTwoLevels (mf_cell_cons_lin_interp_mcslope +
// mf_cell_cons_lin_interp, AMReX, recalled; restated in oracle/pa_oracle.c orc_fillpatch_two_levels): ONE copy of the
// arithmetic for everything that interpolates a coarse level onto fine cells -- the ghost-shell kernels of pa_filter.hip
// (k_fillpatch2, k_fp_do) and the resampling kernel of pa_resample.hip.  Same operations on the same operands in the same
// order wherever it is used (-ffp-contract=off), so their results agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

// Limited slopes and the common factor of one coarse parent.  get(n) = coarse value of neighbour n = (dz + 1) * 9 + (dy + 1) * 3
// + (dx + 1) (13 = the parent itself = u0; beyond a non-periodic wall the nearest cell inside the domain, filterPlt.cpp:164-173):
// the six face neighbours are always asked for, all 27 only where a slope is not zero.  Central slopes limited by df / db, one
// factor alpha for the three directions with dumax = sum |s_d| (r - 1) / (2 r).
// UNROLL: the 27-value pass as straight-line code (a caller that holds the values in registers) or as a loop (a caller whose get
// is a walk through the owner map).
template <bool UNROLL, typename G>
__device__ __forceinline__ void ccl_slopes(G&& get, const double u0, const int r, double sl[3], double& alpha) {
#pragma unroll
  for (int d = 0; d < 3; ++d) {  // (unrolled: a run-time stride sends a caller's 27 values through scratch memory)
    const int st = d == 0 ? 1 : (d == 1 ? 3 : 9);
    const double um = get(13 - st), up = get(13 + st);
    const double dc = 0.5 * (up - um);
    const double df = 2.0 * (up - u0), db = 2.0 * (u0 - um);
    double sx = (df * db >= 0.0) ? fmin(fabs(df), fabs(db)) : 0.0;
    sx = copysign(1.0, dc) * fmin(sx, fabs(dc));
    sl[d] = sx;
  }
  alpha = 1.0;
  if (sl[0] != 0.0 || sl[1] != 0.0 || sl[2] != 0.0) {
    const double dumax = fabs(sl[0]) * (double)(r - 1) / (double)(2 * r) + fabs(sl[1]) * (double)(r - 1) / (double)(2 * r) +
                         fabs(sl[2]) * (double)(r - 1) / (double)(2 * r);
    double umax = u0, umin = u0;
    auto take = [&](int n) {  // dz, dy, dx ascending, dx fastest
      const double v = get(n);
      umin = v < umin ? v : umin;
      umax = v > umax ? v : umax;
    };
    if constexpr (UNROLL) {
#pragma unroll
      for (int n = 0; n < 27; ++n) take(n);
    } else {
      for (int n = 0; n < 27; ++n) take(n);
    }
    if (dumax * alpha > (umax - u0)) alpha = (umax - u0) / dumax;
    if (dumax * alpha > (u0 - umin)) alpha = (u0 - umin) / dumax;
  }
}

// the child at offset rem[d] = i_d - r * ic_d (0 .. r - 1) inside its parent: xoff = (rem + 0.5) / r - 0.5
__device__ __forceinline__ double ccl_child(const double u0, const double sl[3], const double alpha, const int rem[3], const int r) {
  double acc = u0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double xoff = ((double)rem[d] + 0.5) / (double)r - 0.5;
    acc += xoff * (sl[d] * alpha);
  }
  return acc;
}
