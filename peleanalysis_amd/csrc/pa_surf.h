// pa_surf.h -- the surface handle that pa_surfcut.hip (slice, trim, area), pa_surfjoin.hip (merge, scale, product, select) and
// pa_surfsmooth.hip (smooth) share: struct pa_surf and the helpers that size its scratch, scan, sort and launch.  A pa_surf holds the
// nodes COMPONENT-MAJOR, V[c * nN + n], and the elements as 0-based int triples F[3 * e + q].
#pragma once
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "pa_internal.h"

typedef unsigned long long u64;

struct DevBufG {  // grow-only device scratch
  void* p = nullptr;
  size_t cap = 0;
};

struct pa_surf {
  pa_ctx* ctx = nullptr;
  long long nN = 0, nE = 0;
  int nc = 0;
  double* V = nullptr;
  int* F = nullptr;
  // the last slice (device memory, valid until the next slice, trim, merge, scale or smooth)
  bool sliced = false;
  long long nsegs = 0, nverts = 0;
  int64_t rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  enum { B_CS, B_FLAG, B_POS, B_SRC, B_UKEY, B_DKEY, B_RIDX, B_UKS, B_RS, B_HEAD, B_HSCAN, B_REQU, B_HSTART, B_VDK, B_VU, B_VDKS, B_PERM, B_RANK, B_LEN, B_OFF,
         B_SEGS, B_ADJ, B_OFFOUT, B_PAIRS, B_VERTS, B_TMP, B_AUX,
         B_SM_OFF, B_SM_ADJ, B_SM_W, B_SM_WSUM, B_SM_Q0, B_SM_Q1,  // the last smooth (pa_surfsmooth.hip): no other step writes these
         B_N };
  int sm_q = 0;  // which of B_SM_Q0 / B_SM_Q1 holds q after the last iteration
  DevBufG buf[B_N];
};

namespace {
// the item of this thread in a one-thread-per-item launch.  Counts go up to 2^31 - 1, so the last block's index can pass INT_MAX: it is
// formed in 64 bits and clamped to INT_MAX, which no count is below, so the callers' `>= n` guards hold it off
__device__ __forceinline__ int sc_item() {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  return t > 0x7fffffffLL ? 0x7fffffff : (int)t;
}
inline dim3 sc_grid(long long n) { return dim3((unsigned)((n + 255) / 256)); }

int sf_fail(pa_ctx* ctx, const std::string& m) { if (ctx) ctx->err = m; return -1; }
#define SF_HIP(call)                                                                                          \
  do {                                                                                                        \
    const hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) return sf_fail(S->ctx, std::string("pa_surf: " #call ": ") + hipGetErrorString(e_)); \
  } while (0)
#define SF_LAUNCH(kernel, n, ...)                                                               \
  do {                                                                                          \
    if ((n) > 0) { hipLaunchKernelGGL(kernel, sc_grid((n)), dim3(256), 0, st, __VA_ARGS__); ++launches; } \
  } while (0)

template <class T> int sf_need(pa_surf* S, int which, size_t n, T*& out) {
  DevBufG& b = S->buf[which];
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  if (bytes > b.cap) {
    if (b.p) SF_HIP(hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    SF_HIP(hipMalloc(&b.p, bytes));
    b.cap = bytes;
  }
  out = (T*)b.p;
  return 0;
}
int sf_scan(pa_surf* S, const int* in, int* out, size_t n) {
  size_t tb = 0;
  SF_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, 0, n, rocprim::plus<int>(), S->ctx->stream));
  unsigned char* tmp = nullptr;
  if (sf_need(S, pa_surf::B_TMP, tb + 256, tmp)) return -1;
  SF_HIP(rocprim::exclusive_scan(tmp, tb, in, out, 0, n, rocprim::plus<int>(), S->ctx->stream));
  return 0;
}
int sf_sort_pairs(pa_surf* S, const u64* kin, u64* kout, const int* vin, int* vout, size_t n, int end_bit) {
  size_t tb = 0;
  SF_HIP(rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, n, 0, end_bit, S->ctx->stream));
  unsigned char* tmp = nullptr;
  if (sf_need(S, pa_surf::B_TMP, tb + 256, tmp)) return -1;
  SF_HIP(rocprim::radix_sort_pairs(tmp, tb, kin, kout, vin, vout, n, 0, end_bit, S->ctx->stream));
  return 0;
}
// the total of an exclusive scan of 0 / 1 flags: scan[n - 1] + flag[n - 1]
int sf_total(pa_surf* S, const int* flag, const int* scan, long long n, long long* tot) {
  *tot = 0;
  if (n <= 0) return 0;
  int last[2];
  SF_HIP(hipMemcpyAsync(&last[0], scan + (n - 1), sizeof(int), hipMemcpyDeviceToHost, S->ctx->stream));
  SF_HIP(hipMemcpyAsync(&last[1], flag + (n - 1), sizeof(int), hipMemcpyDeviceToHost, S->ctx->stream));
  SF_HIP(hipStreamSynchronize(S->ctx->stream));
  *tot = (long long)last[0] + last[1];
  return 0;
}
bool sf_own(pa_ctx* ctx, const pa_surf* S) { return ctx && S && S->ctx == ctx; }
}  // namespace
