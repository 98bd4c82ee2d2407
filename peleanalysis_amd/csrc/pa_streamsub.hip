// pa_streamsub.hip -- subsetting a stream directory by surface elements (PeleAnalysis Src/streamSub.cpp) on gfx950: the element list
// from the seed points (new: the docs' "by physical location of the streamline seed point"), the selected connectivity (:337-343),
// the boxes it needs (:375-395), the new node numbers (:417-425), the connectivity in them (:439-441) and the copy of the kept boxes.
// INTENT, NOT TEXT: :341 writes every selected element over slots 0 .. nodesPerElt-1 of faceData and :385 then reads that array at the
// FILE's element offset; the text is defined for sElt=0 nElt=1 only.  Built here: faceSel[j * npe + i] = fileFace[E[j] * npe + i].
// Layout: that of pa_streamsel.hip / pa_tubestats.hip -- box g holds ncomp components of ni * nj doubles at ncomp * off_g, component-
// major, i (line) fastest, then j; a pa_ssel holds (ni, nj, jlo, off) per box and node id -> (box, line).  The compact buffer has the
// same layout over the kept boxes: box b' at ncompOut * off'_b'.
// DETERMINISM: no atomic, floating-point or integer, anywhere.  Every count and position is an integer scan (of the element flags: the
// three-launch compaction of DESIGN 3.17; of the box flags, line, point and chunk counts: int64), the flag of an element is recomputed
// by the scatter, and the only race -- several elements flagging one box -- stores the same value 1.  The copy moves 64-bit integers:
// NaN payloads, -0.0 and infinities survive.  Two runs give the same bytes.
#include "pa_internal.h"
#include "pa_streamsel.h"

#include <algorithm>

struct pa_ssub {
  pa_ctx* ctx = nullptr;
  pa_ssel* sel = nullptr;
  long long nElts = 0, nSel = 0;
  int npe = 0;
  long long nBoxes = 0, nNodesNew = 0, nPts = 0, nChunks = 0;
  int* d_flag = nullptr;         // [nbt] 1: a node of faceSel lies in the box
  long long* d_scan = nullptr;   // [nbt + 1][4] exclusive over the kept boxes: new box index, node offset, point offset, chunk offset
  long long* d_bsum = nullptr;   // [nblk][4], [nblk + 1][4]: the box scan beyond one workgroup
  long long* d_boff = nullptr;
  int* d_face = nullptr;         // [nSel][npe] the selected connectivity, in the new numbers once the plan is built
  int* d_newnum = nullptr;       // [nNodes] new number of node id n + 1, 0 where its box is not kept
  int2* d_chunk = nullptr;       // [nChunks] (box g, chunk k): doubles k * SB_CHUNK .. of every component run of box g
  int* d_err = nullptr;
  long long rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace {

#define SB_BLOCK 256
#define SB_CHUNK 2048
#define PA_SSUB_MAXCOMPS 64

struct SbTab {
  const long long* box;
  const int* node;
  long long nNodes;
};
struct SbBounds { double lo[3], hi[3]; };
struct SbComps { int n; int comp[PA_SSUB_MAXCOMPS]; };

// the seed test of element e: every node's point (components 0, 1, 2 at j = 0 of its line) inside lo .. hi, literal <= (NaN fails).
// An id outside 1 .. nNodes, or a line whose j range lacks 0, reads nothing, drops the element and fails the call (err, where not null).
__device__ __forceinline__ int sb_seed_keep(const SbTab& T, const int* face, int npe, long long nElts, const double* data, int ncomp, const SbBounds& Q, long long e, int* err) {
  if (e >= nElts) return 0;
  int keep = 1;
  for (int i = 0; i < npe; ++i) {
    const int id = face[e * npe + i];
    if (id < 1 || id > T.nNodes) {
      if (err) *err = 1;
      return 0;
    }
    const int b = T.node[2 * (long long)(id - 1)], line = T.node[2 * (long long)(id - 1) + 1];
    const long long* B = T.box + 4 * (long long)b;
    const long long ni = B[0], nj = B[1], jlo = B[2];
    if (jlo > 0 || jlo + nj - 1 < 0) {
      if (err) *err = 2;
      return 0;
    }
    const long long base = (long long)ncomp * B[3] + (0 - jlo) * ni + line;
    for (int d = 0; d < 3; ++d) {
      const double x = data[base + (long long)d * ni * nj];
      if (!(Q.lo[d] <= x && x <= Q.hi[d])) keep = 0;
    }
  }
  return keep;
}
// inclusive scan of one int per thread over the workgroup (SB_BLOCK threads); every thread calls it
__device__ __forceinline__ int sb_block_scan(int v, int* s) {
  const int tid = threadIdx.x;
  s[tid] = v;
  __syncthreads();
  for (int off = 1; off < SB_BLOCK; off <<= 1) {
    const int t = tid >= off ? s[tid - off] : 0;
    __syncthreads();
    s[tid] += t;
    __syncthreads();
  }
  return s[tid];
}
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_seed_count(SbTab T, const int* face, int npe, long long nElts, const double* data, int ncomp, SbBounds Q, int* bsum, int* err) {
  __shared__ int s[SB_BLOCK];
  const long long e = blockIdx.x * (long long)SB_BLOCK + threadIdx.x;
  const int inc = sb_block_scan(sb_seed_keep(T, face, npe, nElts, data, ncomp, Q, e, err), s);
  if (threadIdx.x == SB_BLOCK - 1) bsum[blockIdx.x] = inc;
}
// exclusive scan of n counts by ONE workgroup, 16 K counts a pass (one count per SB_BLOCK elements); out[n] = the total
#define SB_SCAN_PER 16
__global__ __launch_bounds__(1024) void k_ssub_scan(const int* cnt, long long* out, long long n) {
  __shared__ long long s[1024];
  __shared__ long long carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (long long base = 0; base < n; base += 1024 * SB_SCAN_PER) {
    const long long q0 = base + (long long)tid * SB_SCAN_PER;
    long long mine = 0;
    for (int k = 0; k < SB_SCAN_PER; ++k)
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
    for (int k = 0; k < SB_SCAN_PER; ++k)
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
// the kept elements in ascending file order: the flag is computed again, not stored.  Where the count pass raised its error flag (the
// same elements, so the same finding) nothing is stored: a refused call leaves elts as it was
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_seed_scatter(SbTab T, const int* face, int npe, long long nElts, const double* data, int ncomp, SbBounds Q, const long long* boff, int* elts,
                                                               const int* err) {
  __shared__ int s[SB_BLOCK];
  const long long e = blockIdx.x * (long long)SB_BLOCK + threadIdx.x;
  const int refused = *err;
  const int keep = sb_seed_keep(T, face, npe, nElts, data, ncomp, Q, e, nullptr);
  const int inc = sb_block_scan(keep, s);
  if (keep && !refused) elts[boff[blockIdx.x] + (inc - 1)] = (int)e;
}

// :337-343 as intended, and the flags of :380-388.  An element outside 0 .. nElts-1 or a node id outside 1 .. nNodes reads nothing more.
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_face(SbTab T, long long nElts, int npe, const int* face, long long nSel, const int* elts, int* faceSel, int* flag, int* err) {
  const long long t = blockIdx.x * (long long)SB_BLOCK + threadIdx.x;
  if (t >= nSel * npe) return;
  const long long j = t / npe;
  const int i = (int)(t - j * npe);
  const int e = elts[j];
  if (e < 0 || e >= nElts) {
    faceSel[t] = 0;
    *err = 1;
    return;
  }
  const int id = face[(long long)e * npe + i];
  if (id < 1 || id > T.nNodes) {
    faceSel[t] = 0;
    *err = 2;
    return;
  }
  faceSel[t] = id;
  flag[T.node[2 * (long long)(id - 1)]] = 1;  // the same value from every thread that names the box
}

// what box g adds to the four scans: 1, its listed lines, its points, its chunks -- nothing when it is not needed
__device__ __forceinline__ void sb_box_vals(const int* flag, const long long* box, const long long* nline, long long g, long long nbt, long long v[4]) {
  v[0] = v[1] = v[2] = v[3] = 0;
  if (g < nbt && flag[g]) {
    const long long np = box[4 * g] * box[4 * g + 1];
    v[0] = 1;
    v[1] = nline[g];
    v[2] = np;
    v[3] = (np + SB_CHUNK - 1) / SB_CHUNK;
  }
}
// inclusive scan of four int64 per thread over the workgroup
__device__ __forceinline__ void sb_block_scan4(long long v[4], long long (*s)[SB_BLOCK]) {
  const int tid = threadIdx.x;
  for (int q = 0; q < 4; ++q) s[q][tid] = v[q];
  __syncthreads();
  for (int off = 1; off < SB_BLOCK; off <<= 1) {
    long long t[4];
    for (int q = 0; q < 4; ++q) t[q] = tid >= off ? s[q][tid - off] : 0;
    __syncthreads();
    for (int q = 0; q < 4; ++q) s[q][tid] += t[q];
    __syncthreads();
  }
  for (int q = 0; q < 4; ++q) v[q] = s[q][tid];
}
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_box_count(const int* flag, const long long* box, const long long* nline, long long nbt, long long* bsum) {
  __shared__ long long s[4][SB_BLOCK];
  long long v[4];
  sb_box_vals(flag, box, nline, blockIdx.x * (long long)SB_BLOCK + threadIdx.x, nbt, v);
  sb_block_scan4(v, s);
  if (threadIdx.x == SB_BLOCK - 1)
    for (int q = 0; q < 4; ++q) bsum[4 * (long long)blockIdx.x + q] = v[q];
}
// exclusive scan of the n block sums by one workgroup, SB_BLOCK a pass; boff[n] = the totals
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_box_sums(const long long* bsum, long long* boff, long long n) {
  __shared__ long long s[4][SB_BLOCK];
  __shared__ long long carry[4];
  const int tid = threadIdx.x;
  if (tid < 4) carry[tid] = 0;
  __syncthreads();
  for (long long base = 0; base < n; base += SB_BLOCK) {
    const long long q0 = base + tid;
    long long mine[4], v[4];
    for (int q = 0; q < 4; ++q) v[q] = mine[q] = q0 < n ? bsum[4 * q0 + q] : 0;
    sb_block_scan4(v, s);
    if (q0 < n)
      for (int q = 0; q < 4; ++q) boff[4 * q0 + q] = carry[q] + v[q] - mine[q];
    __syncthreads();
    if (tid == SB_BLOCK - 1)
      for (int q = 0; q < 4; ++q) carry[q] += v[q];
    __syncthreads();
  }
  if (tid < 4) boff[4 * n + tid] = carry[tid];
}
// scan[g] = what the kept boxes before g hold; scan[nbt] = the totals.  boff == nullptr: the grid is one workgroup
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_box_apply(const int* flag, const long long* box, const long long* nline, long long nbt, const long long* boff, long long* scan) {
  __shared__ long long s[4][SB_BLOCK];
  const long long g = blockIdx.x * (long long)SB_BLOCK + threadIdx.x;
  long long mine[4], v[4];
  sb_box_vals(flag, box, nline, g, nbt, mine);
  for (int q = 0; q < 4; ++q) v[q] = mine[q];
  sb_block_scan4(v, s);
  if (g >= nbt) return;
  for (int q = 0; q < 4; ++q) {
    const long long incl = v[q] + (boff ? boff[4 * (long long)blockIdx.x + q] : 0);
    scan[4 * g + q] = incl - mine[q];
    if (g == nbt - 1) scan[4 * nbt + q] = incl;
  }
}

// :417-425: 1-based, consecutive over the kept boxes in level -> box -> position order
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_newnum(SbTab T, const int* flag, const long long* scan, int* newnum) {
  const long long n = blockIdx.x * (long long)SB_BLOCK + threadIdx.x;
  if (n >= T.nNodes) return;
  const int b = T.node[2 * n];
  newnum[n] = flag[b] ? (int)(scan[4 * (long long)b + 1] + T.node[2 * n + 1] + 1) : 0;
}
// :439-441
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_remap(int* faceSel, long long n, const int* newnum) {
  const long long t = blockIdx.x * (long long)SB_BLOCK + threadIdx.x;
  if (t < n) faceSel[t] = newnum[faceSel[t] - 1];
}
// chunk q belongs to the last box whose chunk offset is <= q (boxes that are not kept are empty ranges, never the last)
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_chunks(const long long* scan, int nbt, long long nChunks, int2* chunk) {
  const long long q = blockIdx.x * (long long)SB_BLOCK + threadIdx.x;
  if (q >= nChunks) return;
  int lo = 0, hi = nbt - 1;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (scan[4 * (long long)mid + 3] <= q) lo = mid;
    else hi = mid - 1;
  }
  chunk[q] = make_int2(lo, (int)(q - scan[4 * (long long)lo + 3]));
}

// one workgroup copies one chunk (at most SB_CHUNK doubles) of one component run of one kept box: contiguous on both sides.  16-byte
// accesses where source and destination share the alignment (a run of an odd number of doubles shifts the next one by 8 bytes: then a
// head of one double comes first), 8-byte accesses where they do not.  The values move as integers.
__global__ __launch_bounds__(SB_BLOCK) void k_ssub_gather(const long long* box, const long long* scan, const int2* chunk, const unsigned long long* data, int ncomp, SbComps S,
                                                         unsigned long long* out, int ncompOut, int c0) {
  const int2 r = chunk[blockIdx.x];
  const int c = blockIdx.y, tid = threadIdx.x;
  const long long* B = box + 4 * (long long)r.x;
  const long long np = B[0] * B[1], at = (long long)r.y * SB_CHUNK;
  const long long len = (np - at < SB_CHUNK) ? np - at : SB_CHUNK;
  const unsigned long long* src = data + (long long)ncomp * B[3] + (long long)S.comp[c] * np + at;
  unsigned long long* dst = out + (long long)ncompOut * scan[4 * (long long)r.x + 2] + (long long)(c0 + c) * np + at;
  const int ms = (int)(((unsigned long long)src >> 3) & 1), md = (int)(((unsigned long long)dst >> 3) & 1);
  if (ms != md) {
    for (long long q = tid; q < len; q += SB_BLOCK) dst[q] = src[q];
    return;
  }
  const long long head = ms, nbody = (len - head) / 2;
  const ulonglong2* s2 = (const ulonglong2*)(src + head);
  ulonglong2* d2 = (ulonglong2*)(dst + head);
  for (long long q = tid; q < nbody; q += SB_BLOCK) d2[q] = s2[q];
  if (tid == 0 && head) dst[0] = src[0];
  if (tid == SB_BLOCK - 1 && head + 2 * nbody < len) dst[len - 1] = src[len - 1];
}

inline dim3 sb_grid(long long n) { return dim3((unsigned)((n + SB_BLOCK - 1) / SB_BLOCK)); }
inline SbTab sb_tab(const pa_ssel* s) { return SbTab{s->d_box, s->d_node, s->nNodes}; }

// the checks of build_nodeMap the sister tools leave to the caller's tables: the ids of a box sit on its lines 0 .. nline-1, one each
// (then the new inside_nodes list of a kept box is a consecutive range).  Built once per handle.
bool sb_prepare(pa_ssel* s) {
  if (s->sub_state != 0) return s->sub_state > 0;
  auto refuse = [&](const std::string& m) {
    s->sub_state = -1;
    s->sub_why = m;
    return false;
  };
  s->nline.assign((size_t)s->nbt, 0);
  for (long long n = 0; n < s->nNodes; ++n) ++s->nline[(size_t)s->node[2 * (size_t)n]];
  std::vector<long long> first((size_t)s->nbt + 1, 0);
  for (int g = 0; g < s->nbt; ++g) first[(size_t)g + 1] = first[(size_t)g] + s->nline[(size_t)g];
  std::vector<char> seen((size_t)s->nNodes, 0);
  for (long long n = 0; n < s->nNodes; ++n) {
    const int b = s->node[2 * (size_t)n], i = s->node[2 * (size_t)n + 1];
    if (i >= s->nline[(size_t)b]) return refuse("node " + std::to_string(n + 1) + " sits on line " + std::to_string(i) + " of box " + std::to_string(b) + ", which lists " + std::to_string(s->nline[(size_t)b]) + " ids");
    char& m = seen[(size_t)(first[(size_t)b] + i)];
    if (m) return refuse("two node ids on line " + std::to_string(i) + " of box " + std::to_string(b));
    m = 1;
  }
  if (hipMalloc(&s->d_nline, sizeof(long long) * (size_t)s->nbt) != hipSuccess ||
      hipMemcpy(s->d_nline, s->nline.data(), sizeof(long long) * (size_t)s->nbt, hipMemcpyHostToDevice) != hipSuccess) {
    if (s->d_nline) (void)hipFree(s->d_nline);  // not a finding about the tables: the next call tries again
    s->d_nline = nullptr;
    s->sub_why = "device allocation or copy failed";
    return false;
  }
  s->sub_state = 1;
  return true;
}

}  // namespace

extern "C" int pa_ssub_select_seedbox(pa_ctx* ctx, pa_ssel* s, const double* data, int32_t ncomp, int64_t nElts, int32_t npe, const int32_t* face, const double lo[3], const double hi[3],
                                      int32_t* elts, int64_t* nsel, int64_t launch[4]) {
  PaBind bind_(ctx);
  if (!ctx || !s || s->ctx != ctx || !nsel || !lo || !hi || nElts < 0 || npe < 1) return pa_fail(ctx, "pa_ssub_select_seedbox: bad argument");
  if (ncomp < 3) return pa_fail(ctx, "pa_ssub_select_seedbox: the seed point needs components 0, 1 and 2 (the buffer holds " + std::to_string(ncomp) + ")");
  if (nElts >= (1LL << 31) - SB_BLOCK || nElts * npe >= (1LL << 40)) return pa_fail(ctx, "pa_ssub_select_seedbox: more than 2^31 elements");
  if (!sb_prepare(s)) return pa_fail(ctx, "pa_ssub_select_seedbox: " + s->sub_why);
  for (int g = 0; g < s->nbt; ++g) {
    const long long* B = &s->box[4 * (size_t)g];
    if (s->nline[(size_t)g] > 0 && (B[2] > 0 || B[2] + B[1] - 1 < 0))
      return pa_fail(ctx, "pa_ssub_select_seedbox: Str box " + std::to_string(g) + " (j = " + std::to_string(B[2]) + " .. " + std::to_string(B[2] + B[1] - 1) + ") has lines but no seed point j = 0");
  }
  *nsel = 0;
  const long long nblk = (nElts + SB_BLOCK - 1) / SB_BLOCK;
  if (launch) { launch[0] = nElts; launch[1] = nblk; launch[2] = (nblk + 1024 * SB_SCAN_PER - 1) / (1024 * SB_SCAN_PER); launch[3] = 0; }
  if (nElts == 0) return 0;
  if (!data || !face || !elts) return pa_fail(ctx, "pa_ssub_select_seedbox: null device array");
  SbBounds Q;
  for (int d = 0; d < 3; ++d) { Q.lo[d] = lo[d]; Q.hi[d] = hi[d]; }
  int* d_bsum = nullptr;
  long long* d_boff = nullptr;
  int* d_err = nullptr;
  auto release = [&]() {
    for (void* p : {(void*)d_bsum, (void*)d_boff, (void*)d_err})
      if (p) (void)hipFree(p);
  };
  if (hipMalloc(&d_bsum, sizeof(int) * (size_t)nblk) != hipSuccess || hipMalloc(&d_boff, sizeof(long long) * (size_t)(nblk + 1)) != hipSuccess || hipMalloc(&d_err, sizeof(int)) != hipSuccess ||
      hipMemsetAsync(d_err, 0, sizeof(int), ctx->stream) != hipSuccess) {
    release();
    return pa_fail(ctx, "pa_ssub_select_seedbox: device allocation failed");
  }
  hipLaunchKernelGGL(k_ssub_seed_count, sb_grid(nElts), dim3(SB_BLOCK), 0, ctx->stream, sb_tab(s), face, (int)npe, (long long)nElts, data, (int)ncomp, Q, d_bsum, d_err);
  hipLaunchKernelGGL(k_ssub_scan, dim3(1), dim3(1024), 0, ctx->stream, d_bsum, d_boff, nblk);
  hipLaunchKernelGGL(k_ssub_seed_scatter, sb_grid(nElts), dim3(SB_BLOCK), 0, ctx->stream, sb_tab(s), face, (int)npe, (long long)nElts, data, (int)ncomp, Q, d_boff, elts, d_err);
  long long n = 0;
  int err = 0;
  const bool ok = hipGetLastError() == hipSuccess && hipMemcpyAsync(&n, d_boff + nblk, sizeof n, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                  hipMemcpyAsync(&err, d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess && pa_sync(ctx) == 0;
  release();
  if (!ok) return pa_fail(ctx, "pa_ssub_select_seedbox: launch or copy failed");
  if (err == 1) return pa_fail(ctx, "pa_ssub_select_seedbox: the element table names a node id outside 1 .. " + std::to_string(s->nNodes));
  if (err) return pa_fail(ctx, "pa_ssub_select_seedbox: a line without a seed point j = 0");
  *nsel = n;
  if (launch) launch[3] = n;
  return 0;
}

extern "C" void pa_ssub_destroy(pa_ssub* p) {
  if (!p) return;
  PaBind bind_(p->ctx);
  for (void* q : {(void*)p->d_flag, (void*)p->d_scan, (void*)p->d_bsum, (void*)p->d_boff, (void*)p->d_face, (void*)p->d_newnum, (void*)p->d_chunk, (void*)p->d_err})
    if (q) (void)hipFree(q);
  delete p;
}

extern "C" pa_ssub* pa_ssub_plan(pa_ctx* ctx, pa_ssel* s, int64_t nElts, int32_t npe, const int32_t* face, int64_t nSel, const int32_t* elts) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  std::unique_ptr<pa_ssub> p;
  auto fail = [&](const std::string& m) -> pa_ssub* {
    pa_ssub_destroy(p.release());
    pa_fail(ctx, "pa_ssub_plan: " + m);
    return nullptr;
  };
  if (!s || s->ctx != ctx || nElts < 0 || npe < 1 || nSel < 0) return fail("bad argument");
  if (nSel == 0) return fail("no element is selected");
  if (!face || !elts) return fail("null device array");
  if (nElts >= (1LL << 31) || nSel * npe >= (1LL << 31) - SB_BLOCK) return fail("more than 2^31 selected element nodes");
  if (!sb_prepare(s)) return fail(s->sub_why);
  p.reset(new pa_ssub);
  p->ctx = ctx;
  p->sel = s;
  p->nElts = nElts;
  p->nSel = nSel;
  p->npe = npe;
  const long long nbt = s->nbt, nblk = (nbt + SB_BLOCK - 1) / SB_BLOCK, nf = nSel * npe;
  bool ok = hipMalloc(&p->d_flag, sizeof(int) * (size_t)nbt) == hipSuccess && hipMalloc(&p->d_scan, sizeof(long long) * 4 * (size_t)(nbt + 1)) == hipSuccess &&
            hipMalloc(&p->d_bsum, sizeof(long long) * 4 * (size_t)nblk) == hipSuccess && hipMalloc(&p->d_boff, sizeof(long long) * 4 * (size_t)(nblk + 1)) == hipSuccess &&
            hipMalloc(&p->d_face, sizeof(int) * (size_t)nf) == hipSuccess && hipMalloc(&p->d_newnum, sizeof(int) * (size_t)std::max<long long>(s->nNodes, 1)) == hipSuccess &&
            hipMalloc(&p->d_err, sizeof(int)) == hipSuccess;
  ok = ok && hipMemsetAsync(p->d_flag, 0, sizeof(int) * (size_t)nbt, ctx->stream) == hipSuccess && hipMemsetAsync(p->d_err, 0, sizeof(int), ctx->stream) == hipSuccess;
  if (!ok) return fail("device allocation failed");
  hipLaunchKernelGGL(k_ssub_face, sb_grid(nf), dim3(SB_BLOCK), 0, ctx->stream, sb_tab(s), (long long)nElts, (int)npe, face, (long long)nSel, elts, p->d_face, p->d_flag, p->d_err);
  const int path = nblk == 1 ? 1 : 2;  // 1: the box scan is one workgroup; 2: block sums, their scan, the blocks again
  if (path == 1) {
    hipLaunchKernelGGL(k_ssub_box_apply, dim3(1), dim3(SB_BLOCK), 0, ctx->stream, p->d_flag, s->d_box, s->d_nline, nbt, (const long long*)nullptr, p->d_scan);
  } else {
    hipLaunchKernelGGL(k_ssub_box_count, dim3((unsigned)nblk), dim3(SB_BLOCK), 0, ctx->stream, p->d_flag, s->d_box, s->d_nline, nbt, p->d_bsum);
    hipLaunchKernelGGL(k_ssub_box_sums, dim3(1), dim3(SB_BLOCK), 0, ctx->stream, p->d_bsum, p->d_boff, nblk);
    hipLaunchKernelGGL(k_ssub_box_apply, dim3((unsigned)nblk), dim3(SB_BLOCK), 0, ctx->stream, p->d_flag, s->d_box, s->d_nline, nbt, p->d_boff, p->d_scan);
  }
  long long tot[4] = {0, 0, 0, 0};
  int err = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(tot, p->d_scan + 4 * nbt, sizeof tot, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(&err, p->d_err, sizeof err, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || pa_sync(ctx) != 0)
    return fail("launch or copy failed");
  if (err == 1) return fail("an element id lies outside 0 .. " + std::to_string(nElts - 1));
  if (err) return fail("the element table names a node id outside 1 .. " + std::to_string(s->nNodes));
  if (tot[1] > 0x7fffffffLL) return fail("the kept boxes list " + std::to_string(tot[1]) + " lines: the new node numbers do not fit int32");
  if (tot[3] > 0x7fffffffLL) return fail("too many copy chunks");
  p->nBoxes = tot[0];
  p->nNodesNew = tot[1];
  p->nPts = tot[2];
  p->nChunks = tot[3];
  if (hipMalloc(&p->d_chunk, sizeof(int2) * (size_t)std::max<long long>(p->nChunks, 1)) != hipSuccess) return fail("device allocation failed");
  if (s->nNodes > 0) hipLaunchKernelGGL(k_ssub_newnum, sb_grid(s->nNodes), dim3(SB_BLOCK), 0, ctx->stream, sb_tab(s), p->d_flag, p->d_scan, p->d_newnum);
  hipLaunchKernelGGL(k_ssub_remap, sb_grid(nf), dim3(SB_BLOCK), 0, ctx->stream, p->d_face, nf, p->d_newnum);
  hipLaunchKernelGGL(k_ssub_chunks, sb_grid(p->nChunks), dim3(SB_BLOCK), 0, ctx->stream, p->d_scan, (int)nbt, p->nChunks, p->d_chunk);
  if (hipGetLastError() != hipSuccess || pa_sync(ctx) != 0) return fail("launch failed");
  const long long rec[8] = {nElts, nSel, nbt, p->nBoxes, p->nChunks, path, nblk, 0};
  std::copy(rec, rec + 8, p->rec);
  return p.release();
}

extern "C" int pa_ssub_counts(const pa_ssub* p, int64_t counts[3]) {
  if (!p || !counts) return 1;
  counts[0] = p->nBoxes;
  counts[1] = p->nNodesNew;
  counts[2] = p->nPts;
  return 0;
}

extern "C" int pa_ssub_last_launch(const pa_ssub* p, int64_t rec[8]) {
  if (!p || !rec) return 1;
  for (int i = 0; i < 8; ++i) rec[i] = p->rec[i];
  return 0;
}

extern "C" int pa_ssub_gather(pa_ctx* ctx, pa_ssub* p, const double* data, int32_t ncomp, int32_t ncompSel, const int32_t* comps, double* out, int32_t ncompOut, int32_t c0) {
  PaBind bind_(ctx);
  if (!ctx || !p || p->ctx != ctx || ncompSel < 1 || !comps || c0 < 0 || ncompOut < c0 + ncompSel) return pa_fail(ctx, "pa_ssub_gather: bad argument (components outside the output buffer)");
  if (ncompSel > PA_SSUB_MAXCOMPS) return pa_fail(ctx, "pa_ssub_gather: more than 64 components in one call");
  SbComps S{};
  S.n = ncompSel;
  for (int c = 0; c < ncompSel; ++c) {
    if (ncomp < 1 || comps[c] < 0 || comps[c] >= ncomp) return pa_fail(ctx, "pa_ssub_gather: component " + std::to_string(comps[c]) + " out of range (the buffer holds " + std::to_string(ncomp) + ")");
    S.comp[c] = comps[c];
  }
  if (!data || !out) return pa_fail(ctx, "pa_ssub_gather: null device array");
  dim3 grid((unsigned)p->nChunks, (unsigned)ncompSel);
  hipLaunchKernelGGL(k_ssub_gather, grid, dim3(SB_BLOCK), 0, ctx->stream, p->sel->d_box, p->d_scan, p->d_chunk, (const unsigned long long*)data, (int)ncomp, S, (unsigned long long*)out,
                     (int)ncompOut, (int)c0);
  if (hipGetLastError() != hipSuccess) return pa_fail(ctx, "pa_ssub_gather: launch failed");
  p->rec[7] = (long long)p->nChunks * ncompSel;
  return pa_sync(ctx);
}

extern "C" int pa_ssub_read(pa_ctx* ctx, pa_ssub* p, int32_t* kept, int64_t* box_desc, int32_t* newNum, int32_t* faceSel) {
  PaBind bind_(ctx);
  if (!ctx || !p || p->ctx != ctx) return pa_fail(ctx, "pa_ssub_read: bad argument");
  const pa_ssel* s = p->sel;
  if (kept || box_desc) {
    std::vector<int> flag((size_t)s->nbt);
    std::vector<long long> scan(4 * (size_t)s->nbt);
    PA_HIP(hipMemcpy(flag.data(), p->d_flag, sizeof(int) * flag.size(), hipMemcpyDeviceToHost));
    PA_HIP(hipMemcpy(scan.data(), p->d_scan, sizeof(long long) * scan.size(), hipMemcpyDeviceToHost));
    for (int g = 0; g < s->nbt; ++g) {
      if (!flag[(size_t)g]) continue;
      const long long b = scan[4 * (size_t)g];
      if (b < 0 || b >= p->nBoxes) return pa_fail(ctx, "pa_ssub_read: the plan's box scan is inconsistent");
      if (kept) kept[b] = g;
      if (box_desc) {
        box_desc[4 * b] = s->box[4 * (size_t)g];
        box_desc[4 * b + 1] = s->box[4 * (size_t)g + 1];
        box_desc[4 * b + 2] = s->box[4 * (size_t)g + 2];
        box_desc[4 * b + 3] = scan[4 * (size_t)g + 2];
      }
    }
  }
  if (newNum && s->nNodes > 0) PA_HIP(hipMemcpy(newNum, p->d_newnum, sizeof(int) * (size_t)s->nNodes, hipMemcpyDeviceToHost));
  if (faceSel) PA_HIP(hipMemcpy(faceSel, p->d_face, sizeof(int) * (size_t)(p->nSel * p->npe), hipMemcpyDeviceToHost));
  return 0;
}
