// pa_amrtofe.hip -- the hex-element mesh of an AMR hierarchy (amrToFE.cpp:296-897) on the device: the centres of all uncovered
// cells become nodes, every 2 x 2 x 2 block of them a brick; at a coarse-fine interface the ghost corners of the fine bricks
// collapse onto coarse cell centres.  The reference fills one BaseFab<Node> per grid on the box grown by one (:467-540), numbers
// the VALID cells of the valid boxes into a std::map<Node,int> (:543-556), inserts every cube whose eight corners are VALID
// into a std::set<Element> (:563-601) and reads the connectivity off the set (:608-625).  Restated as data-parallel passes:
//   1. number   one thread per cell of (grid & subbox), in the reference's order level -> grid -> cell (x fastest): a cell is a
//               node unless the next finer level covers it (:523-540).  Ids = order-preserving compaction: wave ballot +
//               popcount, the four wave counts of a block, a scan over the block sums.  Writes the node table (level, i, j, k,
//               file box) and, per cell, its id or -1.
//   2. tag      one thread per cell of every grown FAB: the node the cell stands for, as its id -- the cell itself (:469-475),
//               the coarse cell under it where no grid of the level holds it (:477-520, grid -1), or none (outside the subbox,
//               or covered).  What the three writes of the reference leave in a cell depends on the cell alone, not on the FAB.
//   3. cubes    one thread per cube base of every grown FAB (:568-597): kept when all eight tags are ids; compacted the same way
//               into a list of 8 ids per cube, in the corner order of :585-592.
//   4. order    Node::operator< (:25-30) is (level, k, j, i): a radix sort of the packed keys of the nodes gives every node its
//               RANK in that order, and Element::operator< (:68-74) is the lexicographic order of the eight ranks.  Four stable
//               LSD radix-sort passes of a permutation over (rank, rank) pairs of corners (6,7), (4,5), (2,3), (0,1), each over
//               the bits in use only; first occurrences are flagged (two boxes generate the cubes across their shared face,
//               whatever else coincides falls to the same comparison) and compacted: connectivity = id + 1 in set order.
//   5. gather   pa_fe_gather: block-ordered coordinates and components of the nodes (:738-814), one thread per output slot.
// No atomics anywhere.  Host read-backs: the node count, the cube count, the element count and an error flag.
// The reference prints "Node not found in node map" (:615-619) and goes on with misnumbered connectivity when a corner names a
// cell that no grid holds (level 0 does not cover the subbox; a fine level that is not properly nested): here the build fails.
#include <algorithm>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "pa_internal.h"

namespace {
constexpr int FE_MAXLEV = 8;

struct FeGrid {  // one box of gridArray[lev] (:421): V = file box & subbox; its NodeFab lives on V grown by one
  DBox V;
  int lev, fb;           // fb: index of the box in the file's BoxArray
  long long voff, goff;  // cells of V / of the grown box before this grid, over all levels
};
struct FeLev {
  DLevelView view;     // the file's BoxArray of the level
  DBox sub;            // subboxArray[lev] (:401-403)
  int rdn, rup;        // ratio to the coarser level / to the finer one (0: none)
  const int* fb2grid;  // file box -> grid, or -1 (the box does not touch the subbox)
};
struct FeTab {
  const FeGrid* grids;
  const FeLev* levs;
  int ngrids, nlev;
  const int* idmap;  // [cells of all V]: node id or -1
};

template <long long FeGrid::*OFF>
__device__ __forceinline__ int grid_of(const FeTab& T, long long x) {  // last g with grids[g].*OFF <= x
  int lo = 0, hi = T.ngrids - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (T.grids[mid].*OFF <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ bool in_box(const DBox& B, int i, int j, int k) {
  return i >= B.lo[0] && i <= B.hi[0] && j >= B.lo[1] && j <= B.hi[1] && k >= B.lo[2] && k <= B.hi[2];
}
// :523-540: covered by the coarsened grids of the next finer level (fine boxes are aligned to the ratio, checked by the caller)
__device__ __forceinline__ bool fe_covered(const FeTab& T, int lev, int i, int j, int k) {
  const int r = T.levs[lev].rup;
  if (!r) return false;
  const int p[3] = {i * r, j * r, k * r};
  const FeLev& F = T.levs[lev + 1];
  if (!in_box(F.sub, p[0], p[1], p[2])) return false;
  const int fb = owner_of(F.view, p);
  return fb >= 0 && F.fb2grid[fb] >= 0;
}
// id of the node of cell (lev, i, j, k), a cell of the level's subbox; -2: no grid of the level holds it, -1: covered
__device__ __forceinline__ int fe_id_at(const FeTab& T, int lev, int i, int j, int k) {
  const FeLev& L = T.levs[lev];
  const int p[3] = {i, j, k};
  const int fb = owner_of(L.view, p);
  if (fb < 0) return -2;
  const int g = L.fb2grid[fb];
  if (g < 0) return -2;
  const DBox V = T.grids[g].V;
  if (!in_box(V, i, j, k)) return -2;
  const long long nx = V.hi[0] - V.lo[0] + 1, ny = V.hi[1] - V.lo[1] + 1;
  return T.idmap[T.grids[g].voff + ((long long)(k - V.lo[2]) * ny + (j - V.lo[1])) * nx + (i - V.lo[0])];
}

// rank of this thread among the flagged threads of its block, in thread order (256 threads = 4 wavefronts of 64); every thread
// of the block calls it.  total: flagged threads of the block.
__device__ __forceinline__ int block_rank(bool f, int& total) {
  __shared__ int ws[4];
  const unsigned long long m = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) ws[w] = __popcll(m);
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < w) off += ws[q];
    total += ws[q];
  }
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

// ---- 1. nodes.  EMIT = false: block sums; true: ids, node table
template <bool EMIT>
__global__ __launch_bounds__(256) void k_fe_nodes(FeTab T, long long NV, int* bsum, const int* boff, int* idmap, int4* nodes, int* nbox) {
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  bool f = false;
  int lev = 0, fb = 0, i = 0, j = 0, k = 0;
  if (t < NV) {
    const FeGrid& G = T.grids[grid_of<&FeGrid::voff>(T, t)];
    const unsigned nx = G.V.hi[0] - G.V.lo[0] + 1, ny = G.V.hi[1] - G.V.lo[1] + 1;
    const unsigned q = (unsigned)(t - G.voff), r = q / nx, kk = r / ny;
    i = G.V.lo[0] + (int)(q - r * nx);
    j = G.V.lo[1] + (int)(r - kk * ny);
    k = G.V.lo[2] + (int)kk;
    lev = G.lev;
    fb = G.fb;
    f = !fe_covered(T, lev, i, j, k);
  }
  int total;
  const int rk = block_rank(f, total);
  if (!EMIT) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    return;
  }
  if (t >= NV) return;
  const int id = boff[blockIdx.x] + rk;
  idmap[t] = f ? id : -1;
  if (f) {
    nodes[id] = make_int4(lev, i, j, k);
    nbox[id] = fb;
  }
}

// ---- 2. tags of the grown FABs
// tag: the node's id; -1: INIT or COVERED; -2: VALID, but no grid holds the node (an error only as a corner of a kept cube)
__global__ __launch_bounds__(256) void k_fe_tag(FeTab T, long long NG, int* tag) {
  const long long u = blockIdx.x * 256LL + threadIdx.x;
  if (u >= NG) return;
  const FeGrid& G = T.grids[grid_of<&FeGrid::goff>(T, u)];
  const unsigned nx = G.V.hi[0] - G.V.lo[0] + 3, ny = G.V.hi[1] - G.V.lo[1] + 3;
  const unsigned q = (unsigned)(u - G.goff), r = q / nx, kk = r / ny;
  const int i = G.V.lo[0] - 1 + (int)(q - r * nx), j = G.V.lo[1] - 1 + (int)(r - kk * ny), k = G.V.lo[2] - 1 + (int)kk;
  const int lev = G.lev;
  const FeLev& L = T.levs[lev];
  int id = -1;
  if (in_box(L.sub, i, j, k) && !fe_covered(T, lev, i, j, k)) {  // INIT outside the subbox (:472), COVERED (:537)
    id = fe_id_at(T, lev, i, j, k);                              // VALID at (lev, iv) (:474)
    if (id == -2 && L.rdn) {                                     // no grid of the level: the coarse alias (:506)
      const int r0 = L.rdn;
      id = fe_id_at(T, lev - 1, coarsen_idx(i, r0), coarsen_idx(j, r0), coarsen_idx(k, r0));
    }
    if (id < 0) id = -2;
  }
  tag[u] = id;
}

// ---- 3. cubes.  EMIT = false: block sums; true: the eight ids of every kept cube
template <bool EMIT>
__global__ __launch_bounds__(256) void k_fe_cubes(FeTab T, long long NG, const int* tag, int* bsum, const int* boff, int* raw, int* err) {
  const long long u = blockIdx.x * 256LL + threadIdx.x;
  bool f = false;
  int c[8];
  if (u < NG) {
    const FeGrid& G = T.grids[grid_of<&FeGrid::goff>(T, u)];
    const unsigned nx = G.V.hi[0] - G.V.lo[0] + 3, ny = G.V.hi[1] - G.V.lo[1] + 3, nz = G.V.hi[2] - G.V.lo[2] + 3;
    const unsigned q = (unsigned)(u - G.goff), r = q / nx, kk = r / ny;
    const unsigned ii = q - r * nx, jj = r - kk * ny;
    if (ii + 1 < nx && jj + 1 < ny && kk + 1 < nz) {  // the base and its seven neighbours lie in the FAB; outside the subbox a tag is -1
      const int* p = tag + u;
      const long long sy = nx, sz = (long long)nx * ny;
      c[0] = p[0]; c[1] = p[1]; c[2] = p[1 + sy]; c[3] = p[sy];  // :585-592
      c[4] = p[sz]; c[5] = p[sz + 1]; c[6] = p[sz + 1 + sy]; c[7] = p[sz + sy];
      f = true;
#pragma unroll
      for (int q = 0; q < 8; ++q) f = f && c[q] != -1;  // all eight VALID (:593-596)
      if (f && (c[0] | c[1] | c[2] | c[3] | c[4] | c[5] | c[6] | c[7]) < 0) *err = 1;  // "Node not found in node map" (:615-619); every writer stores 1
    }
  }
  int total;
  const int rk = block_rank(f, total);
  if (!EMIT) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    return;
  }
  if (!f) return;
  int4* o = (int4*)(raw + 8LL * (boff[blockIdx.x] + rk));
  o[0] = make_int4(c[0], c[1], c[2], c[3]);
  o[1] = make_int4(c[4], c[5], c[6], c[7]);
}

// ---- 4. order
struct FeKeyPack { int nb, dlo[FE_MAXLEV][3]; };
__global__ __launch_bounds__(256) void k_fe_nodekeys(long long N, const int4* nodes, FeKeyPack P, unsigned long long* key, int* idx) {
  const long long n = blockIdx.x * 256LL + threadIdx.x;
  if (n >= N) return;
  const int4 v = nodes[n];  // (level, i, j, k)
  const unsigned long long i = (unsigned)(v.y - P.dlo[v.x][0]), j = (unsigned)(v.z - P.dlo[v.x][1]), k = (unsigned)(v.w - P.dlo[v.x][2]);
  key[n] = ((((unsigned long long)v.x << P.nb | k) << P.nb | j) << P.nb) | i;
  idx[n] = (int)n;
}
__global__ __launch_bounds__(256) void k_fe_rank(long long N, const int* sorted, int* rank) {
  const long long r = blockIdx.x * 256LL + threadIdx.x;
  if (r < N) rank[sorted[r]] = (int)r;
}
// perm == nullptr: the identity (first pass), written to pout
__global__ __launch_bounds__(256) void k_fe_cubekeys(long long M, const int* perm, int* pout, const int* raw, const int* rank, int c0, int nb, unsigned long long* key) {
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t >= M) return;
  const long long e = perm ? perm[t] : t;
  if (!perm) pout[t] = (int)t;
  const int2 ab = *(const int2*)(raw + 8 * e + c0);
  key[t] = ((unsigned long long)(unsigned)rank[ab.x] << nb) | (unsigned)rank[ab.y];
}
template <bool EMIT>
__global__ __launch_bounds__(256) void k_fe_unique(long long M, const int* perm, const int* raw, int* bsum, const int* boff, int32_t* conn) {
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  bool f = false;
  int4 a0 = make_int4(0, 0, 0, 0), a1 = a0;
  if (t < M) {
    const int4* a = (const int4*)(raw + 8LL * perm[t]);
    a0 = a[0]; a1 = a[1];
    f = true;
    if (t > 0) {
      const int4* b = (const int4*)(raw + 8LL * perm[t - 1]);
      const int4 b0 = b[0], b1 = b[1];
      f = a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y || a1.z != b1.z || a1.w != b1.w;
    }
  }
  int total;
  const int rk = block_rank(f, total);
  if (!EMIT) {
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
    return;
  }
  if (!f) return;
  int4* o = (int4*)(conn + 8LL * (boff[blockIdx.x] + rk));
  o[0] = make_int4(a0.x + 1, a0.y + 1, a0.z + 1, a0.w + 1);  // :622
  o[1] = make_int4(a1.x + 1, a1.y + 1, a1.z + 1, a1.w + 1);
}
__global__ __launch_bounds__(256) void k_fe_iota(long long n, int32_t* conn) {  // :626-633
  const long long t = blockIdx.x * 256LL + threadIdx.x;
  if (t < n) conn[t] = (int32_t)(t + 1);
}

// ---- 5. node data (:738-814)
constexpr int FE_GCOMPS = 16;
struct FeGather {
  DMFView mf[FE_MAXLEV];
  const DBox* boxes[FE_MAXLEV];
  double dx[FE_MAXLEV][3], plo[3];
  int comps[FE_GCOMPS], ncomp, coords, connect_cc;
};
__global__ __launch_bounds__(256) void k_fe_gather(FeGather A, long long NF, const int4* nodes, const int* nbox, double* out /* row 0 of this launch */, double* xyz) {
  const long long m = blockIdx.x * 256LL + threadIdx.x;
  if (m >= NF) return;
  const long long n = A.connect_cc ? m : (m >> 3);
  const int4 v = nodes[n];
  const int lev = v.x;
  if (A.coords) {
    int iv[3] = {v.y, v.z, v.w};
    double offset = 0.5;
    if (!A.connect_cc) {  // :779-787, the block under "#if BLSPACEDIM==3" is never compiled: corners 4..7 stay at iv
      const int c = (int)(m & 7);
      offset = 0.0;
      if (c == 1 || c == 2) iv[0] += 1;
      if (c == 2 || c == 3) iv[1] += 1;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) xyz[d * NF + m] = A.plo[d] + ((double)iv[d] + offset) * A.dx[lev][d];  // :799
  }
  const DMFView& M = A.mf[lev];
  const int b = nbox[n];
  const DBox B = A.boxes[lev][b];
  const double* base = M.data + M.off[b];
  for (int c = 0; c < A.ncomp; ++c) out[c * NF + m] = base[fab_index(B, M.ng, M.ncomp, A.comps[c], v.y, v.z, v.w)];  // :809
}

struct Arena {
  unsigned char* p;
  size_t used = 0;
  template <class T> T* take(size_t n) { T* r = (T*)(p + used); used += (n * sizeof(T) + 255) / 256 * 256; return r; }
};
inline size_t al(size_t n, size_t sz) { return (n * sz + 255) / 256 * 256; }
inline int bits_for(long long n) {  // bits that hold 0 .. n - 1
  int b = 1;
  while ((1LL << b) < n) ++b;
  return b;
}
DBox isect(const DBox& a, const DBox& b) {
  DBox r;
  for (int d = 0; d < 3; ++d) { r.lo[d] = std::max(a.lo[d], b.lo[d]); r.hi[d] = std::min(a.hi[d], b.hi[d]); }
  return r;
}
bool ok_box(const DBox& b) { return b.lo[0] <= b.hi[0] && b.lo[1] <= b.hi[1] && b.lo[2] <= b.hi[2]; }
}  // namespace

struct pa_fe {
  pa_ctx* ctx = nullptr;
  int nlev = 0, connect_cc = 1;
  long long nnodes = 0, nelts = 0, nfinal = 0, ncubes = 0;
  std::vector<const pa_level*> levels;
  double dx[FE_MAXLEV][3], plo[3];
  int4* d_nodes = nullptr;   // (level, i, j, k) of every node id
  int* d_nbox = nullptr;     // its box in the file's BoxArray
  int32_t* d_conn = nullptr;
  hipEvent_t ev[7] = {};     // 0-4: the boundaries of number, tag, cubes, order in the build; 5, 6: around the last gather
  bool gathered = false;
};

extern "C" void pa_fe_destroy(pa_fe* F) {
  if (!F) return;
  PaBind bind_(F->ctx);
  if (F->ctx && F->ctx->stream) (void)hipStreamSynchronize(F->ctx->stream);
  if (F->d_nodes) (void)hipFree(F->d_nodes);
  if (F->d_nbox) (void)hipFree(F->d_nbox);
  if (F->d_conn) (void)hipFree(F->d_conn);
  for (hipEvent_t e : F->ev)
    if (e) (void)hipEventDestroy(e);
  delete F;
}

static int fe_build(pa_ctx* ctx, pa_fe* F, int nlev_in, const pa_level* const* levels, const int32_t* ratios, const pa_box* subbox) {
  hipStream_t st = ctx->stream;
  // ---- the grids of every level (:374-452)
  DBox sub[FE_MAXLEV];
  std::vector<FeGrid> grids;
  std::vector<std::vector<int>> fb2grid;
  long long NV = 0, NG = 0;
  int nlev = 0;
  for (int lev = 0; lev < nlev_in; ++lev) {
    const pa_level* L = levels[lev];
    DBox dom;
    for (int d = 0; d < 3; ++d) { dom.lo[d] = L->domlo[d]; dom.hi[d] = L->domhi[d]; }
    if (lev == 0) {
      sub[0] = dom;
      if (subbox) {
        DBox b;
        for (int d = 0; d < 3; ++d) { b.lo[d] = subbox->lo[d]; b.hi[d] = subbox->hi[d]; }
        sub[0] = isect(b, dom);
        if (!ok_box(sub[0])) return pa_fail(ctx, "pa_fe_build: the box does not intersect the domain");
      }
    } else {
      const int r = ratios[lev - 1];
      for (int d = 0; d < 3; ++d) {
        if ((long long)(levels[lev - 1]->domhi[d] + 1) * r - 1 != L->domhi[d] || (long long)levels[lev - 1]->domlo[d] * r != L->domlo[d])
          return pa_fail(ctx, "pa_fe_build: the domain of level " + std::to_string(lev) + " is not the refined domain of the level below");
        sub[lev].lo[d] = sub[lev - 1].lo[d] * r;
        sub[lev].hi[d] = (sub[lev - 1].hi[d] + 1) * r - 1;
      }
    }
    std::vector<int> map(L->boxes.size(), -1);
    const size_t before = grids.size();
    for (size_t b = 0; b < L->boxes.size(); ++b) {
      const DBox V = isect(L->boxes[b], sub[lev]);
      if (!ok_box(V)) continue;
      map[b] = (int)grids.size();
      FeGrid G;
      G.V = V; G.lev = lev; G.fb = (int)b; G.voff = NV; G.goff = NG;
      long long nv = 1, ng = 1;
      for (int d = 0; d < 3; ++d) { nv *= V.hi[d] - V.lo[d] + 1; ng *= V.hi[d] - V.lo[d] + 3; }
      if (ng >= 0x7fffffffLL) return pa_fail(ctx, "pa_fe_build: a grid of more than 2^31 cells: node and connectivity counts beyond int");
      NV += nv; NG += ng;
      grids.push_back(G);
    }
    if (grids.size() == before) break;  // :445-451: the first level without a grid ends the hierarchy
    fb2grid.push_back(std::move(map));
    nlev = lev + 1;
  }
  if (nlev == 0) return pa_fail(ctx, "pa_fe_build: no grid of level 0 touches the box");
  for (int lev = 1; lev < nlev; ++lev) {  // :499-507 writes outside dst for a box that is not aligned
    const int r = ratios[lev - 1];
    for (const DBox& B : levels[lev]->boxes)
      for (int d = 0; d < 3; ++d)
        if (B.lo[d] % r != 0 || (B.hi[d] + 1) % r != 0) return pa_fail(ctx, "pa_fe_build: a box of level " + std::to_string(lev) + " is not aligned to the refinement ratio " + std::to_string(r));
  }
  if (NG >= 0x7fffffffLL) return pa_fail(ctx, "pa_fe_build: more than 2^31 cells in the grown grids: node and connectivity counts beyond int");
  F->nlev = nlev;
  F->levels.assign(levels, levels + nlev);
  int maxlen = 1;
  for (int lev = 0; lev < nlev; ++lev)
    for (int d = 0; d < 3; ++d) {
      F->dx[lev][d] = (levels[0]->prob_hi[d] - levels[0]->prob_lo[d]) / (double)(levels[lev]->domhi[d] - levels[lev]->domlo[d] + 1);  // :718-724
      maxlen = std::max(maxlen, levels[lev]->domhi[d] - levels[lev]->domlo[d] + 1);
    }
  for (int d = 0; d < 3; ++d) F->plo[d] = levels[0]->prob_lo[d];
  FeKeyPack KP;
  KP.nb = bits_for(maxlen);
  const int keybits = 3 * KP.nb + bits_for(nlev);
  if (keybits > 64) return pa_fail(ctx, "pa_fe_build: the domain is too large for a 64-bit node key");
  for (int lev = 0; lev < FE_MAXLEV; ++lev)
    for (int d = 0; d < 3; ++d) KP.dlo[lev][d] = lev < nlev ? levels[lev]->domlo[d] : 0;

  // ---- stage memory (the context's grow-only scratch): tables, id map, tags, block sums
  const size_t nblk = (size_t)((NG + 255) / 256);
  size_t tscan = 0;
  (void)rocprim::exclusive_scan(nullptr, tscan, (int*)nullptr, (int*)nullptr, 0, nblk, rocprim::plus<int>(), st);
  size_t nfb = 0;
  for (auto& m : fb2grid) nfb += al(m.size(), 4);
  const size_t bytes = al(grids.size(), sizeof(FeGrid)) + al(nlev, sizeof(FeLev)) + nfb + al((size_t)NV, 4) + al((size_t)NG, 4) + 2 * al(nblk, 4) + al(tscan, 1) + 512;
  if (pa_ensure_scr(ctx, bytes)) return 1;
  Arena A{(unsigned char*)ctx->d_scr};
  FeGrid* d_grids = A.take<FeGrid>(grids.size());
  FeLev* d_levs = A.take<FeLev>(nlev);
  std::vector<FeLev> hl(nlev);
  for (int lev = 0; lev < nlev; ++lev) {
    int* d_map = A.take<int>(fb2grid[lev].size());
    PA_HIP(hipMemcpyAsync(d_map, fb2grid[lev].data(), 4 * fb2grid[lev].size(), hipMemcpyHostToDevice, st));
    hl[lev].view = levels[lev]->view;
    hl[lev].sub = sub[lev];
    hl[lev].rdn = lev > 0 ? ratios[lev - 1] : 0;
    hl[lev].rup = lev + 1 < nlev ? ratios[lev] : 0;
    hl[lev].fb2grid = d_map;
  }
  int* idmap = A.take<int>((size_t)NV);
  int* tag = A.take<int>((size_t)NG);
  int* bsum = A.take<int>(nblk);
  int* boff = A.take<int>(nblk);
  void* tmp = A.take<unsigned char>(tscan);
  int* d_err = A.take<int>(64);
  PA_HIP(hipMemcpyAsync(d_grids, grids.data(), grids.size() * sizeof(FeGrid), hipMemcpyHostToDevice, st));
  PA_HIP(hipMemcpyAsync(d_levs, hl.data(), nlev * sizeof(FeLev), hipMemcpyHostToDevice, st));
  PA_HIP(hipMemsetAsync(d_err, 0, 256, st));
  const FeTab T{d_grids, d_levs, (int)grids.size(), nlev, idmap};
  const dim3 blk(256);
  auto nb_of = [](long long n) { return dim3((unsigned)((std::max<long long>(n, 1) + 255) / 256)); };
  auto scan = [&](size_t n) -> int {
    size_t tb = tscan;
    PA_HIP(rocprim::exclusive_scan(tmp, tb, bsum, boff, 0, n, rocprim::plus<int>(), st));
    return 0;
  };
  auto total = [&](size_t n, long long& out) -> int {  // blocks 0 .. n - 1: offset + sum of the last one
    int a = 0, b = 0;
    PA_HIP(hipMemcpyAsync(&a, boff + (n - 1), 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipMemcpyAsync(&b, bsum + (n - 1), 4, hipMemcpyDeviceToHost, st));
    PA_HIP(hipStreamSynchronize(st));
    out = (long long)a + b;
    return 0;
  };
  for (hipEvent_t& e : F->ev) PA_HIP(hipEventCreate(&e));

  // ---- 1. nodes
  PA_HIP(hipEventRecord(F->ev[0], st));
  const dim3 gv = nb_of(NV), gg = nb_of(NG);
  hipLaunchKernelGGL(k_fe_nodes<false>, gv, blk, 0, st, T, NV, bsum, (const int*)nullptr, (int*)nullptr, (int4*)nullptr, (int*)nullptr);
  if (scan(gv.x)) return 1;
  long long N = 0;
  if (total(gv.x, N)) return 1;
  if (N == 0) return pa_fail(ctx, "pa_fe_build: no node");
  F->nnodes = N;
  PA_HIP(hipMalloc(&F->d_nodes, (size_t)N * sizeof(int4)));
  PA_HIP(hipMalloc(&F->d_nbox, (size_t)N * 4));
  hipLaunchKernelGGL(k_fe_nodes<true>, gv, blk, 0, st, T, NV, bsum, (const int*)boff, idmap, F->d_nodes, F->d_nbox);
  PA_HIP(hipEventRecord(F->ev[1], st));
  // ---- 2. tags
  hipLaunchKernelGGL(k_fe_tag, gg, blk, 0, st, T, NG, tag);
  PA_HIP(hipEventRecord(F->ev[2], st));
  // ---- 3. cubes
  hipLaunchKernelGGL(k_fe_cubes<false>, gg, blk, 0, st, T, NG, (const int*)tag, bsum, (const int*)nullptr, (int*)nullptr, d_err);
  if (scan(gg.x)) return 1;
  long long M = 0;
  if (total(gg.x, M)) return 1;
  int h_err = 0;
  PA_HIP(hipMemcpy(&h_err, d_err, 4, hipMemcpyDeviceToHost));
  if (h_err) return pa_fail(ctx, "pa_fe_build: Node not found in node map: a corner of an element lies in no grid (level 0 does not cover the box, or a fine level is not properly nested)");
  F->ncubes = M;
  if (!F->connect_cc) {  // :603, :626-633: one element per node
    if (8 * N >= 0x7fffffffLL) return pa_fail(ctx, "pa_fe_build: node and connectivity counts beyond int");
    F->nelts = N;
    F->nfinal = 8 * N;
    PA_HIP(hipMalloc(&F->d_conn, (size_t)N * 32));
    PA_HIP(hipEventRecord(F->ev[3], st));
    hipLaunchKernelGGL(k_fe_iota, nb_of(8 * N), blk, 0, st, 8 * N, F->d_conn);
    PA_HIP(hipEventRecord(F->ev[4], st));
    PA_HIP(hipGetLastError());
    PA_HIP(hipStreamSynchronize(st));
    return 0;
  }
  F->nfinal = N;
  if (M == 0) {
    PA_HIP(hipEventRecord(F->ev[3], st));
    PA_HIP(hipEventRecord(F->ev[4], st));
    PA_HIP(hipStreamSynchronize(st));
    return 0;
  }
  // ---- 4. order: its arrays are sized from the cube count while the stage memory is in use: the context's second scratch
  const int rb = bits_for(N);
  size_t t1 = 0, t2 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t1, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)N, 0, keybits, st);
  (void)rocprim::radix_sort_pairs(nullptr, t2, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr, (int*)nullptr, (size_t)M, 0, 2 * rb, st);
  const size_t tsort = std::max(t1, t2);
  const size_t K = (size_t)std::max(N, M);
  const size_t wbytes = al((size_t)M * 8, 4) + 2 * al(K, 8) + 2 * al(K, 4) + al((size_t)N, 4) + al(tsort, 1) + 256;
  if (pa_ensure_scr(ctx, wbytes, 1)) return 1;
  Arena W{(unsigned char*)ctx->d_scr2};
  int* raw = W.take<int>((size_t)M * 8);
  unsigned long long* key[2] = {W.take<unsigned long long>(K), W.take<unsigned long long>(K)};
  int* perm[2] = {W.take<int>(K), W.take<int>(K)};
  int* rank = W.take<int>((size_t)N);
  void* stmp = W.take<unsigned char>(tsort);
  hipLaunchKernelGGL(k_fe_cubes<true>, gg, blk, 0, st, T, NG, (const int*)tag, bsum, (const int*)boff, raw, d_err);
  PA_HIP(hipEventRecord(F->ev[3], st));
  const dim3 gn = nb_of(N), gm = nb_of(M);
  hipLaunchKernelGGL(k_fe_nodekeys, gn, blk, 0, st, N, (const int4*)F->d_nodes, KP, key[0], perm[0]);
  size_t tb = tsort;
  PA_HIP(rocprim::radix_sort_pairs(stmp, tb, key[0], key[1], perm[0], perm[1], (size_t)N, 0, keybits, st));
  hipLaunchKernelGGL(k_fe_rank, gn, blk, 0, st, N, (const int*)perm[1], rank);
  int cur = 0;  // perm[cur]: the order so far
  for (int pass = 0; pass < 4; ++pass) {
    const int c0 = 6 - 2 * pass;
    hipLaunchKernelGGL(k_fe_cubekeys, gm, blk, 0, st, M, pass ? (const int*)perm[cur] : (const int*)nullptr, perm[cur], (const int*)raw, (const int*)rank, c0, rb, key[0]);
    tb = tsort;
    PA_HIP(rocprim::radix_sort_pairs(stmp, tb, key[0], key[1], perm[cur], perm[cur ^ 1], (size_t)M, 0, 2 * rb, st));
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_fe_unique<false>, gm, blk, 0, st, M, (const int*)perm[cur], (const int*)raw, bsum, (const int*)nullptr, (int32_t*)nullptr);
  if (scan(gm.x)) return 1;
  long long E = 0;
  if (total(gm.x, E)) return 1;
  if (8 * E >= 0x7fffffffLL) return pa_fail(ctx, "pa_fe_build: node and connectivity counts beyond int");
  F->nelts = E;
  PA_HIP(hipMalloc(&F->d_conn, (size_t)E * 32));
  hipLaunchKernelGGL(k_fe_unique<true>, gm, blk, 0, st, M, (const int*)perm[cur], (const int*)raw, bsum, (const int*)boff, F->d_conn);
  PA_HIP(hipEventRecord(F->ev[4], st));
  PA_HIP(hipGetLastError());
  PA_HIP(hipStreamSynchronize(st));
  return 0;
}

// amrToFE.cpp:374-452 (subbox, gridArray, the level that ends the hierarchy) and :465-633 (nodeMap, elements, connData)
extern "C" pa_fe* pa_fe_build(pa_ctx* ctx, int nlev, const pa_level* const* levels, const int32_t* ratios, const pa_box* subbox, int connect_cc,
                              int32_t* nlev_used, int64_t* nnodes, int64_t* nelts) {
  PaBind bind_(ctx);
  if (!ctx) return nullptr;
  if (!levels || nlev < 1 || nlev > FE_MAXLEV || (nlev > 1 && !ratios)) { pa_fail(ctx, "pa_fe_build: 1 to " + std::to_string(FE_MAXLEV) + " levels and their ratios"); return nullptr; }
  for (int l = 0; l < nlev; ++l) {
    if (!levels[l] || levels[l]->ctx != ctx) { pa_fail(ctx, "pa_fe_build: a level of another context"); return nullptr; }
    if (levels[l]->nranks != 1) { pa_fail(ctx, "pa_fe_build: sharded levels are not supported (one GPU)"); return nullptr; }
    if (l + 1 < nlev && (ratios[l] < 2 || ratios[l] > 64)) { pa_fail(ctx, "pa_fe_build: refinement ratio out of range"); return nullptr; }
  }
  pa_fe* F = new pa_fe;
  F->ctx = ctx;
  F->connect_cc = connect_cc ? 1 : 0;
  if (fe_build(ctx, F, nlev, levels, ratios, subbox)) {
    pa_fe_destroy(F);
    return nullptr;
  }
  if (nlev_used) *nlev_used = F->nlev;
  if (nnodes) *nnodes = F->nfinal;
  if (nelts) *nelts = F->nelts;
  return F;
}

// amrToFE.cpp:608-633: connData, [nelts][8], 1-based; the array belongs to the mesh
extern "C" int pa_fe_connectivity(pa_ctx* ctx, const pa_fe* F, const int32_t** dev_conn) {
  if (!ctx || !F || !dev_conn) return pa_fail(ctx, "pa_fe_connectivity: null argument");
  *dev_conn = F->d_conn;
  return 0;
}

// amrToFE.cpp:638-646: nodeVect, (level, i, j, k) of every node id; the array belongs to the mesh.  nids: nodeVect.size(), which is
// nelts rather than the node count of the output without connect_cc
extern "C" int pa_fe_nodes(pa_ctx* ctx, const pa_fe* F, int64_t* nids, const int32_t** dev_nodes) {
  if (!ctx || !F || !dev_nodes) return pa_fail(ctx, "pa_fe_nodes: null argument");
  if (nids) *nids = F->nnodes;
  *dev_nodes = (const int32_t*)F->d_nodes;
  return 0;
}

// amrToFE.cpp:711-814: tmpData in block ordering
extern "C" int pa_fe_gather(pa_ctx* ctx, pa_fe* F, int nlev, const pa_mf* const* mfs, int ncomp, const int32_t* comps, double* dev_out) {
  PaBind bind_(ctx);
  if (!ctx || !F || !mfs || !dev_out || (ncomp > 0 && !comps) || ncomp < 0) return pa_fail(ctx, "pa_fe_gather: null argument");
  if (nlev < F->nlev) return pa_fail(ctx, "pa_fe_gather: the mesh uses " + std::to_string(F->nlev) + " levels");
  FeGather A;
  for (int l = 0; l < F->nlev; ++l) {
    if (!mfs[l] || mfs[l]->lev != F->levels[l]) return pa_fail(ctx, "pa_fe_gather: multifab " + std::to_string(l) + " does not live on the level the mesh was built from");
    for (int c = 0; c < ncomp; ++c)
      if (comps[c] < 0 || comps[c] >= mfs[l]->ncomp) return pa_fail(ctx, "pa_fe_gather: component out of range");
    A.mf[l] = mfs[l]->view;
    A.boxes[l] = F->levels[l]->d_boxes;
    for (int d = 0; d < 3; ++d) A.dx[l][d] = F->dx[l][d];
  }
  for (int d = 0; d < 3; ++d) A.plo[d] = F->plo[d];
  A.connect_cc = F->connect_cc;
  const long long NF = F->nfinal;
  hipStream_t st = ctx->stream;
  PA_HIP(hipEventRecord(F->ev[5], st));
  const dim3 g((unsigned)((NF + 255) / 256)), blk(256);
  for (int c0 = 0; c0 == 0 || c0 < ncomp; c0 += FE_GCOMPS) {
    A.ncomp = std::min(FE_GCOMPS, ncomp - c0);
    A.coords = c0 == 0;
    for (int c = 0; c < A.ncomp; ++c) A.comps[c] = comps[c0 + c];
    hipLaunchKernelGGL(k_fe_gather, g, blk, 0, st, A, NF, (const int4*)F->d_nodes, (const int*)F->d_nbox, dev_out + (3 + c0) * NF, dev_out);
  }
  PA_HIP(hipEventRecord(F->ev[6], st));
  PA_HIP(hipGetLastError());
  F->gathered = true;
  return 0;
}

// milliseconds of the stages of the build (number, tag, cubes, order) and of the last gather (0 before the first); the raw cube count
extern "C" int pa_fe_stage_times(pa_ctx* ctx, const pa_fe* F, double ms[5], int64_t* ncubes) {
  PaBind bind_(ctx);
  if (!ctx || !F || !ms) return pa_fail(ctx, "pa_fe_stage_times: null argument");
  PA_HIP(hipStreamSynchronize(ctx->stream));
  for (int s = 0; s < 4; ++s) {
    float t = 0.f;
    PA_HIP(hipEventElapsedTime(&t, F->ev[s], F->ev[s + 1]));
    ms[s] = t;
  }
  ms[4] = 0.0;
  if (F->gathered) {
    float t = 0.f;
    PA_HIP(hipEventElapsedTime(&t, F->ev[5], F->ev[6]));
    ms[4] = t;
  }
  if (ncubes) *ncubes = F->ncubes;
  return 0;
}
