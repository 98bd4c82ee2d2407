// iso_ref_wrap.cpp -- C entry points around the REFERENCE's own isosurface arithmetic.  oracle/Makefile `ref` cuts
// Src/isosurface.cpp from `static Real isoVal_DEF` to just before `Collate` (Edge, VI_doIt, VertexInterp, Segmentise,
// Polygonise with its two tables, Node, Element) into oracle/_ref/iso_slice.inc at build time and compiles this file
// twice, -DAMREX_SPACEDIM=3 -> oracle/_ref/libiso_ref3.so and =2 -> libiso_ref2.so (the reference's types live at global
// scope, so one library cannot hold both).  The slice is never copied into this repository.
// Test infrastructure only: pins oracle/pa_oracle_mc.c, oracle.msq_fab and oracle.iso_merge (and through the recorded
// outputs, tests/golden/mc_ref.npz, the HIP kernels) to the reference's compiled code.
// What is OURS here, and restated from main(): the per-FAB loop (:1572-1592) with the vertex ids of :1601-1611, and the
// node / element sets (:1687-1726, :1751-1807).  Box::next runs x fastest: RECALLED (amrex_shim.h, fact (2)).
#include "amrex_shim.h"

#include <cstdint>

using namespace amrex;
using std::cerr;
using std::endl;
using std::list;
using std::string;
using std::vector;

#include "iso_slice.inc"  // oracle/_ref/, made by the Makefile from the reference tree

namespace {

FArrayBox view(const double* p, const int32_t* lo, const int32_t* hi, int ncomp) {
  FArrayBox f;
  f.p = p;
  f.ncomp = ncomp;
  for (int d = 0; d < AMREX_SPACEDIM; ++d) {
    f.lo[d] = lo[d];
    f.n[d] = (long)hi[d] - lo[d] + 1;
  }
  return f;
}

}  // namespace

// One FAB.  state [ncomp][nz][ny][nx] (2-D: [ncomp][ny][nx]) over slo..shi, mask over the same box, base points llo..lhi.
// Outputs (written when the buffers hold them; the counts always): verts [nv][ncomp] in vertCache order, keys
// [nv][2*DIM] = (IV_l, IV_r), elts [ne][DIM] local vertex ids in the order the elements were appended.
#if AMREX_SPACEDIM == 3
extern "C" int ref_mc_fab(
#else
extern "C" int ref_msq_fab(
#endif
    const double* state, const double* mask, const int32_t* slo, const int32_t* shi, int ncomp, int isocomp, double isoval, const int32_t* llo,
    const int32_t* lhi, double* verts, int32_t* keys, int64_t max_v, int32_t* elts, int64_t max_e, int64_t* nv_out, int64_t* ne_out) {
  const FArrayBox sfab = view(state, slo, shi, ncomp), mfab = view(mask, slo, shi, 1);
  for (int d = 0; d < AMREX_SPACEDIM; ++d)
    if (llo[d] <= lhi[d] && (llo[d] < slo[d] || lhi[d] + 1 > shi[d])) return 1;  // a cell's far corner would leave the FAB
  PMap vertCache;  // :1572
#if AMREX_SPACEDIM == 2
  SegList elements;  // :1575-1582; loopBox.next(iv): x fastest
  for (int j = llo[1]; j <= lhi[1]; ++j)
    for (int i = llo[0]; i <= lhi[0]; ++i) {
      IntVect iv;
      iv[0] = i; iv[1] = j;
      auto eltSegs = Segmentise(sfab, mfab, vertCache, iv, isoval, isocomp);
      for (size_t q = 0; q < eltSegs.size(); q++) elements.push_back(eltSegs[q]);
    }
#else
  TriList elements;  // :1584-1592 (CheckSurfaceNormal only prints)
  for (int k = llo[2]; k <= lhi[2]; ++k)
    for (int j = llo[1]; j <= lhi[1]; ++j)
      for (int i = llo[0]; i <= lhi[0]; ++i) {
        IntVect iv;
        iv[0] = i; iv[1] = j; iv[2] = k;
        auto eltTris = Polygonise(sfab, mfab, vertCache, iv, isoval, isocomp);
        for (size_t q = 0; q < eltTris.size(); q++) elements.push_back(eltTris[q]);
      }
#endif
  // :1601-1611: ids in vertCache order
  std::map<PMapIt, unsigned int, PMapItCompare> ptID;
  unsigned int id = 0;
  const int64_t nv = (int64_t)vertCache.size(), ne = (int64_t)elements.size();
  const bool wv = verts && keys && max_v >= nv, we = elts && max_e >= ne;
  for (PMapIt it = vertCache.begin(); it != vertCache.end(); ++it) {
    if (wv) {
      for (int c = 0; c < ncomp; ++c) verts[(int64_t)id * ncomp + c] = it->second[c];
      for (int d = 0; d < AMREX_SPACEDIM; ++d) {
        keys[(int64_t)id * 2 * AMREX_SPACEDIM + d] = it->first.IV_l[d];
        keys[(int64_t)id * 2 * AMREX_SPACEDIM + AMREX_SPACEDIM + d] = it->first.IV_r[d];
      }
    }
    ptID[it] = id++;
  }
  if (we) {
    int64_t e = 0;
    for (const auto& elt : elements) {
      for (int k = 0; k < AMREX_SPACEDIM; ++k) elts[e * AMREX_SPACEDIM + k] = (int32_t)ptID[elt[k]];
      ++e;
    }
  }
  *nv_out = nv;
  *ne_out = ne;
  return 0;
}

// The global node / element sets over the reference's own std::set<Node> and std::set<Element>.  Fragments in order:
// verts = all fragments' vertices [sum nv][ncomp] (each fragment in vertCache order), elts = all fragments' elements
// [sum ne][DIM] as fragment-local ids.  nodes_out [<= sum nv][ncomp] by m_idx, elts_out [<= sum ne][DIM] in
// std::set<Element> order.  Node::operator< is not a strict weak ordering (which std::set requires).  Returns
//   0  the reference's answer
//   3  nodeSet.find(n) at :1699 returned end() -- the reference dereferences that iterator (undefined behaviour); nothing
//      is dereferenced here and nothing is returned
//   4  a check of OURS: the reference ran through, and the outputs hold its answer, but the finished nodeSet holds two
//      nodes that its own ordering calls equivalent (closer than epsilon_DEF): an insert walked past the copy it should
//      have met, and which copies survive depends on the shape of the tree
extern "C" int ref_iso_merge(int64_t nfrag, const int64_t* nv, const int64_t* ne, const double* verts, const int32_t* elts, int ncomp,
                             double* nodes_out, int64_t* nn_out, int32_t* elts_out, int64_t* nelt_out) {
  std::set<Node> nodeSet;
  std::set<Element> eltSet;
  int64_t ov = 0, oe = 0;
  for (int64_t f = 0; f < nfrag; ++f) {
    // :1687-1701, the vertices of the fragment standing for vertCache.begin() .. end()
    std::vector<std::set<Node>::iterator> PMI_N_map((size_t)nv[f]);
    for (int64_t q = 0; q < nv[f]; ++q) {
      const double* p = verts + (ov + q) * ncomp;
      const std::vector<Real> pt(p, p + ncomp);
      const Node n(pt, nodeSet.size());
      std::pair<std::set<Node>::iterator, bool> nsit = nodeSet.insert(n);
      if (nsit.second) {
        PMI_N_map[(size_t)q] = nsit.first;
      } else {
        std::set<Node>::iterator found = nodeSet.find(n);
        if (found == nodeSet.end()) return 3;  // before anything is dereferenced
        PMI_N_map[(size_t)q] = found;
      }
    }
    // :1706-1726
    std::vector<int> v(AMREX_SPACEDIM);
    for (int64_t t = 0; t < ne[f]; ++t) {
      for (int k = 0; k < AMREX_SPACEDIM; ++k) v[k] = PMI_N_map[(size_t)elts[(oe + t) * AMREX_SPACEDIM + k]]->m_idx;
#if AMREX_SPACEDIM == 2
      if (v[0] != v[1]) eltSet.insert(Element(v));
#else
      const bool degenerate = (v[0] == v[1] || v[1] == v[2] || v[0] == v[2]);
      if (!degenerate) eltSet.insert(Element(v));
#endif
    }
    ov += nv[f];
    oe += ne[f];
  }
  // :1751-1754, :1777-1784
  std::vector<std::set<Node>::iterator> sortedNodes(nodeSet.size());
  for (std::set<Node>::iterator it = nodeSet.begin(); it != nodeSet.end(); ++it) sortedNodes[it->m_idx] = it;
  for (size_t i = 0; i < sortedNodes.size(); ++i) {
    const Real* vec = sortedNodes[i]->m_vec;
    const int N = sortedNodes[i]->m_size;
    for (int j = 0; j < N; ++j) nodes_out[i * N + j] = vec[j];
  }
  // :1790-1807
  int64_t cnt = 0;
  for (std::set<Element>::const_iterator it = eltSet.begin(); it != eltSet.end(); ++it) {
    for (int j = 0; j < AMREX_SPACEDIM; ++j) elts_out[cnt * AMREX_SPACEDIM + j] = (*it)[j];
    ++cnt;
  }
  *nn_out = (int64_t)nodeSet.size();
  *nelt_out = cnt;
  // code 4 (ours, after the outputs are written: the reference itself ran through and this IS its answer): equivalent
  {  // nodes are closer than epsilon_DEF, so they sit in the same or in neighbouring cells of a 1e-14 grid
    const double H = 1.0e-14;
    std::map<std::vector<long long>, std::vector<const Node*>> grid;
    for (std::set<Node>::iterator it = nodeSet.begin(); it != nodeSet.end(); ++it) {
      std::vector<long long> g(AMREX_SPACEDIM);
      for (int d = 0; d < AMREX_SPACEDIM; ++d) g[d] = (long long)std::floor((*it)[d] / H);
      std::vector<long long> c(AMREX_SPACEDIM);
      for (int o = 0; o < (AMREX_SPACEDIM == 3 ? 27 : 9); ++o) {
        for (int d = 0, r = o; d < AMREX_SPACEDIM; ++d, r /= 3) c[d] = g[d] + r % 3 - 1;
        auto hit = grid.find(c);
        if (hit == grid.end()) continue;
        for (const Node* q : hit->second)
          if (!(*q < *it) && !(*it < *q)) return 4;
      }
      grid[g].push_back(&*it);
    }
  }
  return 0;
}
