// binmef_ref_wrap.cpp -- C entry points around the REFERENCE's own surface binning.  oracle/Makefile `ref` cuts
// Src/binMEF.cpp from `Real triangleArea(` to just before `main` (triangleArea, orderNodes, findDE, findFG, getBin,
// satisfyCondition, processTriangle, with the statics areaOutsideCondition and NmyTriangles) into
// oracle/_ref/binmef_slice.inc at build time and compiles this file into oracle/_ref/libbinmef_ref.so.  The slice is never
// copied into this repository.  Test infrastructure only: pins tests/binmef_ref.py and, through the recorded outputs
// (tests/golden/binmef_ref.npz), the kernels of peleanalysis_amd/csrc/pa_binmef.hip to the reference's compiled code.
// What is OURS here, and restated from main(): the bin edges (:477-489) and the element loop (:522-540).  `map` names a
// recording type: the reference's `bins[AbinI] += area` appends (bin vector, area), so its leaves come out in visiting order
// and the caller forms the serial sums from them in that order.
#include "surf_shim.h"

using namespace amrex;
using std::pow;
using std::vector;

namespace {
struct Leaf {
  vector<int> bin;
  double area;
};
vector<Leaf> g_leaves;
}  // namespace

template <class K, class V>
struct map {
  struct Proxy {
    const K& key;
    void operator+=(V a) { g_leaves.push_back(Leaf{key, a}); }
  };
  Proxy operator[](const K& k) { return Proxy{k}; }
};

#include "binmef_slice.inc"  // oracle/_ref/, made by the Makefile from the reference tree

// nodes [nnodes][ncomp] node-major, elts [nelts][3] 1-based.  Returns 0, or 1 where the reference's AMREX_ALWAYS_ASSERT on
// the split fractions (:121, :159) fired (the leaves so far stay readable).  counts = {leaves, NmyTriangles}; sums =
// {areaOutsideCondition, the serial total of triangleArea over the elements (:535)}.
extern "C" int ref_binmef_run(int64_t nnodes, int ncomp, const double* nodes, int64_t nelts, const int32_t* elts, int nc, const int32_t* bin_comps,
                              const double* bin_min, const double* bin_max, const int32_t* nbins, double area_eps, int cond_apply, int cond_comp,
                              double cond_val, int cond_sgn, int64_t* counts, double* sums) {
  vector<vector<Real> > nodeVec((size_t)nnodes);
  for (int64_t i = 0; i < nnodes; ++i) nodeVec[(size_t)i].assign(nodes + i * ncomp, nodes + (i + 1) * ncomp);
  vector<int> binComps(bin_comps, bin_comps + nc), nBins(nbins, nbins + nc);
  vector<Real> binMin(bin_min, bin_min + nc), binMax(bin_max, bin_max + nc);
  // :477-489
  vector<Real> dBin(nc);
  for (int i = 0; i < nc; ++i) dBin[i] = (binMax[i] - binMin[i]) / nBins[i];
  vector<vector<Real> > binLO(nc);
  for (int j = 0; j < nc; ++j) {
    binLO[j].resize(nBins[j]);
    for (int i = 0; i < nBins[j]; ++i) binLO[j][i] = binMin[j] + i * dBin[j];
  }
  g_leaves.clear();
  NmyTriangles = 0;
  areaOutsideCondition = 0.;
  Real area = 0;
  map<vector<int>, Real> bins;
  int rc = 0;
  try {
    // :522-540
    for (int64_t i = 0; i < nelts; ++i) {
      const vector<Real>& A = nodeVec[elts[3 * i + 0] - 1];
      const vector<Real>& B = nodeVec[elts[3 * i + 1] - 1];
      const vector<Real>& C = nodeVec[elts[3 * i + 2] - 1];
      vector<int> Abin = getBin(A, binComps, binLO, binMax);
      vector<int> Bbin = getBin(B, binComps, binLO, binMax);
      vector<int> Cbin = getBin(C, binComps, binLO, binMax);
      area += triangleArea(A, B, C);
      processTriangle(A, Abin, B, Bbin, C, Cbin, bins, binLO, binMax, area_eps, binComps, cond_comp, cond_val, cond_sgn, cond_apply != 0);
    }
  } catch (const ref_assert_failed&) {
    rc = 1;
  }
  counts[0] = (int64_t)g_leaves.size();
  counts[1] = (int64_t)NmyTriangles;
  sums[0] = areaOutsideCondition;
  sums[1] = area;
  return rc;
}

// the leaves of the last run, in visiting order: bins [leaves][nc], areas [leaves]
extern "C" void ref_binmef_leaves(int nc, int32_t* bins, double* areas) {
  for (size_t q = 0; q < g_leaves.size(); ++q) {
    for (int j = 0; j < nc; ++j) bins[q * nc + j] = g_leaves[q].bin[j];
    areas[q] = g_leaves[q].area;
  }
}

// triangleArea (:46-60) of one triangle
extern "C" double ref_binmef_triangle_area(const double* p0, const double* p1, const double* p2) {
  return triangleArea(vector<Real>(p0, p0 + 3), vector<Real>(p1, p1 + 3), vector<Real>(p2, p2 + 3));
}
