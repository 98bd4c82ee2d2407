// mergemef_ref_wrap.cpp -- C entry points around the REFERENCE's own surface merge.  oracle/Makefile `ref` cuts the
// definition of merge_iso out of Src/mergeMEF.cpp (from the second line that opens with `merge_iso(` -- a forward declaration
// precedes it -- to just before `write_iso`) into oracle/_ref/mergemef_slice.inc at build time and compiles this file into
// oracle/_ref/libmergemef_ref.so against the owning FArrayBox of surf_shim.h.  The slice is never copied into this repository.
// Test infrastructure only: pins tests/surfjoin_ref.py (merge_iso) and, through tests/golden/mergemef_ref.npz, the merge
// kernels of pa_surfjoin.hip.
#include "surf_shim.h"

using namespace amrex;
using std::cerr;
using std::cout;
using std::endl;
using std::map;
using std::string;
using std::vector;

static void  // the slice opens at the function's name
#include "mergemef_slice.inc"  // oracle/_ref/, made by the Makefile from the reference tree

namespace {
vector<double> g_nodes;
vector<int32_t> g_elts;
}  // namespace

// M and S: nodes [n][ncomp] node-major, elts [ne][3] 1-based.  counts = {nodes, elements} of M afterwards.  Returns 1 where
// the reference aborts, 2 where it would divide by zero (:150, :154: a surface without elements) -- it is not called then.
extern "C" int ref_mergemef_run(int64_t n_m, int ncomp, const double* nodes_m, int64_t ne_m, const int32_t* elts_m, int64_t n_s, const double* nodes_s,
                                int64_t ne_s, const int32_t* elts_s, double eps, int rem_dup_nodes, int64_t* counts) {
  if (ne_m == 0 || ne_s == 0) return 2;
  ref_mute quiet;
  FArrayBox nodesM, nodes;
  ref_to_fab(nodesM, nodes_m, n_m, ncomp);
  ref_to_fab(nodes, nodes_s, n_s, ncomp);
  Array<int> faceDataM(elts_m, elts_m + 3 * ne_m), faceData(elts_s, elts_s + 3 * ne_s);
  int nEltsM = (int)ne_m;
  try {
    merge_iso(nodesM, faceDataM, nEltsM, nodes, faceData, (int)ne_s, eps, 0, rem_dup_nodes != 0);
  } catch (const ref_aborted&) {
    return 1;
  }
  ref_from_fab(nodesM, g_nodes);
  g_elts.assign(faceDataM.begin(), faceDataM.end());
  counts[0] = nodesM.box().numPts();
  counts[1] = nEltsM;
  return 0;
}

extern "C" void ref_mergemef_get(double* nodes, int32_t* elts) {
  std::copy(g_nodes.begin(), g_nodes.end(), nodes);
  std::copy(g_elts.begin(), g_elts.end(), elts);
}
