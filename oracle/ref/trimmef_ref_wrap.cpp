// trimmef_ref_wrap.cpp -- C entry points around the REFERENCE's own surface trimming.  oracle/Makefile `ref` cuts
// Src/trimMEFgen.cpp from `surface_area(` to just before `main` (surface_area, trim_surface, trim_surface_RXY,
// remove_unused_nodes, triangle_area) into oracle/_ref/trimmef_slice.inc at build time and compiles this file into
// oracle/_ref/libtrimmef_ref.so against the owning FArrayBox of surf_shim.h.  The slice is never copied into this repository.
// Test infrastructure only: pins tests/surfcut_ref.py (trim_surface, triangle_areas) and, through
// tests/golden/trimmef_ref.npz, the trim and area kernels of pa_surfcut.hip.
// What is OURS here, and restated from main(): the order of the calls (:433-458, :524).
#include "surf_shim.h"

using namespace amrex;
using std::cerr;
using std::cout;
using std::endl;
using std::map;
using std::string;
using std::vector;

Real  // the slice opens at the function's name
#include "trimmef_slice.inc"  // oracle/_ref/, made by the Makefile from the reference tree

namespace {
const char* SIGN[5] = {"lt", "le", "gt", "ge", "eq"};
vector<double> g_nodes;
vector<int32_t> g_elts;
}  // namespace

// nodes [nnodes][ncomp] node-major, elts [nelts][3] 1-based; conditions (comps, signs as 0..4 = lt le gt ge eq, vals); rxy < 0:
// no radius.  counts = {nodes left, elements left, nodes removed as unused}.  Returns 1 where the reference aborts.
extern "C" int ref_trimmef_run(int64_t nnodes, int ncomp, const double* nodes_in, int64_t nelts, const int32_t* elts, int nconds,
                               const int32_t* comps_in, const int32_t* signs_in, const double* vals_in, double RXY, int sign_rxy, int64_t* counts) {
  ref_mute quiet;
  FArrayBox nodes;
  ref_to_fab(nodes, nodes_in, nnodes, ncomp);
  Vector<int> faceData(elts, elts + 3 * nelts);
  const int nodesPerElt = 3;
  try {
    if (nconds > 0) {  // :433-451
      Vector<int> comps(comps_in, comps_in + nconds);
      Vector<string> signs((size_t)nconds);
      for (int i = 0; i < nconds; ++i) signs[i] = SIGN[signs_in[i]];
      Vector<Real> vals(vals_in, vals_in + nconds);
      trim_surface(comps, signs, vals, nodes, faceData, nodesPerElt);
    }
    if (RXY >= 0) {  // :453-458
      string sign_RXY = SIGN[sign_rxy];
      trim_surface_RXY(sign_RXY, RXY, nodes, faceData, nodesPerElt);
    }
    const long before = nodes.box().numPts();
    remove_unused_nodes(nodes, faceData, nodesPerElt);  // :524
    counts[2] = before - nodes.box().numPts();
  } catch (const ref_aborted&) {
    return 1;
  }
  ref_from_fab(nodes, g_nodes);
  g_elts.assign(faceData.begin(), faceData.end());
  counts[0] = nodes.box().numPts();
  counts[1] = (int64_t)(g_elts.size() / 3);
  return 0;
}

extern "C" void ref_trimmef_get(double* nodes, int32_t* elts) {
  std::copy(g_nodes.begin(), g_nodes.end(), nodes);
  std::copy(g_elts.begin(), g_elts.end(), elts);
}

// per [nelts]: surface_area (:53-87) of each element on its own (0 + its term: the term), and triangle_area (:374-409);
// the return value is surface_area of the whole surface, the reference's serial sum
extern "C" double ref_trimmef_areas(int64_t nnodes, int ncomp, const double* nodes_in, int64_t nelts, const int32_t* elts, double* per, double* tri) {
  FArrayBox nodes;
  ref_to_fab(nodes, nodes_in, nnodes, ncomp);
  Vector<int> faceData(elts, elts + 3 * nelts), one(3);
  for (int64_t k = 0; k < nelts; ++k) {
    for (int j = 0; j < 3; ++j) one[j] = elts[3 * k + j];
    per[k] = surface_area(nodes, one, 3);
  }
  triangle_area(nodes.dataPtr(0), nodes.dataPtr(1), nodes.dataPtr(2), faceData, (int)nelts, (int)nnodes, tri);
  return surface_area(nodes, faceData, 3);
}
