// slicemef_ref_wrap.cpp -- C entry points around the REFERENCE's own surface slicing.  oracle/Makefile `ref` cuts three
// parts of Src/sliceMEF.cpp into oracle/_ref/ at build time and compiles this file into oracle/_ref/libslicemef_ref.so:
//   slicemef_types.inc  the line of epsilon_DEF, and `typedef Array<Real> Point;` to just before `main` (Edge, PMap, vertCache,
//                       vertVec, Segment, the comparisons, the declarations)
//   slicemef_funcs.inc  the definition of FindMySeg to the end of the file (Segment's members, VI_doIt, VertexInterp, Segmentise)
//   slicemef_body.inc   the body of `for (int k=0; k<loc.size(); ++k)` up to `string outfileRoot = rootName`: the element loop,
//                       the numbering of the vertices, the walk along the segments and the joining of the line fragments
// The slices are never copied into this repository.  Test infrastructure only: pins tests/surfcut_ref.py (slice_surface,
// contour_lines) and, through tests/golden/slicemef_ref.npz, pa_surfcut.hip and tools/common/pa_contour.h.
// What is OURS here: the variables of main() that the loop body reads (GridPts :231-237, faceData, nElts, nodesPerElt, dir, loc,
// names), declared around the included body, and the copy of its results.
#include "surf_shim.h"

using namespace amrex;
using std::cerr;
using std::cout;
using std::endl;
using std::list;
using std::map;
using std::pair;
using std::set;
using std::string;
using std::vector;

#include "slicemef_types.inc"  // oracle/_ref/, made by the Makefile from the reference tree
#include "slicemef_funcs.inc"

namespace {
vector<double> g_verts;
vector<int32_t> g_pairs, g_segs, g_lines, g_line_off;
}  // namespace

// nodes [nnodes][ncomp] node-major, elts [nelts][3] 1-based; one location.  counts = {vertices, segments, lines, segments on the lines}
extern "C" int ref_slicemef_run(int64_t nnodes, int ncomp, const double* nodes, int64_t nelts, const int32_t* elts, int dir_, double location,
                                int64_t* counts) {
  ref_mute quiet;
  const int nComp = ncomp;
  vector<Point> GridPts((size_t)nnodes);  // :231-237
  for (int64_t i = 0; i < nnodes; ++i) {
    GridPts[(size_t)i].resize(nComp);
    for (int j = 0; j < nComp; ++j) GridPts[(size_t)i][j] = nodes[i * nComp + j];
  }
  Array<int> faceData(elts, elts + 3 * nelts);
  int nElts = (int)nelts;
  const int nodesPerElt = 3;
  int dir = dir_;
  Array<Real> loc(1, location);
  vector<string> names((size_t)nComp, string("c"));
  vertCache.clear();
  vertVec.clear();
  g_verts.clear();
  g_pairs.clear();
  g_segs.clear();
  g_lines.clear();
  g_line_off.assign(1, 0);
  for (int k = 0; k < loc.size(); ++k)
#include "slicemef_body.inc"  // opens the loop's brace; `segments`, `cLines`, vertCache and vertVec hold the result
    for (PMapIt it = vertCache.begin(); it != vertCache.end(); ++it) {
      g_pairs.push_back(it->first.first);
      g_pairs.push_back(it->first.second);
      for (int j = 0; j < nComp; ++j) g_verts.push_back(it->second.first[j]);
    }
    for (SegList::const_iterator it = segments.begin(); it != segments.end(); ++it) {
      g_segs.push_back(it->ID_l());
      g_segs.push_back(it->ID_r());
    }
    for (std::list<SegList>::iterator it = cLines.begin(); it != cLines.end(); ++it) {
      for (SegList::const_iterator its = it->begin(); its != it->end(); ++its) {
        g_lines.push_back(its->ID_l());
        g_lines.push_back(its->ID_r());
      }
      g_line_off.push_back((int32_t)(g_lines.size() / 2));
    }
    vertCache.clear();  // :441
  }
  counts[0] = (int64_t)(g_pairs.size() / 2);
  counts[1] = (int64_t)(g_segs.size() / 2);
  counts[2] = (int64_t)g_line_off.size() - 1;
  counts[3] = (int64_t)(g_lines.size() / 2);
  return 0;
}

// the last run: verts [nv][ncomp] and pairs [nv][2] in vertCache order, segs [ns][2], lines [nl_segs][2], line_off [nlines + 1]
extern "C" void ref_slicemef_get(double* verts, int32_t* pairs, int32_t* segs, int32_t* lines, int32_t* line_off) {
  std::copy(g_verts.begin(), g_verts.end(), verts);
  std::copy(g_pairs.begin(), g_pairs.end(), pairs);
  std::copy(g_segs.begin(), g_segs.end(), segs);
  std::copy(g_lines.begin(), g_lines.end(), lines);
  std::copy(g_line_off.begin(), g_line_off.end(), line_off);
}

// VI_doIt (:581-605) on two points of ncomp values
extern "C" void ref_slicemef_vi(double val, int comp, int ncomp, const double* p1, const double* p2, double* out) {
  vector<Point> pts(2);
  pts[0].assign(p1, p1 + ncomp);
  pts[1].assign(p2, p2 + ncomp);
  const Point r = VI_doIt(val, comp, pts, 0, 1);
  std::copy(r.begin(), r.end(), out);
}
