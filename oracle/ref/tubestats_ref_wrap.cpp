// tubestats_ref_wrap.cpp -- C entry points around the REFERENCE's own stream-tube arithmetic.  oracle/Makefile `ref` cuts three
// parts of Src/streamTubeStats.cpp into oracle/_ref/ at build time and compiles this file into oracle/_ref/libtubestats_ref.so
// against the IntVect, Box, FArrayBox and MultiFab of surf_shim.h:
//   tubestats_mlloc.inc  struct MLloc
//   tubestats_edge.inc   `struct Edge` to just before `main` (EdgeLT, NeighborMap, buildNodeNeighbors, smoothVals)
//   tubestats_slice.inc  `tetVol(const Real* A,` to just before the definition of ml_Nlevels (tetVol, max_grad, peak_val,
//                        wedge_volume_int, wedge_surf_area, build_nodeMap)
// The slices are never copied into this repository.  Test infrastructure only: pins tests/tubestats_ref.py and, through
// tests/golden/tubestats_ref.npz, the kernels of pa_tubestats.hip.
// What is OURS here: one level of FABs built from flat tables, and the loops over elements and nodes around the calls.
#include "surf_shim.h"

using namespace amrex;
using std::cerr;
using std::cout;
using std::endl;
using std::map;
using std::ostream;
using std::pair;
using std::set;
using std::string;
using std::vector;

#include "tubestats_mlloc.inc"  // oracle/_ref/, made by the Makefile from the reference tree
#include "tubestats_edge.inc"
Real  // the slice opens at the function's name
#include "tubestats_slice.inc"

namespace {
MultiFab g_mf;
std::vector<MLloc> g_map;
Vector<Vector<int> > g_nb;
const int IDX[3] = {0, 1, 2};

Vector<const MLloc*> corners(const int32_t* face, int64_t e) {
  Vector<const MLloc*> p(3);
  for (int k = 0; k < 3; ++k) p[k] = &g_map[(size_t)face[3 * e + k] - 1];
  return p;
}
}  // namespace

// Str boxes in order: desc [nbox][3] = (ni, nj, jlo), data = every box's [ncomp][nj][ni] one after the other (X Y Z first),
// ins_off [nbox + 1] / ins_ids = the 1-based node ids of every box, in line order.  build_nodeMap is the reference's.  -> nNodes
extern "C" int64_t ref_tube_load(int nbox, const int64_t* desc, int ncomp, const double* data, const int64_t* ins_off, const int32_t* ins_ids) {
  g_mf.fabs.assign((size_t)nbox, FArrayBox());
  Vector<Vector<Vector<int> > > inside(1);
  inside[0].resize((size_t)nbox);
  for (int g = 0; g < nbox; ++g) {
    const int ni = (int)desc[3 * g], nj = (int)desc[3 * g + 1], jlo = (int)desc[3 * g + 2];
    FArrayBox& f = g_mf.fabs[(size_t)g];
    f.resize(Box(IntVect(0, jlo, 0), IntVect(ni - 1, jlo + nj - 1, 0)), ncomp);
    std::copy(data, data + (long)ncomp * ni * nj, f.dataPtr());
    data += (long)ncomp * ni * nj;
    inside[0][(size_t)g].assign(ins_ids + ins_off[g], ins_ids + ins_off[g + 1]);
  }
  g_map = build_nodeMap(inside);
  return (int64_t)g_map.size();
}

// per element: wedge_volume_int over pt .. pt + 1 (comp < 0: the volume), wedge_surf_area at pt.  Returns 1 where a box does not
// hold the point (the reference reads outside its FAB there).
extern "C" int ref_tube_wedges(int64_t nelts, const int32_t* face, int pt, int comp, double* vol, double* area) {
  Vector<MultiFab*> data(1, &g_mf);
  Vector<int> idX(IDX, IDX + 3);
  try {
    for (int64_t e = 0; e < nelts; ++e) {
      const Vector<const MLloc*> p = corners(face, e);
      if (vol) vol[e] = wedge_volume_int(p, pt, comp, data, idX);
      if (area) area[e] = wedge_surf_area(p, data, idX, pt);
    }
  } catch (const std::out_of_range&) {
    return 1;
  }
  return 0;
}

// per node: max_grad of component comp
extern "C" void ref_tube_max_grad(int comp, double* out) {
  Vector<MultiFab*> data(1, &g_mf);
  Vector<int> idX(IDX, IDX + 3);
  for (size_t n = 0; n < g_map.size(); ++n) out[n] = max_grad(g_map[n], comp, data, idX);
}

// per node: peak_val of component pcomp, samples [ns][nNodes], ok [nNodes]
extern "C" void ref_tube_peaks(int pcomp, int ns, const int32_t* sample_comps, double* samples, uint8_t* ok) {
  ref_mute quiet;
  Vector<MultiFab*> data(1, &g_mf);
  Vector<int> sc(sample_comps, sample_comps + ns);
  Vector<Real> got((size_t)ns);
  for (size_t n = 0; n < g_map.size(); ++n) {
    bool good = false;
    peak_val(g_map[n], pcomp, sc, got, &good, data);
    for (int s = 0; s < ns; ++s) samples[(size_t)s * g_map.size() + n] = got[(size_t)s];
    ok[n] = good ? 1 : 0;
  }
}

// buildNodeNeighbors; -> the number of entries; rowptr [nelts + 1] is written, the lists are kept for the two calls below
extern "C" int64_t ref_tube_neighbors(int64_t nelts, const int32_t* face, int nnodes, int64_t* rowptr) {
  const Vector<int> faceData(face, face + 3 * nelts);
  g_nb = buildNodeNeighbors(faceData, nnodes);
  rowptr[0] = 0;
  for (size_t i = 0; i < g_nb.size(); ++i) rowptr[i + 1] = rowptr[i] + (int64_t)g_nb[i].size();
  return rowptr[g_nb.size()];
}

extern "C" void ref_tube_neighbor_cols(int32_t* cols) {
  for (size_t i = 0; i < g_nb.size(); ++i)
    for (size_t k = 0; k < g_nb[i].size(); ++k) *cols++ = g_nb[i][k];
}

// one pass of smoothVals over the lists of the last ref_tube_neighbors
extern "C" void ref_tube_smooth(int64_t nelts, const double* vals, const double* area, double* out) {
  const Vector<Real> v(vals, vals + nelts), a(area, area + nelts);
  Vector<Real> nv((size_t)nelts);
  smoothVals(nv, v, a, g_nb);
  std::copy(nv.begin(), nv.end(), out);
}
