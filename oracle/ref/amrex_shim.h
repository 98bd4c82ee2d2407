// amrex_shim.h -- the sliver of AMReX that the arithmetic of the REFERENCE's Src/isosurface.cpp needs (Edge :50
// through Element :930: VI_doIt, VertexInterp, Segmentise, Polygonise with its two tables, Node::operator<, Element).
// Our own code; test infrastructure only.  oracle/Makefile `ref` cuts that part out of the reference at build time
// into oracle/_ref/ and compiles it against this header (oracle/ref/iso_ref_wrap.cpp); nothing of the reference's text
// is kept in this repository.
//
// Everything below is a plain restatement of an interface.  Two facts are RECALLED from AMReX, not compiled from it,
// and the results depend on both:
//   (1) IntVect::operator< is lexicographic with the LAST index most significant.  std::map<Edge, Point> is ordered by
//       it, and the vertex ids of a FAB are positions in that map.
//   (2) Box::next runs x fastest (restated by the loops of iso_ref_wrap.cpp, not here).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include <list>
#include <map>
#include <set>
#include <string>
#include <vector>

#if !defined(AMREX_SPACEDIM) || (AMREX_SPACEDIM != 2 && AMREX_SPACEDIM != 3)
#error "compile with -DAMREX_SPACEDIM=2 or -DAMREX_SPACEDIM=3"
#endif

#define AMREX_ASSERT(x) ((void)0)
#if AMREX_SPACEDIM == 2
#define AMREX_D_TERM(a, b, c) a b
#else
#define AMREX_D_TERM(a, b, c) a b c
#endif

namespace amrex {

using Real = double;

template <class T>
struct Vector : public std::vector<T> {
  using std::vector<T>::vector;
  T* dataPtr() noexcept { return this->data(); }
  const T* dataPtr() const noexcept { return this->data(); }
};

struct IntVect {
  int vect[AMREX_SPACEDIM];
  IntVect() {
    for (int d = 0; d < AMREX_SPACEDIM; ++d) vect[d] = 0;
  }
  int& operator[](int d) { return vect[d]; }
  int operator[](int d) const { return vect[d]; }
  bool operator==(const IntVect& r) const {
    for (int d = 0; d < AMREX_SPACEDIM; ++d)
      if (vect[d] != r.vect[d]) return false;
    return true;
  }
  // RECALLED fact (1): lexicographic, last index most significant
  bool operator<(const IntVect& r) const {
    for (int d = AMREX_SPACEDIM - 1; d >= 0; --d)
      if (vect[d] != r.vect[d]) return vect[d] < r.vect[d];
    return false;
  }
  IntVect operator+(const IntVect& r) const {
    IntVect o;
    for (int d = 0; d < AMREX_SPACEDIM; ++d) o.vect[d] = vect[d] + r.vect[d];
    return o;
  }
};

inline IntVect BASISV(int dir) {
  IntVect o;
  o.vect[dir] = 1;
  return o;
}

// a view of [ncomp][nz][ny][nx] doubles (x fastest, component slowest: the layout of a FAB) over the box lo .. lo + n - 1
struct FArrayBox {
  const Real* p;
  int lo[AMREX_SPACEDIM];
  long n[AMREX_SPACEDIM];
  int ncomp;
  long index(const IntVect& iv) const {
    long o = 0;
    for (int d = AMREX_SPACEDIM - 1; d >= 0; --d) o = o * n[d] + (iv[d] - lo[d]);
    return o;
  }
  long npts() const {
    long m = 1;
    for (int d = 0; d < AMREX_SPACEDIM; ++d) m *= n[d];
    return m;
  }
  int nComp() const { return ncomp; }
  Real operator()(const IntVect& iv, int comp = 0) const { return p[comp * npts() + index(iv)]; }
  void getVal(Real* data, const IntVect& iv) const {
    const long o = index(iv), m = npts();
    for (int c = 0; c < ncomp; ++c) data[c] = p[c * m + o];
  }
};

}  // namespace amrex
