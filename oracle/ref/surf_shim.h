// surf_shim.h -- the sliver of AMReX / BoxLib that the arithmetic of the REFERENCE's surface tools needs: Src/binMEF.cpp
// (triangleArea through processTriangle), Src/sliceMEF.cpp (the types, FindMySeg through Segmentise, the body of the
// loop over the locations), Src/trimMEFgen.cpp (surface_area through triangle_area), Src/mergeMEF.cpp (merge_iso) and
// Src/streamTubeStats.cpp (MLloc, Edge through smoothVals, tetVol through build_nodeMap).
// Our own code; test infrastructure only.  oracle/Makefile `ref` cuts those parts out of the reference at build time
// into oracle/_ref/*.inc and compiles them against this header (oracle/ref/*_ref_wrap.cpp); nothing of the reference's
// text is kept in this repository.  amrex_shim.h serves the isosurface libraries and is left as it is.
//
// Everything below is a plain restatement of an interface.  These facts are RECALLED from AMReX, not compiled from
// it, and the results depend on them:
//   (1) A FArrayBox holds its components one after the other, x fastest within one: dataPtr(c)[i] is component c of point
//       i, fab(iv, c) the same by index.  resize() keeps nothing (the new storage is filled with NaN here, so a value the
//       reference never wrote shows).  copy(src) copies every component over the intersection of the two boxes.  A MultiFab
//       is indexed by the number of the box.  A point outside the FAB throws here (the reference would read past it).
//   (2) IntVect::operator<= is "not lexicographically greater", last index most significant; Box::next runs x fastest and
//       leaves the box through the LAST index.  On the one-row boxes (0,0,0)..(n-1,0,0) the tools use,
//       `for (iv = smallEnd(); iv <= bigEnd(); next(iv))` therefore visits 0 .. n-1, and nothing for n = 0.
//   (3) Box::numPts of a box with hi < lo is 0 here (trimming every node away leaves (0,0,0)..(-1,0,0)); AMReX asserts
//       box.ok() only in debug builds.  growHi(d, n) adds n to the upper end.
//   (4) BL_ASSERT is off in an optimised build; AMREX_ALWAYS_ASSERT is always on (here it throws; the wrappers return a
//       code).  Abort ends the program (here it throws).  ParallelDescriptor::IOProcessor() is true on one rank.
//   (5) Array<T> (BoxLib) and Vector<T> (AMReX) are std::vector<T> with dataPtr().
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <list>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#define BL_SPACEDIM 3
#define AMREX_SPACEDIM 3
#define AMREX_D_DECL(a, b, c) a, b, c
#define BL_ASSERT(x) ((void)0)
#define AMREX_ASSERT(x) ((void)0)

struct ref_assert_failed {};
struct ref_aborted {
  std::string what;
};
#define AMREX_ALWAYS_ASSERT(x) \
  do {                         \
    if (!(x)) throw ref_assert_failed(); \
  } while (0)

namespace amrex {

using Real = double;

template <class T>
struct Vector : public std::vector<T> {
  using std::vector<T>::vector;
  T* dataPtr() noexcept { return this->data(); }
  const T* dataPtr() const noexcept { return this->data(); }
};
template <class T>
using Array = Vector<T>;

[[noreturn]] inline void Abort(const char* msg) { throw ref_aborted{msg}; }
[[noreturn]] inline void Abort(const std::string& msg) { throw ref_aborted{msg}; }

namespace ParallelDescriptor {
inline bool IOProcessor() { return true; }
}  // namespace ParallelDescriptor

struct IntVect {
  int vect[3];
  IntVect() : vect{0, 0, 0} {}
  IntVect(int i, int j, int k) : vect{i, j, k} {}
  static IntVect TheZeroVector() { return IntVect(); }
  int& operator[](int d) { return vect[d]; }
  int operator[](int d) const { return vect[d]; }
  // RECALLED fact (2)
  bool operator<(const IntVect& r) const {
    for (int d = 2; d >= 0; --d)
      if (vect[d] != r.vect[d]) return vect[d] < r.vect[d];
    return false;
  }
  bool operator<=(const IntVect& r) const { return !(r < *this); }
  IntVect operator+(const IntVect& r) const { return IntVect(vect[0] + r[0], vect[1] + r[1], vect[2] + r[2]); }
  IntVect& operator+=(const IntVect& r) {
    for (int d = 0; d < 3; ++d) vect[d] += r[d];
    return *this;
  }
};
inline IntVect operator*(int s, const IntVect& v) { return IntVect(s * v[0], s * v[1], s * v[2]); }
inline IntVect BASISV(int dir) {
  IntVect o;
  o[dir] = 1;
  return o;
}

struct Box {
  IntVect lo, hi;
  Box() : lo(), hi(-1, -1, -1) {}
  Box(const IntVect& l, const IntVect& h) : lo(l), hi(h) {}
  const IntVect& smallEnd() const { return lo; }
  const IntVect& bigEnd() const { return hi; }
  int length(int d) const { return hi[d] - lo[d] + 1; }
  // RECALLED fact (3)
  long numPts() const {
    long m = 1;
    for (int d = 0; d < 3; ++d) m *= std::max(0, length(d));
    return m;
  }
  bool numPtsOK() const { return true; }
  // RECALLED fact (2)
  void next(IntVect& iv) const {
    for (int d = 0; d < 3; ++d) {
      if (++iv[d] <= hi[d] || d == 2) return;
      iv[d] = lo[d];
    }
  }
  Box& growHi(int d, int n) {
    hi[d] += n;
    return *this;
  }
};

// an owning FAB; RECALLED fact (1)
class FArrayBox {
 public:
  FArrayBox() : m_nc(0) {}
  FArrayBox(const Box& b, int nc) { resize(b, nc); }
  const Box& box() const { return m_box; }
  int nComp() const { return m_nc; }
  Real* dataPtr(int c = 0) { return m_d.data() + (long)c * m_box.numPts(); }
  const Real* dataPtr(int c = 0) const { return m_d.data() + (long)c * m_box.numPts(); }
  long index(const IntVect& iv) const {
    long o = 0;
    for (int d = 2; d >= 0; --d) {
      if (iv[d] < m_box.lo[d] || iv[d] > m_box.hi[d]) throw std::out_of_range("surf_shim.h: a point outside the FAB");  // ours: BL_ASSERT is off
      o = o * m_box.length(d) + (iv[d] - m_box.lo[d]);
    }
    return o;
  }
  Real& operator()(const IntVect& iv, int c = 0) { return dataPtr(c)[index(iv)]; }
  const Real& operator()(const IntVect& iv, int c = 0) const { return dataPtr(c)[index(iv)]; }
  void resize(const Box& b, int nc) {
    m_box = b;
    m_nc = nc;
    m_d.assign((size_t)(b.numPts() * nc), std::numeric_limits<Real>::quiet_NaN());
  }
  void clear() {
    m_box = Box();
    m_nc = 0;
    m_d.clear();
  }
  FArrayBox& copy(const FArrayBox& src) {
    IntVect a, b;
    for (int d = 0; d < 3; ++d) {
      a[d] = std::max(m_box.lo[d], src.m_box.lo[d]);
      b[d] = std::min(m_box.hi[d], src.m_box.hi[d]);
    }
    for (int c = 0; c < std::min(m_nc, src.m_nc); ++c)
      for (int k = a[2]; k <= b[2]; ++k)
        for (int j = a[1]; j <= b[1]; ++j)
          for (int i = a[0]; i <= b[0]; ++i) (*this)(IntVect(i, j, k), c) = src(IntVect(i, j, k), c);
    return *this;
  }

 private:
  Box m_box;
  int m_nc;
  std::vector<Real> m_d;
};

// the FABs of one level, by index
struct MultiFab {
  std::vector<FArrayBox> fabs;
  FArrayBox& operator[](int i) { return fabs[(size_t)i]; }
  const FArrayBox& operator[](int i) const { return fabs[(size_t)i]; }
  int size() const { return (int)fabs.size(); }
  int nComp() const { return fabs.empty() ? 0 : fabs[0].nComp(); }
};

}  // namespace amrex

namespace BoxLib {
using amrex::Abort;
using amrex::BASISV;
}  // namespace BoxLib

// the tools talk on std::cout / std::cerr while they compute; a wrapper holds one of these for the length of a call
struct ref_mute {
  std::ostringstream sink;
  std::streambuf *out, *err;
  ref_mute() : out(std::cout.rdbuf(sink.rdbuf())), err(std::cerr.rdbuf(sink.rdbuf())) {}
  ~ref_mute() {
    std::cout.rdbuf(out);
    std::cerr.rdbuf(err);
  }
};

// node-major [n][nc] doubles <-> a FAB over (0,0,0)..(n-1,0,0)
inline void ref_to_fab(amrex::FArrayBox& f, const double* nodes, int64_t n, int nc) {
  f.resize(amrex::Box(amrex::IntVect(), amrex::IntVect((int)n - 1, 0, 0)), nc);
  for (int c = 0; c < nc; ++c)
    for (int64_t i = 0; i < n; ++i) f.dataPtr(c)[i] = nodes[i * nc + c];
}
inline void ref_from_fab(const amrex::FArrayBox& f, std::vector<double>& out) {
  const long n = f.box().numPts();
  const int nc = f.nComp();
  out.assign((size_t)(n * nc), 0.0);
  for (int c = 0; c < nc; ++c)
    for (long i = 0; i < n; ++i) out[(size_t)(i * nc + c)] = f.dataPtr(c)[i];
}
