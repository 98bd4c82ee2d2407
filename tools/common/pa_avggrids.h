// pa_avggrids.h -- the output BoxArray of one level of avgPlotfiles3d (avgPlotfiles.cpp:141-152, :161-163).  Host arithmetic on
// boxes only and nothing else included, so that a stand-alone program can be built from it (tools/src/avgGridsCheck.cpp: the
// sanitizer build of tests/test_avgplt_ref.py).  B: any box type with inclusive int lo[3], hi[3].
//
// Where every file that has the level holds the same box list, that list is kept unchanged (:146).  Elsewhere the reference
// catenates the lists, calls BoxArray::removeOverlap and then maxSize(output_max_grid_size); removeOverlap's decomposition is
// not restated -- ANY disjoint set of boxes with the same union is a correct BoxArray for the output, and the value of a cell
// does not depend on it.  Here: every box minus the boxes before it, then chopped.
#pragma once
#include <cstddef>
#include <vector>

namespace pa {

template <typename B>
inline bool same_box_list(const std::vector<B>& a, const std::vector<B>& b) {  // BoxList::operator!=, :146
  if (a.size() != b.size()) return false;
  for (std::size_t i = 0; i < a.size(); ++i)
    for (int d = 0; d < 3; ++d)
      if (a[i].lo[d] != b[i].lo[d] || a[i].hi[d] != b[i].hi[d]) return false;
  return true;
}

// b minus c as disjoint boxes appended to out (at most 6)
template <typename B>
inline void box_subtract(const B& b, const B& c, std::vector<B>& out) {
  int lo[3], hi[3];
  for (int d = 0; d < 3; ++d) {
    lo[d] = b.lo[d] > c.lo[d] ? b.lo[d] : c.lo[d];
    hi[d] = b.hi[d] < c.hi[d] ? b.hi[d] : c.hi[d];
    if (lo[d] > hi[d]) { out.push_back(b); return; }
  }
  B cur = b;
  for (int d = 0; d < 3; ++d) {
    if (cur.lo[d] < lo[d]) { B p = cur; p.hi[d] = lo[d] - 1; out.push_back(p); cur.lo[d] = lo[d]; }
    if (cur.hi[d] > hi[d]) { B p = cur; p.lo[d] = hi[d] + 1; out.push_back(p); cur.hi[d] = hi[d]; }
  }
}

template <typename B>
inline std::vector<B> disjoint_cover(const std::vector<B>& in) {
  std::vector<B> done, pieces, next;
  for (const B& b : in) {
    pieces.assign(1, b);
    for (std::size_t c = 0, nc = done.size(); c < nc && !pieces.empty(); ++c) {
      next.clear();
      for (const B& p : pieces) box_subtract(p, done[c], next);
      pieces.swap(next);
    }
    done.insert(done.end(), pieces.begin(), pieces.end());
  }
  return done;
}

// BoxArray::maxSize: every box in pieces of at most n cells per direction (even split)
template <typename B>
inline std::vector<B> chop_max_size(const std::vector<B>& in, int n) {
  std::vector<B> out;
  for (const B& b : in) {
    int parts[3], base[3], rem[3];
    for (int d = 0; d < 3; ++d) {
      const int len = b.hi[d] - b.lo[d] + 1;
      parts[d] = (len + n - 1) / n;
      base[d] = len / parts[d];
      rem[d] = len % parts[d];
    }
    auto start = [&](int d, int p) { return b.lo[d] + p * base[d] + (p < rem[d] ? p : rem[d]); };
    for (int z = 0; z < parts[2]; ++z)
      for (int y = 0; y < parts[1]; ++y)
        for (int x = 0; x < parts[0]; ++x) {
          B p = b;
          const int q[3] = {x, y, z};
          for (int d = 0; d < 3; ++d) { p.lo[d] = start(d, q[d]); p.hi[d] = start(d, q[d] + 1) - 1; }
          out.push_back(p);
        }
  }
  return out;
}

// lists: the level's box list of every file that has the level, in infiles order (at least one)
template <typename B>
inline std::vector<B> avg_level_grids(const std::vector<std::vector<B>>& lists, int max_grid_size, bool* all_same = nullptr) {
  bool same = true;
  for (std::size_t f = 1; f < lists.size(); ++f) same = same && same_box_list(lists[0], lists[f]);
  if (all_same) *all_same = same;
  if (same) return lists[0];
  std::vector<B> all;
  for (const auto& l : lists) all.insert(all.end(), l.begin(), l.end());
  return chop_max_size(disjoint_cover(all), max_grid_size);
}

}  // namespace pa
