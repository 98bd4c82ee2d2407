// pa_contour.h -- the line assembly of sliceMEF.cpp:270-360, kept to the letter, on the host:
//   * start at the left end of the first remaining segment; repeatedly take the FIRST remaining segment that touches the current
//     vertex (FindMySeg :537-546), flipped if necessary, and move to its other end; on a dead end open a new line and continue from
//     the left end of the first remaining segment WITHOUT consuming it (:281-309);
//   * then join fragments until nothing changes (:311-351): the outer fragment's end ids are read once per outer step, so they go
//     stale after a splice, and the three join branches come in the reference's order;
//   * then drop the empty lines (:354-360).
// contour_lines takes "the first remaining segment that touches v" from the incidence CSR (vertex -> its segments in ascending
// segment index, as pa_surf_slice_read returns it) with one cursor per vertex: the first phase is linear in the segments, where
// FindMySeg scans the list (quadratic).  contour_lines_scan is the deliberately plain list scan; both give the same lines for ANY
// segment soup (vertices of degree 3 and more, duplicate segments, segments with both ends on one vertex): tools/src/contourCheck.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <list>
#include <vector>

namespace pa {

struct CSeg { int l, r; };  // vertex ids of the two ends
typedef std::list<std::list<CSeg>> CLines;

namespace contour_detail {
inline bool same(const CSeg& a, const CSeg& b) { return a.l == b.l && a.r == b.r; }

// :311-360
inline void join_fragments(CLines& lines) {
  bool changed;
  do {
    changed = false;
    for (auto it = lines.begin(); it != lines.end(); ++it) {
      if (it->empty()) continue;
      const int idx_l = it->front().l, idx_r = it->back().r;  // read once per outer fragment
      for (auto jt = lines.begin(); jt != lines.end(); ++jt) {
        if (jt->empty() || same(it->front(), jt->front())) continue;
        auto reversed = [&] {
          jt->reverse();
          for (CSeg& s : *jt) { const int t = s.l; s.l = s.r; s.r = t; }
        };
        if (idx_r == jt->front().l) {
          it->splice(it->end(), *jt);
          changed = true;
        } else if (idx_r == jt->back().r) {
          reversed();
          it->splice(it->end(), *jt);
          changed = true;
        } else if (idx_l == jt->front().l) {
          reversed();
          it->splice(it->begin(), *jt);
          changed = true;
        }
      }
    }
  } while (changed);
  lines.remove_if([](const std::list<CSeg>& l) { return l.empty(); });
}
}  // namespace contour_detail

// segs [nsegs] in element order; csr_off [nverts + 1], csr_adj [2 * nsegs]: the segments of each vertex in ascending index (a segment
// with both ends on one vertex is listed twice in that vertex's row)
// the first phase alone (:273-309): the fragments before they are joined
inline CLines contour_walk(const std::vector<CSeg>& segs, const std::vector<int32_t>& csr_off, const std::vector<int32_t>& csr_adj) {
  CLines lines;
  const size_t n = segs.size();
  if (n == 0) return lines;
  std::vector<char> used(n, 0);
  std::vector<int32_t> cur(csr_off.begin(), csr_off.end() - 1);  // per vertex: the first entry of its row that may still be unused
  size_t first = 0, left = n;                                    // the first remaining segment of the list
  int idx = segs[0].l;
  lines.emplace_back();
  while (left > 0) {
    int32_t& c = cur[(size_t)idx];
    const int32_t end = csr_off[(size_t)idx + 1];
    while (c < end && used[(size_t)csr_adj[(size_t)c]]) ++c;
    if (c < end) {
      const int i = csr_adj[(size_t)c];
      const CSeg s = segs[(size_t)i];
      lines.back().push_back(s.l == idx ? s : CSeg{s.r, s.l});
      used[(size_t)i] = 1;
      --left;
      idx = s.l == idx ? s.r : s.l;
    } else {
      while (used[first]) ++first;
      lines.emplace_back();
      idx = segs[first].l;
    }
  }
  return lines;
}
inline CLines contour_lines(const std::vector<CSeg>& segs, const std::vector<int32_t>& csr_off, const std::vector<int32_t>& csr_adj) {
  CLines lines = contour_walk(segs, csr_off, csr_adj);
  contour_detail::join_fragments(lines);
  return lines;
}

// the same by the reference's own means: a list of the remaining segments, scanned from its front for every step
inline CLines contour_walk_scan(const std::vector<CSeg>& segs) {
  CLines lines;
  std::list<CSeg> rest(segs.begin(), segs.end());
  if (rest.empty()) return lines;
  int idx = rest.front().l;
  lines.emplace_back();
  while (!rest.empty()) {
    auto it = rest.begin();
    while (it != rest.end() && it->l != idx && it->r != idx) ++it;
    if (it != rest.end()) {
      const CSeg s = *it;
      lines.back().push_back(s.l == idx ? s : CSeg{s.r, s.l});
      rest.erase(it);
      idx = s.l == idx ? s.r : s.l;
    } else {
      lines.emplace_back();
      idx = rest.front().l;
    }
  }
  return lines;
}
inline CLines contour_lines_scan(const std::vector<CSeg>& segs) {
  CLines lines = contour_walk_scan(segs);
  contour_detail::join_fragments(lines);
  return lines;
}

// the incidence CSR of a segment list on the host (contourCheck, and a caller without a device result)
inline void contour_csr(const std::vector<CSeg>& segs, int nverts, std::vector<int32_t>& off, std::vector<int32_t>& adj) {
  off.assign((size_t)nverts + 1, 0);
  for (const CSeg& s : segs) { ++off[(size_t)s.l + 1]; ++off[(size_t)s.r + 1]; }
  for (int v = 0; v < nverts; ++v) off[(size_t)v + 1] += off[(size_t)v];
  adj.assign(2 * segs.size(), 0);
  std::vector<int32_t> at(off.begin(), off.end() - 1);
  for (size_t i = 0; i < segs.size(); ++i) {  // ascending i: every row ends up ascending; the left end first, as the requests are
    adj[(size_t)at[(size_t)segs[i].l]++] = (int32_t)i;
    adj[(size_t)at[(size_t)segs[i].r]++] = (int32_t)i;
  }
}

}  // namespace pa
