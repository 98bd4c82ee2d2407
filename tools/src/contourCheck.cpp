// contourCheck -- the host line assembly of sliceMEF3d (tools/common/pa_contour.h) as a stand-alone program, so that it can be run
// under AddressSanitizer + UBSan and timed without a GPU.
//   contourCheck lines   stdin: nverts nsegs, then nsegs rows "l r" (vertex ids, 0-based)
//                        stdout: "fast <n>" and n rows "l r l r ..." (the segments of each line as the CSR walk assembles them), then
//                        "scan <n>" and the rows of the plain list scan.  Exit 3 when the two differ.
//   contourCheck time    the same input; stdout: "fast_ms <t> scan_ms <t> join_ms <t> fragments <n> lines <n>": the first phase (the
//                        walk) by the CSR and by the list scan (scan_ms -1 with a third argument "noscan"), then the join phase,
//                        which both share
#include "../common/pa_contour.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>

static bool read_segs(int& nverts, std::vector<pa::CSeg>& segs) {
  long long nv = 0, ns = 0;
  if (std::scanf("%lld %lld", &nv, &ns) != 2 || nv < 0 || ns < 0 || nv > 0x7fffffffLL || ns > 0x3fffffffLL) return false;
  nverts = (int)nv;
  segs.resize((size_t)ns);
  for (pa::CSeg& s : segs)
    if (std::scanf("%d %d", &s.l, &s.r) != 2 || s.l < 0 || s.r < 0 || s.l >= nverts || s.r >= nverts) return false;
  return true;
}

static void print(const char* tag, const pa::CLines& lines) {
  std::printf("%s %zu\n", tag, lines.size());
  for (const auto& ln : lines) {
    bool first = true;
    for (const pa::CSeg& s : ln) { std::printf(first ? "%d %d" : " %d %d", s.l, s.r); first = false; }
    std::printf("\n");
  }
}

static bool equal(const pa::CLines& a, const pa::CLines& b) {
  if (a.size() != b.size()) return false;
  auto jt = b.begin();
  for (auto it = a.begin(); it != a.end(); ++it, ++jt) {
    if (it->size() != jt->size()) return false;
    auto q = jt->begin();
    for (auto p = it->begin(); p != it->end(); ++p, ++q)
      if (p->l != q->l || p->r != q->r) return false;
  }
  return true;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode != "lines" && mode != "time") { std::fprintf(stderr, "usage: contourCheck lines | time [noscan]\n"); return 2; }
  int nverts = 0;
  std::vector<pa::CSeg> segs;
  if (!read_segs(nverts, segs)) { std::fprintf(stderr, "contourCheck: bad input\n"); return 2; }
  std::vector<int32_t> off, adj;
  if (mode == "lines") {
    pa::contour_csr(segs, nverts, off, adj);
    const pa::CLines fast = pa::contour_lines(segs, off, adj), scan = pa::contour_lines_scan(segs);
    print("fast", fast);
    print("scan", scan);
    if (!equal(fast, scan)) { std::fprintf(stderr, "contourCheck: the CSR walk and the list scan give different lines\n"); return 3; }
    return 0;
  }
  const bool noscan = argc > 2 && std::strcmp(argv[2], "noscan") == 0;
  typedef std::chrono::steady_clock clk;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t0 = clk::now();
  pa::contour_csr(segs, nverts, off, adj);
  pa::CLines fast = pa::contour_walk(segs, off, adj);  // the CSR is built on the host here: its time is part of the walk's
  const auto t1 = clk::now();
  double scan_ms = -1.0;
  if (!noscan) {
    const pa::CLines scan = pa::contour_walk_scan(segs);
    scan_ms = ms(t1, clk::now());
    if (!equal(fast, scan)) { std::fprintf(stderr, "contourCheck: the CSR walk and the list scan give different fragments\n"); return 3; }
  }
  const size_t fragments = fast.size();
  const auto t2 = clk::now();
  pa::contour_detail::join_fragments(fast);
  std::printf("fast_ms %.3f scan_ms %.3f join_ms %.3f fragments %zu lines %zu\n", ms(t0, t1), scan_ms, ms(t2, clk::now()), fragments, fast.size());
  return 0;
}
