// flattenPlanCheck -- the host side of flattenAMRFile3d (tools/common/pa_flatten_plan.h: slab planner, rectangle builder, offset
// table, streaming writer) as a stand-alone program, for tests that build it with and without -fsanitize=address,undefined
// (tests/test_flatten_ref.py).  No GPU: the library is linked for pa_mf_layout alone.
//   flattenPlanCheck rects   stdin: slab_boxes, nfile + rows "lo0 lo1 lo2 hi0 hi1 hi2", nout + rows
//                            stdout: per slab "slab b0 b1 nrect nfileboxes" and its rectangles "fbox obox lo0 lo1 lo2 hi0 hi1 hi2" (obox: global)
//   flattenPlanCheck write <dir>   stdin: nx ny nz max_grid_size ncomp seed
//                            writes <dir>/ref with pa::write_plotfile and <dir>/s0 .. s3 with the streaming writer in several orders of
//                            slabs and component batches; checks the offset table against a sequential writer (write_fab) and the
//                            trees byte for byte; stdout: "ok <nboxes> <bytes of Cell_D>"
#include <cstdio>
#include <sstream>

#include "../common/pa_flatten_plan.h"

namespace {

bool read_boxes(std::vector<pa::Box3>& v) {
  int n = 0;
  if (std::scanf("%d", &n) != 1 || n < 0) return false;
  v.resize((size_t)n);
  for (pa::Box3& b : v)
    if (std::scanf("%d %d %d %d %d %d", &b.lo[0], &b.lo[1], &b.lo[2], &b.hi[0], &b.hi[1], &b.hi[2]) != 6) return false;
  return true;
}

std::string slurp(const std::string& f) {
  std::ifstream in(f, std::ios::binary);
  if (!in) { std::fprintf(stderr, "flattenPlanCheck: cannot read %s\n", f.c_str()); std::exit(3); }
  std::stringstream s;
  s << in.rdbuf();
  return s.str();
}

int do_rects() {
  int slab_boxes = 0;
  std::vector<pa::Box3> file, out;
  if (std::scanf("%d", &slab_boxes) != 1 || !read_boxes(file) || !read_boxes(out)) { std::fprintf(stderr, "flattenPlanCheck: bad input\n"); return 2; }
  for (const auto& s : pa::flat_slabs((int)out.size(), slab_boxes)) {
    const std::vector<pa::Box3> slab(out.begin() + s.first, out.begin() + s.second);
    std::vector<long long> covered;
    const std::vector<pa::FlatRect> rects = pa::flat_rects(file, slab, nullptr, &covered);
    const std::vector<int> ids = pa::flat_file_boxes(file, slab);
    long long sum = 0, csum = 0;
    for (const pa::FlatRect& r : rects) sum += r.numPts();
    for (long long c : covered) csum += c;
    if (sum != csum) { std::fprintf(stderr, "flattenPlanCheck: covered counts do not add up\n"); return 3; }
    std::printf("slab %d %d %zu %zu\n", s.first, s.second, rects.size(), ids.size());
    for (const pa::FlatRect& r : rects) std::printf("%d %d %d %d %d %d %d %d\n", r.fbox, r.obox + s.first, r.lo[0], r.lo[1], r.lo[2], r.hi[0], r.hi[1], r.hi[2]);
  }
  return 0;
}

int do_write(const std::string& dir) {
  int n[3], mgs = 0, ncomp = 0;
  unsigned long long seed = 0;
  if (std::scanf("%d %d %d %d %d %llu", &n[0], &n[1], &n[2], &mgs, &ncomp, &seed) != 6 || mgs < 1 || ncomp < 1) { std::fprintf(stderr, "flattenPlanCheck: bad input\n"); return 2; }
  const pa::Box3 dom{{0, 0, 0}, {n[0] - 1, n[1] - 1, n[2] - 1}};
  const std::vector<pa::Box3> boxes = pa::max_size({dom}, mgs);
  const int nb = (int)boxes.size();
  std::vector<std::string> names;
  for (int c = 0; c < ncomp; ++c) names.push_back("var" + std::to_string(c));
  const double plo[3] = {0.0, -1.0, 0.25}, phi[3] = {1.0, 1.0, 0.75}, time = 0.375;
  std::vector<pa::HostMF> mf(1);
  mf[0].define(boxes, ncomp, 0);
  unsigned long long x = seed * 2862933555777941757ull + 3037000493ull;
  for (int b = 0; b < nb; ++b)
    for (int c = 0; c < ncomp; ++c) {
      double* p = mf[0].ptr(b, c, boxes[(size_t)b].lo[0], boxes[(size_t)b].lo[1], boxes[(size_t)b].lo[2]);
      for (long long i = 0; i < boxes[(size_t)b].numPts(); ++i) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        p[i] = (double)(long long)(x >> 20) * 0x1p-40 - 4096.0;
      }
    }
  *mf[0].ptr(0, 0, 0, 0, 0) = -0.0;
  ::mkdir(dir.c_str(), 0755);
  pa::write_plotfile(dir + "/ref", names, {dom}, plo, phi, mf, time, {0});

  // the offset table against a sequential writer
  const pa::FlatOffsets offs(boxes, ncomp);
  {
    std::ostringstream os;
    long long pos = 0;
    for (int b = 0; b < nb; ++b) {
      if (offs.fab[(size_t)b] != pos) { std::fprintf(stderr, "flattenPlanCheck: FAB %d at %lld, a sequential writer puts it at %lld\n", b, offs.fab[(size_t)b], pos); return 3; }
      std::vector<double> fab((size_t)ncomp * (size_t)boxes[(size_t)b].numPts());
      for (int c = 0; c < ncomp; ++c) {
        std::memcpy(fab.data() + (size_t)c * (size_t)boxes[(size_t)b].numPts(), mf[0].ptr(b, c, boxes[(size_t)b].lo[0], boxes[(size_t)b].lo[1], boxes[(size_t)b].lo[2]), 8 * (size_t)boxes[(size_t)b].numPts());
        if (offs.block((size_t)b, c, boxes[(size_t)b].numPts()) != pos + (long long)offs.hdr[(size_t)b].size() + 8LL * c * boxes[(size_t)b].numPts()) { std::fprintf(stderr, "flattenPlanCheck: block offset\n"); return 3; }
      }
      pos += pa::write_fab(os, boxes[(size_t)b], ncomp, fab.data());
    }
    if (pos != offs.total || os.str() != slurp(dir + "/ref/Level_0/Cell_D_00000")) { std::fprintf(stderr, "flattenPlanCheck: the sequential writer's file differs from write_plotfile's\n"); return 3; }
  }

  // the streaming writer: (slab_boxes, comp_batch, slabs reversed, batches reversed)
  const int orders[4][4] = {{nb, ncomp, 0, 0}, {1, 1, 0, 0}, {3, 2, 1, 0}, {2, 1, 1, 1}};
  for (int o = 0; o < 4; ++o) {
    const std::string out = dir + "/s" + std::to_string(o);
    pa::FlatWriter W(out, names, dom, plo, phi, boxes, time);
    W.open();
    std::vector<std::pair<int, int>> slabs = pa::flat_slabs(nb, orders[o][0]);
    {  // slabs partition the boxes in order
      int at = 0;
      for (const auto& s : slabs) {
        if (s.first != at || s.second <= s.first || s.second - s.first > std::max(1, orders[o][0])) { std::fprintf(stderr, "flattenPlanCheck: slabs do not partition the boxes\n"); return 3; }
        at = s.second;
      }
      if (at != nb) { std::fprintf(stderr, "flattenPlanCheck: slabs do not cover the boxes\n"); return 3; }
    }
    if (orders[o][2]) std::reverse(slabs.begin(), slabs.end());
    std::vector<int> batches;
    for (int c = 0; c < ncomp; c += orders[o][1]) batches.push_back(c);
    if (orders[o][3]) std::reverse(batches.begin(), batches.end());
    for (int c0 : batches) {
      const int nc = std::min(orders[o][1], ncomp - c0);
      for (const auto& s : slabs) {
        pa::HostMF h;
        h.define(std::vector<pa::Box3>(boxes.begin() + s.first, boxes.begin() + s.second), nc, 0);
        for (int b = s.first; b < s.second; ++b)
          for (int a = 0; a < nc; ++a)
            std::memcpy(h.ptr(b - s.first, a, boxes[(size_t)b].lo[0], boxes[(size_t)b].lo[1], boxes[(size_t)b].lo[2]),
                        mf[0].ptr(b, c0 + a, boxes[(size_t)b].lo[0], boxes[(size_t)b].lo[1], boxes[(size_t)b].lo[2]), 8 * (size_t)boxes[(size_t)b].numPts());
        W.put_slab(s.first, c0, nc, h);
      }
    }
    W.finish();
    for (const char* f : {"/Header", "/Level_0/Cell_H", "/Level_0/Cell_D_00000"})
      if (slurp(out + f) != slurp(dir + "/ref" + f)) { std::fprintf(stderr, "flattenPlanCheck: order %d: %s differs from write_plotfile's\n", o, f); return 3; }
  }
  std::printf("ok %d %lld\n", nb, offs.total);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "rects") return do_rects();
  if (mode == "write" && argc > 2) return do_write(argv[2]);
  std::fprintf(stderr, "usage: flattenPlanCheck rects | write <dir>\n");
  return 2;
}
