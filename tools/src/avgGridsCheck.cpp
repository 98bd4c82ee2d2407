// avgGridsCheck -- the output-grid builder of avgPlotfiles3d (tools/common/pa_avggrids.h) as a stand-alone program, for tests
// that build it with and without -fsanitize=address,undefined (tests/test_avgplt_ref.py).  No GPU, no library.
//   stdin:  max_grid_size nlists, then per list: n and n rows "lo0 lo1 lo2 hi0 hi1 hi2"
//   stdout: "same <0|1>", "<nboxes>", then the boxes, one row each
#include <cstdio>

#include "../common/pa_avggrids.h"

struct Box { int lo[3], hi[3]; };

int main() {
  int mgs = 0, nlists = 0;
  if (std::scanf("%d %d", &mgs, &nlists) != 2 || mgs < 1 || nlists < 1) { std::fprintf(stderr, "avgGridsCheck: bad header\n"); return 2; }
  std::vector<std::vector<Box>> lists((size_t)nlists);
  for (auto& l : lists) {
    int n = 0;
    if (std::scanf("%d", &n) != 1 || n < 0) { std::fprintf(stderr, "avgGridsCheck: bad list\n"); return 2; }
    l.resize((size_t)n);
    for (Box& b : l)
      if (std::scanf("%d %d %d %d %d %d", &b.lo[0], &b.lo[1], &b.lo[2], &b.hi[0], &b.hi[1], &b.hi[2]) != 6) { std::fprintf(stderr, "avgGridsCheck: bad box\n"); return 2; }
  }
  bool same = false;
  const std::vector<Box> out = pa::avg_level_grids(lists, mgs, &same);
  std::printf("same %d\n%zu\n", same ? 1 : 0, out.size());
  for (const Box& b : out) std::printf("%d %d %d %d %d %d\n", b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2]);
  return 0;
}
