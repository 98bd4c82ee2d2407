// celltiles_host.hip -- the tile table and the decode of peleanalysis_amd/csrc/pa_celltiles.h as a stand-alone program
// (tests/test_celltiles_host.py): it makes no HIP API call and needs no GPU.  Records on stdin, numbers in decimal:
//   <aax> <march> <kt> <nboxes>, then per box <lo0> <lo1> <lo2> <hi0> <hi1> <hi2>
// The table is counted by celltiles_count, the function CellTileTable::build uploads from, and every (tile, thread of 256) is decoded
// the way the kernels do it.  Per record:
//   "T <ntiles> <outside> <ragged>": visits of a thread with a cell (ok) that fall outside its box, and tiles whose threads do not
//                                    agree on the box and on m0 .. m1 (k_integral's wavefront sums need the same loop bounds in every lane)
//   per box one line, a digit per valid cell (x fastest, then y, z): how often it was visited (9: nine times or more)
// With (aax, march, kt) = (1, 2, 16) the compile-time form of the statistics kernels is decoded as well and must agree (else exit 3).
#include "pa_celltiles.h"
#include <cstdio>
#include <cstring>
#include <vector>

static bool same(const CellTile& a, const CellTile& b) {
  return a.b == b.b && a.i == b.i && a.a == b.a && a.m0 == b.m0 && a.m1 == b.m1 && a.ok == b.ok && memcmp(&a.B, &b.B, sizeof(DBox)) == 0;
}

int main() {
  int aax, march, kt, nb;
  while (scanf("%d %d %d %d", &aax, &march, &kt, &nb) == 4) {
    if (nb < 1 || kt < 1 || aax < 1 || aax > 2 || march != 3 - aax) return 2;
    std::vector<DBox> boxes(nb);
    for (DBox& B : boxes)
      if (scanf("%d %d %d %d %d %d", &B.lo[0], &B.lo[1], &B.lo[2], &B.hi[0], &B.hi[1], &B.hi[2]) != 6) return 2;
    std::vector<int> cum;
    if (celltiles_count(boxes.data(), nb, aax, march, kt, cum)) return 2;
    const CellTab T = {cum.data(), nb, cum[nb]};
    const CellWalk W = {march, aax, kt};
    std::vector<std::vector<int>> seen(nb);
    for (int b = 0; b < nb; ++b) {
      const DBox& B = boxes[b];
      seen[b].assign((size_t)(B.hi[0] - B.lo[0] + 1) * (B.hi[1] - B.lo[1] + 1) * (B.hi[2] - B.lo[2] + 1), 0);
    }
    long long outside = 0, ragged = 0;
    for (int t = 0; t < T.ntiles; ++t) {
      const CellTile c0 = celltile_decode(T, W, boxes.data(), t, 0);
      bool rag = false;
      for (unsigned tid = 0; tid < 256; ++tid) {
        const CellTile c = celltile_decode(T, W, boxes.data(), t, tid);
        if (aax == 1 && march == 2 && kt == 16 && !same(c, celltile_decode(T, CellWalkFixed<1, 2, 16>(), boxes.data(), t, tid))) return 3;
        rag = rag || c.b != c0.b || c.m0 != c0.m0 || c.m1 != c0.m1;
        if (!c.ok) continue;
        for (int m = c.m0; m <= c.m1; ++m) {
          int idx[3];
          celltile_cell(W, c, m, idx);
          bool in = c.b >= 0 && c.b < nb;
          for (int d = 0; in && d < 3; ++d) in = idx[d] >= boxes[c.b].lo[d] && idx[d] <= boxes[c.b].hi[d];
          if (!in) { ++outside; continue; }
          const DBox& B = boxes[c.b];
          const size_t nx = B.hi[0] - B.lo[0] + 1, ny = B.hi[1] - B.lo[1] + 1;
          ++seen[c.b][((size_t)(idx[2] - B.lo[2]) * ny + (idx[1] - B.lo[1])) * nx + (idx[0] - B.lo[0])];
        }
      }
      ragged += rag;
    }
    printf("T %d %lld %lld\n", T.ntiles, outside, ragged);
    for (int b = 0; b < nb; ++b) {
      for (int v : seen[b]) putchar('0' + (v > 9 ? 9 : v));
      putchar('\n');
    }
  }
  return 0;
}
