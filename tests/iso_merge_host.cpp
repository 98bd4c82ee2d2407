// iso_merge_host.cpp -- stand-alone program around tools/common/pa_isomerge.h (pa::IsoMerger, the tools' host path of the
// node / element sets), for tests/test_mc_oracle.py: built plain and with the address and undefined-behaviour sanitizers.
//   iso_merge_host IN OUT
// IN : int64 dim, ncomp, nfrag; per fragment int64 nv, ne, then nv * ncomp doubles, then ne * 3 int32 (2-D: rows (id0, id1, -1))
// OUT: int64 nnodes, nelts; nnodes * ncomp doubles; nelts * dim int32
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pa_isomerge.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  int64_t head[3];
  if (!rd(in, head, sizeof head)) return 4;
  const int dim = (int)head[0], nc = (int)head[1];
  if ((dim != 2 && dim != 3) || nc < dim || head[2] < 0) return 4;
  pa::IsoMerger merger(nc, dim);
  for (int64_t f = 0; f < head[2]; ++f) {
    int64_t n[2];
    if (!rd(in, n, sizeof n) || n[0] < 0 || n[1] < 0) return 4;
    std::vector<double> v((size_t)(n[0] * nc));
    std::vector<int32_t> t((size_t)(n[1] * 3));
    if (!rd(in, v.data(), v.size() * sizeof(double)) || !rd(in, t.data(), t.size() * sizeof(int32_t))) return 4;
    for (int64_t q = 0; q < n[1]; ++q)
      for (int k = 0; k < dim; ++k)
        if (t[3 * q + k] < 0 || t[3 * q + k] >= n[0]) return 5;
    merger.add(v.data(), n[0], t.data(), n[1]);
  }
  std::fclose(in);
  merger.finish();
  const std::vector<int32_t> e = merger.elements();
  const int64_t out[2] = {(int64_t)merger.num_nodes(), (int64_t)(e.size() / dim)};
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 6;
  bool ok = std::fwrite(out, sizeof out, 1, o) == 1;
  if (!merger.nodes().empty()) ok = ok && std::fwrite(merger.nodes().data(), sizeof(double), merger.nodes().size(), o) == merger.nodes().size();
  if (!e.empty()) ok = ok && std::fwrite(e.data(), sizeof(int32_t), e.size(), o) == e.size();
  return std::fclose(o) == 0 && ok ? 0 : 7;
}
