// streamSubCheck -- the host-only pieces of streamSub3d (tools/common/pa_streamsub.h) as a stand-alone program, so that they can be
// run under AddressSanitizer + UBSan and checked without a GPU.  A refusal prints "abort <message>" and exits 0.
//   streamSubCheck outfile <infile>                      stdout: the default output name
//   streamSubCheck elements <nElts> [key=value ...]      stdout: "seed <lo> <hi>" (three and three, %.17g) or "list e ..."
//   streamSubCheck comps <n> <n file names> [names ...]  stdout: "comps c ..."
//   streamSubCheck tables <bySeed> <ncomp>               stdin: nlev, per level nbox, per box "ni nj jlo nids id ...", then nface and the
//                                                        ids.  stdout: "ok <boxes> <nodes> <points>", then "box ni nj jlo off lev b" per
//                                                        box and "node g k" per node id
#include "../common/pa_streamsub.h"

#include <cstdio>
#include <cstring>

static int refuse(const std::string& why) {
  std::printf("abort %s\n", why.c_str());
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  std::string why;
  if (mode == "outfile" && argc == 3) {
    std::printf("%s\n", pa::streamsub_default_outfile(argv[2]).c_str());
    return 0;
  }
  if (mode == "elements" && argc >= 3) {
    const long long nElts = std::atoll(argv[2]);
    pa::ParmParse pp(argc - 2, argv + 2);  // argv[2] stands where the program's name does
    pa::SubKeys K;
    pa::streamsub_read_keys(pp, K);
    bool bySeed = false;
    std::vector<int32_t> E;
    if (!pa::streamsub_element_list(K, nElts, bySeed, E, why)) return refuse(why);
    if (bySeed) {
      std::printf("seed");
      for (double v : K.seedLo) std::printf(" %.17g", v);
      for (double v : K.seedHi) std::printf(" %.17g", v);
    } else {
      std::printf("list");
      for (int32_t e : E) std::printf(" %d", e);
    }
    std::printf("\n");
    return 0;
  }
  if (mode == "comps" && argc >= 3) {
    const int n = std::atoi(argv[2]);
    if (n < 0 || 3 + n > argc) { std::fprintf(stderr, "streamSubCheck: bad input\n"); return 2; }
    const std::vector<std::string> fileNames(argv + 3, argv + 3 + n), want(argv + 3 + n, argv + argc);
    std::vector<int> comps;
    if (!pa::streamsub_components(fileNames, want, comps, why)) return refuse(why);
    std::printf("comps");
    for (int c : comps) std::printf(" %d", c);
    std::printf("\n");
    return 0;
  }
  if (mode == "tables" && argc == 4) {
    int nlev = 0;
    if (std::scanf("%d", &nlev) != 1 || nlev < 0 || nlev > 64) { std::fprintf(stderr, "streamSubCheck: bad input\n"); return 2; }
    std::vector<std::vector<pa::SubBox>> boxes((size_t)nlev);
    std::vector<std::vector<std::vector<int32_t>>> inside((size_t)nlev);
    for (int l = 0; l < nlev; ++l) {
      int nbox = 0;
      if (std::scanf("%d", &nbox) != 1 || nbox < 0 || nbox > 100000) { std::fprintf(stderr, "streamSubCheck: bad input\n"); return 2; }
      for (int b = 0; b < nbox; ++b) {
        pa::SubBox B;
        long long nids = 0;
        if (std::scanf("%lld %lld %lld %lld", &B.ni, &B.nj, &B.jlo, &nids) != 4 || B.ni < 1 || B.nj < 1 || nids < 0 || nids > 10000000) { std::fprintf(stderr, "streamSubCheck: bad input\n"); return 2; }
        std::vector<int32_t> ids((size_t)nids);
        for (int32_t& v : ids)
          if (std::scanf("%d", &v) != 1) { std::fprintf(stderr, "streamSubCheck: bad input\n"); return 2; }
        boxes[(size_t)l].push_back(B);
        inside[(size_t)l].push_back(ids);
      }
    }
    long long nface = 0;
    if (std::scanf("%lld", &nface) != 1 || nface < 0 || nface > 100000000) { std::fprintf(stderr, "streamSubCheck: bad input\n"); return 2; }
    std::vector<int32_t> face((size_t)nface);
    for (int32_t& v : face)
      if (std::scanf("%d", &v) != 1) { std::fprintf(stderr, "streamSubCheck: bad input\n"); return 2; }
    pa::SubTables T;
    if (!pa::streamsub_tables(boxes, inside, face, std::atoi(argv[2]) != 0, std::atoi(argv[3]), T, why)) return refuse(why);
    std::printf("ok %zu %lld %lld\n", T.lev_of.size(), T.num_nodes, T.npts);
    for (size_t g = 0; g < T.lev_of.size(); ++g)
      std::printf("box %lld %lld %lld %lld %d %d\n", (long long)T.box_desc[4 * g], (long long)T.box_desc[4 * g + 1], (long long)T.box_desc[4 * g + 2], (long long)T.box_desc[4 * g + 3], T.lev_of[g], T.box_of[g]);
    for (long long n = 0; n < T.num_nodes; ++n) std::printf("node %d %d\n", T.node_table[2 * (size_t)n], T.node_table[2 * (size_t)n + 1]);
    return 0;
  }
  std::fprintf(stderr, "usage: streamSubCheck outfile <infile> | elements <nElts> [key=value ...] | comps <n> <names ...> [names ...] | tables <bySeed> <ncomp>\n");
  return 2;
}
