// binmef_host -- the rounds of pa_surfbin_add_surface on the HOST, without a device: the same round loop (sb_rounds), the same code
// for one path of the recursion (sb_chain is __host__ __device__) and the same slice rule (pa_binmef_slice); only the three steps that
// the library launches as kernels (SbDeviceOps) are written out here as loops over the items -- the body of k_sb_init is the one
// piece that exists twice, and has to be kept in step by hand.  Writes every
// (key, area) the kernels would add -- key < ntab: a bin, ntab: outside the condition, ntab + 1: an element's area -- and prints the
// rounds, the peak list occupancy and the sliced rounds.  tests/test_binmef_ref.py builds it, compares its leaves with
// tests/binmef_ref.py and runs it under the sanitizers; profiles/r09_binmef.txt section 2 is its output.
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off tools/bench/binmef_host.hip -o binmef_host
//   binmef_host <in> <out>    in: 8 int64 (nnodes nelts nc cond_apply cond_sgn work_items 0 0), 16 doubles (binMin[4] binMax[4]
//                             nBins[4] condVal areaEps 0 0), the node components [3 + nc (+ 1)][nnodes], the elements [nelts][3] int32
#include "../../peleanalysis_amd/csrc/pa_binmef.hip"
#include <cstdio>
int pa_fail(pa_ctx*, const std::string&) { return 1; }

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 1;
  long long hdr[8];
  double dpar[16];
  if (std::fread(hdr, 8, 8, f) != 8 || std::fread(dpar, 8, 16, f) != 16) return 1;
  const long long nnodes = hdr[0], nelts = hdr[1], cap = hdr[5];
  const int nc = (int)hdr[2], cond_apply = (int)hdr[3], cond_sgn = (int)hdr[4];
  const int nv = 3 + nc + (cond_apply ? 1 : 0);
  std::vector<double> nodes((size_t)nv * nnodes);
  std::vector<int> elts((size_t)3 * nelts);
  if (std::fread(nodes.data(), 8, nodes.size(), f) != nodes.size() || std::fread(elts.data(), 4, elts.size(), f) != elts.size()) return 1;
  std::fclose(f);
  SbArgs P;
  std::memset(&P, 0, sizeof P);
  std::vector<double> edges;
  P.nc = nc; P.cond_apply = cond_apply; P.cond_sgn = cond_sgn; P.cond_val = dpar[12]; P.area_eps = dpar[13];
  P.maxiter = nc + 4;
  P.ntab = 1;
  for (int j = 0; j < nc; ++j) {
    P.nb[j] = (int)dpar[8 + j];
    P.eoff[j] = (int)edges.size();
    P.bmax[j] = dpar[4 + j];
    const std::vector<double> e = pa_binmef_edges(dpar[j], dpar[4 + j], P.nb[j]);
    edges.insert(edges.end(), e.begin(), e.end());
    P.maxiter += P.nb[j] + 3;
    P.ntab *= P.nb[j];
  }
  P.edges = edges.data();
  std::vector<SbItem> La((size_t)cap), Ta((size_t)cap);
  long long nonfinite = 0;
  int flag = 0;
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 1;
  auto put = [&](long long key, double a) { std::fwrite(&key, 8, 1, o); std::fwrite(&a, 8, 1, o); };
  struct HostOps {  // what SbDeviceOps launches, one item after the other
    const SbArgs& P;
    const std::vector<double>& nodes;
    const std::vector<int>& elts;
    long long nnodes;
    int nv;
    long long& nonfinite;
    int& flag;
    decltype(put)& put;
    int init(long long e0, long long n, SbItem* L) {  // k_sb_init
      for (long long t = 0; t < n; ++t) {
        SbItem it;
        std::memset(&it, 0, sizeof it);
        bool fin = true;
        for (int q = 0; q < 3; ++q) {
          const long long node = elts[(size_t)(3 * (e0 + t) + q)] - 1;
          for (int c = 0; c < SB_NV; ++c) {
            const int src = c < 3 + P.nc ? c : (c == SB_NV - 1 && P.cond_apply ? 3 + P.nc : -1);
            const double v = src >= 0 && src < nv ? nodes[(size_t)src * nnodes + node] : 0.0;
            fin = fin && std::isfinite(v);
            it.p[q].v[c] = v;
          }
        }
        if (fin) {
          for (int q = 0; q < 3; ++q) sb_getbin(P, it.p[q]);
          it.binID = 0;
          put(P.ntab + 1, sb_area(it.p[0].v, it.p[1].v, it.p[2].v));
        } else {
          it.binID = -1;
          ++nonfinite;
        }
        L[t] = it;
      }
      return 0;
    }
    int count(const SbItem* L, long long from, long long n, int* cr) {  // k_sb_count
      for (long long t = from; t < n; ++t) {
        long long key;
        double leaf;
        int fl = 0;
        cr[2 * t] = sb_chain<false>(P, L[t].p[0], L[t].p[1], L[t].p[2], L[t].binID, nullptr, 0, 0, fl, key, leaf);
        cr[2 * t + 1] = sb_rem(P, L[t]);
      }
      return 0;
    }
    int emit(SbItem* L, long long i0, long long m, const long long* off, SbItem* T, long long tot) {  // k_sb_emit
      for (long long t = 0; t < m; ++t) {
        long long key;
        double leaf;
        const SbItem& it = L[i0 + t];
        (void)sb_chain<true>(P, it.p[0], it.p[1], it.p[2], it.binID, T, off[t], tot, flag, key, leaf);
        if (key >= 0) put(key, leaf);
      }
      if (i0 > 0 && tot) std::memcpy(L + i0, T, (size_t)tot * sizeof(SbItem));
      return 0;
    }
  } ops{P, nodes, elts, nnodes, nv, nonfinite, flag, put};
  SbRounds st;
  const int rc = sb_rounds(ops, nelts, cap, La.data(), Ta.data(), st);
  if (rc == 2) {
    std::printf("STUCK n %lld children %lld rounds %lld\n", st.stuck_n, st.stuck_children, st.rounds);
    return 2;
  }
  std::fclose(o);
  std::printf("rounds %lld peak %lld sliced %lld items %lld nonfinite %lld flag %d\n", st.rounds, st.peak, st.sliced, st.items, nonfinite, flag);
  return rc;
}
