// streamsub_host -- the subsetting of streamSub3d on ONE host thread, written from its definition with the containers the reference uses
// (a std::set of needed boxes per level, a std::map for the new numbers): the yardstick beside tools/streamsub_bench.py.
//   streamsub_host nboxes lines points ncomp nelts frac reps
// Synthetic directory of the bench's shape: `nboxes` boxes of `lines` lines with `points` points (j = 0 in the middle), node ids in
// storage order, element e on nodes e/2, e/2+1, e/2+2, the seed x of a line of box g in [g, g+1) / nboxes; the seed box keeps x <= frac.
// Prints: select_ms plan_ms copy_ms (best of `reps` each) kept_elements kept_boxes kept_points
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

int main(int argc, char** argv) {
  if (argc != 8) { std::fprintf(stderr, "usage: streamsub_host nboxes lines points ncomp nelts frac reps\n"); return 2; }
  const long long nb = std::atoll(argv[1]), ni = std::atoll(argv[2]), nj = std::atoll(argv[3]), ncomp = std::atoll(argv[4]), nElts = std::atoll(argv[5]);
  const double frac = std::atof(argv[6]);
  const int reps = std::atoi(argv[7]), npe = 3;
  if (nb < 1 || ni < 1 || nj < 1 || ncomp < 3 || nElts < 1 || reps < 1) return 2;
  const long long N = nb * ni, np = ni * nj, j0 = nj / 2;
  std::vector<double> data((size_t)(nb * ncomp * np));
  uint64_t s = 88172645463325252ULL;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
  for (double& v : data) v = rnd();
  for (long long g = 0; g < nb; ++g)
    for (long long i = 0; i < ni; ++i) data[(size_t)(g * ncomp * np + j0 * ni + i)] = ((double)g + rnd()) / (double)nb;
  std::vector<int> face((size_t)(nElts * npe));
  for (long long e = 0; e < nElts; ++e)
    for (int k = 0; k < npe; ++k) face[(size_t)(e * npe + k)] = (int)((e / 2 + k) % N) + 1;
  const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {frac, 1.0, 1.0};
  typedef std::chrono::steady_clock clk;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  double best[3] = {1e300, 1e300, 1e300};
  long long keptE = 0, keptB = 0, keptP = 0;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = clk::now();
    std::vector<int> E;
    for (long long e = 0; e < nElts; ++e) {
      bool keep = true;
      for (int k = 0; k < npe; ++k) {
        const long long n = face[(size_t)(e * npe + k)] - 1, g = n / ni, i = n % ni;
        for (int d = 0; d < 3; ++d) {
          const double x = data[(size_t)(g * ncomp * np + d * np + j0 * ni + i)];
          if (!(lo[d] <= x && x <= hi[d])) keep = false;
        }
      }
      if (keep) E.push_back((int)e);
    }
    const auto t1 = clk::now();
    std::vector<int> faceSel(E.size() * npe);
    for (size_t j = 0; j < E.size(); ++j)
      for (int k = 0; k < npe; ++k) faceSel[j * npe + k] = face[(size_t)E[j] * npe + k];
    std::set<int> needed;
    for (int v : faceSel) needed.insert((int)((v - 1) / ni));
    std::map<int, int> newNum;
    int cnt = 1;
    for (int g : needed)
      for (long long i = 0; i < ni; ++i) newNum[(int)(g * ni + i) + 1] = cnt++;
    for (int& v : faceSel) v = newNum[v];
    const auto t2 = clk::now();
    std::vector<double> out((size_t)((long long)needed.size() * ncomp * np));
    size_t at = 0;
    for (int g : needed) {
      std::memcpy(out.data() + at, data.data() + (size_t)(g * ncomp * np), sizeof(double) * (size_t)(ncomp * np));
      at += (size_t)(ncomp * np);
    }
    const auto t3 = clk::now();
    if (ms(t0, t1) < best[0]) best[0] = ms(t0, t1);
    if (ms(t1, t2) < best[1]) best[1] = ms(t1, t2);
    if (ms(t2, t3) < best[2]) best[2] = ms(t2, t3);
    keptE = (long long)E.size();
    keptB = (long long)needed.size();
    keptP = keptB * np;
    if (out[out.size() / 2] < -1.0 || faceSel.empty()) std::printf("#\n");  // the results are used
  }
  std::printf("%.3f %.3f %.3f %lld %lld %lld\n", best[0], best[1], best[2], keptE, keptB, keptP);
  return 0;
}
