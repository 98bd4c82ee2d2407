// streamsel_host.cpp -- the host baseline of tools/streamsel_bench.py: the node loop of streamScatter.cpp:119-155 (the peak of the
// conditioning component scanned from the middle of the line, the range test, the gather of the variables of the kept lines) on one
// thread, over synthetic Str boxes in the library's layout (component-major, line fastest, then j), uniform values in [0, 1).
//   streamsel_host <nboxes> <lines per box> <points per line> <nvars> <moreThan> <lessThan> <reps>
// prints: ms per pass (the best of reps), kept lines, a checksum
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  const long long nb = std::atoll(argv[1]), ni = std::atoll(argv[2]), nj = std::atoll(argv[3]);
  const int nv = std::atoi(argv[4]), reps = std::atoi(argv[7]);
  const double more = std::atof(argv[5]), less = std::atof(argv[6]);
  const int ncomp = 1 + nv, lo = -(int)(nj / 2), hi = lo + (int)nj - 1;
  std::vector<double> data((size_t)(nb * ncomp * ni * nj));
  uint64_t s = 88172645463325252ULL;
  for (auto& v : data) {  // xorshift64, 53 bits
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    v = (double)(s >> 11) * (1.0 / 9007199254740992.0);
  }
  std::vector<double> out((size_t)(nb * ni * (nv > 0 ? nv : 1)));
  double best = 1e300, sum = 0;
  long long kept = 0;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    kept = 0;
    for (long long b = 0; b < nb; ++b) {
      const double* fab = data.data() + (size_t)(b * ncomp * ni * nj);
      for (long long pt = 0; pt < ni; ++pt) {
        int ptOnStr = (int)(0.5 * (lo + hi));
        double hiVal = fab[(size_t)((ptOnStr - lo) * ni + pt)];
        for (int j = lo; j <= hi; ++j) {
          const double val = fab[(size_t)((j - lo) * ni + pt)];
          if (val > hiVal) {
            hiVal = val;
            ptOnStr = j;
          }
        }
        if ((hiVal >= more) && (hiVal < less)) {
          for (int c = 0; c < nv; ++c) out[(size_t)(kept * nv + c)] = fab[(size_t)(((1 + c) * nj + (ptOnStr - lo)) * ni + pt)];
          ++kept;
        }
      }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (ms < best) best = ms;
  }
  for (long long q = 0; q < kept * nv; ++q) sum += out[(size_t)q];
  std::printf("%.4f %lld %.17g\n", best, kept, sum);
  return 0;
}
