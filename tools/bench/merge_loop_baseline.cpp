// merge_loop_baseline.cpp -- the host baseline of tools/surfjoin_bench.py: the all-pairs, first-match node search that a merge without
// a grid amounts to (what mergeMEF.cpp:186-208 computes), written as tests/surfjoin_ref.py writes it.  Serial, one core.  Never the
// code under test: the device paths are timed against it and their node ids compared with its.
//   merge_loop_baseline <base.bin> <added.bin> <eps> <reps> <ids.bin>
// base.bin / added.bin: int64 n, then the x, y and z columns as doubles.  Prints one time in ms per repeat; writes, as int32, the id of
// every added point in the joined set (the first base point within eps, or the next free id) from the last repeat.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Cloud {
  int64_t n = 0;
  std::vector<double> x, y, z;
};

static Cloud read_cloud(const char* file) {
  Cloud c;
  FILE* f = std::fopen(file, "rb");
  if (!f || std::fread(&c.n, 8, 1, f) != 1 || c.n < 0) { std::fprintf(stderr, "cannot read %s\n", file); std::exit(1); }
  for (std::vector<double>* col : {&c.x, &c.y, &c.z}) {
    col->resize((size_t)c.n);
    if (std::fread(col->data(), 8, (size_t)c.n, f) != (size_t)c.n) { std::fprintf(stderr, "truncated %s\n", file); std::exit(1); }
  }
  std::fclose(f);
  return c;
}

// the smallest index of a base point whose squared distance to p, summed x first, is at most e2; -1 if there is none
static int64_t first_within(const Cloud& base, double px, double py, double pz, double e2) {
  for (int64_t j = 0; j < base.n; ++j) {
    const double ax = px - base.x[(size_t)j], ay = py - base.y[(size_t)j], az = pz - base.z[(size_t)j];
    if (((ax * ax) + ay * ay) + az * az <= e2) return j;
  }
  return -1;
}

int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const Cloud base = read_cloud(argv[1]), added = read_cloud(argv[2]);
  const double eps = std::atof(argv[3]);
  const int reps = std::atoi(argv[4]);
  const double e2 = eps * eps;
  std::vector<int32_t> ids((size_t)added.n);
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    int64_t fresh = 0;
    for (int64_t i = 0; i < added.n; ++i) {
      const int64_t hit = first_within(base, added.x[(size_t)i], added.y[(size_t)i], added.z[(size_t)i], e2);
      ids[(size_t)i] = (int32_t)(hit >= 0 ? hit : base.n + fresh++);
    }
    std::printf("%.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    std::fflush(stdout);
  }
  FILE* f = std::fopen(argv[5], "wb");
  if (!f || std::fwrite(ids.data(), 4, ids.size(), f) != ids.size()) return 1;
  std::fclose(f);
  return 0;
}
