// fixed192_host.hip -- the HOST half of peleanalysis_amd/csrc/pa_fixed192.h as a stand-alone program (tests/test_fixed192_host.py): it makes no
// HIP API call and needs no GPU.  Records on stdin, one per line, numbers in hex:
//   S <s (decimal)> <n> <bits of n doubles>   -> "<flags> <limb0> <limb1> <limb2> <bits of from_fixed>": to_fixed of every term, u192_add, from_fixed
//   M <limb0> <limb1> <limb2> <n>             -> "<limb0> <limb1> <limb2>" of u192_mul(a, n)
//   K <bits of M>                             -> scale_of(M) (decimal)
#include "pa_fixed192.h"
#include <cstdio>
#include <vector>

int main() {
  char op;
  while (scanf(" %c", &op) == 1) {
    if (op == 'S') {
      int s;
      unsigned long n;
      if (scanf("%d %lx", &s, &n) != 2) return 2;
      U192 acc = {{0, 0, 0}};
      int flag = 0;
      for (unsigned long i = 0; i < n; ++i) {
        u64 b;
        if (scanf("%llx", &b) != 1) return 2;
        double t;
        memcpy(&t, &b, 8);
        u192_add(acc, to_fixed(t, s, flag));
      }
      const double r = from_fixed(acc.w, s);
      u64 rb;
      memcpy(&rb, &r, 8);
      printf("%x %llx %llx %llx %llx\n", flag, acc.w[0], acc.w[1], acc.w[2], rb);
    } else if (op == 'M') {
      U192 a;
      u64 n;
      if (scanf("%llx %llx %llx %llx", &a.w[0], &a.w[1], &a.w[2], &n) != 4) return 2;
      const U192 r = u192_mul(a, n);
      printf("%llx %llx %llx\n", r.w[0], r.w[1], r.w[2]);
    } else if (op == 'K') {
      u64 b;
      if (scanf("%llx", &b) != 1) return 2;
      double M;
      memcpy(&M, &b, 8);
      printf("%d\n", scale_of(M));
    } else {
      return 2;
    }
  }
  return 0;
}
