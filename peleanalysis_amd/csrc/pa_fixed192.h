// pa_fixed192.h -- the 192-bit fixed-point arithmetic of the reproducible sums: shared by pa_stats.hip (jpdf,
// conditionalMean), pa_integral.hip (integral, rmsVel) and pa_binmef.hip (binMEF).  A sum is a two's-complement integer of three 64-bit limbs in units of 2^-s,
// s chosen from the declared magnitude M of its terms (scale_of: M < 2^k -> s = 157 - k), added with 64-bit integer atomics and
// rounded ONCE when it is read (from_fixed).  Integer addition is associative: the order of the adds drops out, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>

typedef unsigned long long u64;

struct U192 { u64 w[3]; };

__host__ __device__ __forceinline__ void u192_add(U192& a, const U192& b) {
  const u64 r0 = a.w[0] + b.w[0];
  const u64 c0 = r0 < b.w[0] ? 1ull : 0ull;
  const u64 t1 = a.w[1] + b.w[1];
  u64 c1 = t1 < b.w[1] ? 1ull : 0ull;
  const u64 r1 = t1 + c0;
  c1 += r1 < c0 ? 1ull : 0ull;
  a.w[2] = a.w[2] + b.w[2] + c1;
  a.w[1] = r1;
  a.w[0] = r0;
}
__host__ __device__ __forceinline__ u64 u64_mulhi(u64 a, u64 b) {
#ifdef __HIP_DEVICE_COMPILE__
  return __umul64hi(a, b);
#else
  return (u64)(((unsigned __int128)a * b) >> 64);
#endif
}
__host__ __device__ __forceinline__ U192 u192_mul(const U192& a, u64 n) {  // a * n mod 2^192 (two's complement: signed a, n >= 0)
  U192 r;
  r.w[0] = a.w[0] * n;
  const u64 h0 = u64_mulhi(a.w[0], n);
  const u64 l1 = a.w[1] * n;
  r.w[1] = l1 + h0;
  const u64 c = r.w[1] < h0 ? 1ull : 0ull;
  r.w[2] = a.w[2] * n + u64_mulhi(a.w[1], n) + c;
  return r;
}
__host__ __device__ __forceinline__ bool u192_zero(const U192& a) { return (a.w[0] | a.w[1] | a.w[2]) == 0; }

// t * 2^s, truncated towards zero, as a 192-bit two's-complement integer.  A term that is not finite, or that is larger than twice the
// declared magnitude, sets a flag instead (pa_*_read then fails loudly).
enum { PA_ST_OVERFLOW = 1, PA_ST_BADBIN = 2, PA_ST_NONFINITE = 4 };
__host__ __device__ __forceinline__ U192 to_fixed(double t, int s, int& flag) {
  U192 r = {{0, 0, 0}};
  long long bits;
#ifdef __HIP_DEVICE_COMPILE__
  bits = __double_as_longlong(t);
#else
  memcpy(&bits, &t, 8);
#endif
  const int ex = (int)((bits >> 52) & 0x7ff);
  u64 m = (u64)bits & ((1ull << 52) - 1);
  if (ex == 0x7ff) { flag |= PA_ST_NONFINITE; return r; }
  int E;
  if (ex == 0) { E = -1074; } else { m |= 1ull << 52; E = ex - 1075; }
  if (m == 0) return r;
  int sh = E + s;  // value = m * 2^sh
  if (sh + 53 > 158) { flag |= PA_ST_OVERFLOW; return r; }
  if (sh <= -53) return r;
  if (sh < 0) { m >>= -sh; sh = 0; }
  const int limb = sh >> 6, q = sh & 63;
  const u64 lo = m << q, hi = q ? (m >> (64 - q)) : 0ull;
  r.w[0] = limb == 0 ? lo : 0ull;
  r.w[1] = limb == 1 ? lo : (limb == 0 ? hi : 0ull);
  r.w[2] = limb == 2 ? lo : (limb == 1 ? hi : 0ull);
  if (bits < 0) {  // negate
    r.w[0] = ~r.w[0]; r.w[1] = ~r.w[1]; r.w[2] = ~r.w[2];
    const U192 one = {{1, 0, 0}};
    u192_add(r, one);
  }
  return r;
}

// the exact integer v * 2^-s rounded ONCE to double (nearest even): the top 64 significant bits + a sticky bit, then ldexp
static double from_fixed(const u64 w_in[3], int s) {
  u64 w[3] = {w_in[0], w_in[1], w_in[2]};
  const bool neg = (w[2] >> 63) != 0;
  if (neg) {
    w[0] = ~w[0]; w[1] = ~w[1]; w[2] = ~w[2];
    if (++w[0] == 0 && ++w[1] == 0) ++w[2];
  }
  int top = -1;
  for (int l = 2; l >= 0 && top < 0; --l)
    if (w[l]) top = 64 * l + 63 - __builtin_clzll(w[l]);
  if (top < 0) return 0.0;
  double v;
  if (top < 64) {
    v = (double)w[0];
    v = std::ldexp(v, -s);
  } else {
    const int drop = top - 63;  // bits below the 64 kept ones
    u64 kept = 0;
    bool sticky = false;
    for (int b = 0; b < 192; b += 64) {  // kept = (w >> drop) & (2^64 - 1)
      const int l = b >> 6;
      const int rel = b - drop;  // position of limb l's bit 0 in the shifted number
      if (rel >= 64 || rel <= -64) continue;
      kept |= rel >= 0 ? (w[l] << rel) : (w[l] >> -rel);
    }
    for (int l = 0; l < 3; ++l) {  // any dropped bit set?
      const int lo_bit = 64 * l;
      if (drop <= lo_bit) break;
      const int nb = drop - lo_bit >= 64 ? 64 : drop - lo_bit;
      const u64 mask = nb == 64 ? ~0ull : ((1ull << nb) - 1);
      if (w[l] & mask) sticky = true;
    }
    if (sticky) kept |= 1ull;
    v = std::ldexp((double)kept, drop - s);
  }
  return neg ? -v : v;
}

// limbs[0..2] += v with 64-bit integer atomics; carries travel with the add that caused them (addition mod 2^192 commutes)
__device__ __forceinline__ void u192_atomic_add(u64* p, const U192& v) {
  u64 c = 0;
  if (v.w[0]) {
    const u64 old = atomicAdd(p, v.w[0]);
    c = (old + v.w[0]) < old ? 1ull : 0ull;
  }
  const u64 a1 = v.w[1] + c;
  u64 c1 = a1 < c ? 1ull : 0ull;
  if (a1) {
    const u64 old = atomicAdd(p + 1, a1);
    c1 += (old + a1) < old ? 1ull : 0ull;
  }
  const u64 a2 = v.w[2] + c1;
  if (a2) atomicAdd(p + 2, a2);
}

static int scale_of(double M) {  // M < 2^k  ->  157 - k
  if (!(M > 0.0) || !std::isfinite(M)) return 157;
  int k;
  (void)std::frexp(M, &k);
  return 157 - k;
}

// the 64 lanes' sum of v in every lane (xor butterfly; every lane of the wavefront must be active)
__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ U192 wave_sum_u192(U192 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    U192 b;
    b.w[0] = __shfl_xor(v.w[0], o);
    b.w[1] = __shfl_xor(v.w[1], o);
    b.w[2] = __shfl_xor(v.w[2], o);
    u192_add(v, b);
  }
  return v;
}
