// What the CTC prefix beam searches (beam.hip, ctc_beam_lm.hip) share: fp64 log-sum-exp of two and three terms, the
// order-preserving key of a total, and the prefix hash.
#pragma once
#include "common.h"
#include <math.h>

constexpr double DNEG = -INFINITY;

__device__ __forceinline__ double lse2d(double a, double b) {
  const double m = fmax(a, b);
  if (m == DNEG) return DNEG;
  return m + log(exp(a - m) + exp(b - m));
}
__device__ __forceinline__ double lse3d(double a, double b, double c) {
  const double m = fmax(fmax(a, b), c);
  if (m == DNEG) return DNEG;
  return m + log(exp(a - m) + exp(b - m) + exp(c - m));
}
// order-preserving map double -> uint64 (ascending), and its inverse
__device__ __forceinline__ unsigned long long okey(double x) {
  unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double unokey(unsigned long long k) {
  const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}
// hash of a prefix from its parent's and the appended label
__device__ __forceinline__ unsigned long long hmix(unsigned long long h, int c) {
  unsigned long long x = h * 0x9E3779B97F4A7C15ull + (unsigned long long)(c + 1);
  x ^= x >> 32; x *= 0xD6E8FEB86659FD93ull; x ^= x >> 29;
  return x;
}
