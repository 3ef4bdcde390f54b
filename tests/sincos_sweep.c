/* The host side of the sweep over every binary32 argument of the project's sincos (tests/sincos_restatement.h; the device side is
 * rdoom_selftest_sincos, rust-doom_amd/csrc/hip/selftest.hip).  A binade is bits >> 23, sign and exponent together: 512 of them,
 * 2^23 arguments each.  Per binade: the 64-bit order-independent sum the device entry point returns (the mix is restated here from
 * include/rdoom.h's comment), the raw (s, c) pairs, and the worst error of sin and of cos against float64 sin / cos in the measure
 * of tests/test_world_host.py::test_restatement_sincos_within_two_ulp.
 * -DSINCOS_VARIANT=1 replaces the reduction's 2/pi by its neighbouring float: a function that is wrong in the last place of one
 * constant, for the tests to show that the sums notice.
 * Built by the tests like the restatements (tests/sincos_ref.py): gcc -O2 -ffp-contract=off -fno-fast-math. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(SINCOS_VARIANT) && SINCOS_VARIANT
#define SINCOS_TWO_OVER_PI 0x1.45f308p-1f /* the float above 0.636619772f = 0x1.45f306p-1f */
#endif
#include "sincos_restatement.h"

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static uint32_t canonical(float f) { return f != f ? 0x7FC00000u : to_bits(f); }

/* include/rdoom.h, rdoom_selftest_sincos */
static uint64_t term(uint32_t x, uint32_t s, uint32_t c) {
  uint64_t h = (uint64_t)x * 0x9E3779B97F4A7C15ull;
  h ^= ((uint64_t)s << 32) | c;
  h ^= h >> 32;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  h *= 0xD6E8FEB86659FD93ull;
  h ^= h >> 32;
  return h;
}

/* sums[b] for the binades b0 <= b < b1 (sums: all 512 slots) */
void ss_sums(uint32_t b0, uint32_t b1, uint64_t *sums) {
  for (uint32_t b = b0; b < b1 && b < 512u; b++) {
    uint64_t sum = 0;
    for (uint32_t m = 0; m < (1u << 23); m++) {
      uint32_t bits = (b << 23) | m;
      float s, c;
      sincos_restated(from_bits(bits), &s, &c);
      sum += term(bits, canonical(s), canonical(c));
    }
    sums[b] = sum;
  }
}

/* the (s, c) pairs of binade b's 2^23 arguments, by mantissa: 2^24 floats */
void ss_raw(uint32_t b, float *out) {
  for (uint32_t m = 0; m < (1u << 23); m++) sincos_restated(from_bits((b << 23) | m), &out[2 * (size_t)m], &out[2 * (size_t)m + 1]);
}

/* one argument at a time, for the comparison with the numpy copy: n arguments' bits in, n (s, c) pairs out */
void ss_eval(const uint32_t *bits, uint32_t n, float *out) {
  for (uint32_t i = 0; i < n; i++) sincos_restated(from_bits(bits[i]), &out[2 * (size_t)i], &out[2 * (size_t)i + 1]);
}

/* |got - want| in units of the last place of the binary32 nearest to want where want is not tiny; near a zero of the function,
 * relative to the reduction's absolute error floor (1e-12): test_restatement_sincos_within_two_ulp's measure */
static double measure(float got, double want) {
  if (fabs(want) > 1e-5) {
    float w = fabsf((float)want);
    double ulp = (double)nextafterf(w, INFINITY) - (double)w;
    return fabs((double)got - want) / ulp;
  }
  return fabs((double)got - want) / 1e-12;
}

/* binade b (a finite one) at every `stride`-th mantissa: worst[0] the worst error of sin, worst[1] of cos; at[0], at[1] the bits
 * of the first argument that attains each */
void ss_worst(uint32_t b, uint32_t stride, double *worst, uint32_t *at) {
  worst[0] = worst[1] = -1.0;
  at[0] = at[1] = b << 23;
  for (uint32_t m = 0; m < (1u << 23); m += stride) {
    uint32_t bits = (b << 23) | m;
    float x = from_bits(bits), s, c;
    sincos_restated(x, &s, &c);
    double es = measure(s, sin((double)x)), ec = measure(c, cos((double)x));
    if (es > worst[0] || es != es) worst[0] = es, at[0] = bits; /* (a NaN error takes the slot and keeps it) */
    if (ec > worst[1] || ec != ec) worst[1] = ec, at[1] = bits;
  }
}
