/* Test-side restatement of the project's binary32 sine and cosine (the product's is rust-doom_amd/csrc/hip/sincos_rd.hpp), the one
 * definition every C restatement includes: Cody-Waite reduction by pi/2 in three parts, then the Cephes sinf / cosf polynomials
 * on [-pi/4, pi/4], written out operation by operation.  Build with -ffp-contract=off -fno-fast-math, as the restatements are.
 *
 * Domain (tests/test_sincos_host.py, tests/test_gpu_sincos.py, tests/golden/sincos_error.json): the bits are the device's for
 * every one of the 2^32 arguments; the results are within 2 of the project's ulp measure for |x| < 512, degrade from there
 * (the curve is recorded to 16384 and described to 8192); beyond 8192 no accuracy is promised -- only reproducible bits.
 *
 * The quadrant is floor(x * 2/pi + 1/2) mod 4, taken through the conversion gfx950 has (v_cvt_i32_f32): it saturates at INT_MIN
 * and INT_MAX and gives 0 for a NaN.  (int)turns is undefined in C from |turns| >= 2^31 on and for inf and NaN -- x86 gives
 * INT_MIN there -- so the three cases are written out and the cast is reached in range only. */
#ifndef SINCOS_RESTATEMENT_H
#define SINCOS_RESTATEMENT_H
#include <limits.h>
#include <math.h>

#ifndef SINCOS_TWO_OVER_PI
#define SINCOS_TWO_OVER_PI 0.636619772f /* = 0x1.45f306p-1f */
#endif

static inline int sincos_quadrant(float turns) {
  int whole;
  if (turns != turns) whole = 0;
  else if (turns >= 2147483648.0f) whole = INT_MAX;
  else if (turns <= -2147483648.0f) whole = INT_MIN;
  else whole = (int)turns;
  return whole & 3;
}

static inline void sincos_restated(float x, float *sn, float *cs) {
  float turns = floorf(x * SINCOS_TWO_OVER_PI + 0.5f);
  float rem = x - turns * 1.5703125f;
  rem = rem - turns * 4.837512969970703125e-4f;
  rem = rem - turns * 7.54978995489188216e-8f;
  float sq = rem * rem;
  float sine = -1.9515295891e-4f * sq + 8.3321608736e-3f;
  sine = sine * sq - 1.6666654611e-1f;
  sine = sine * sq * rem + rem;
  float cosine = 2.443315711809948e-5f * sq - 1.388731625493765e-3f;
  cosine = cosine * sq + 4.166664568298827e-2f;
  cosine = cosine * sq * sq - 0.5f * sq + 1.0f;
  switch (sincos_quadrant(turns)) {
    case 0: *sn = sine, *cs = cosine; break;
    case 1: *sn = cosine, *cs = -sine; break;
    case 2: *sn = -sine, *cs = -cosine; break;
    default: *sn = -cosine, *cs = sine; break;
  }
}
#endif
