// The project's own binary32 sine and cosine, shared by the player step (world.hip) and the player cameras (frames.hip): one
// definition, so that a camera computed from a state and the look direction the step computes from it read the same bits.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace rdoom_dev {

// Project-owned binary32 sine and cosine: Cody-Waite reduction by pi/2 in three parts (the first two short enough that
// j * part is exact for |j| < 2^12), then the minimax polynomials of the Cephes library's sinf / cosf on [-pi/4, pi/4].
// Every operation is written out, so an IEEE host evaluating the same expressions gets the same bits.
//
// The domain, as rdoom_selftest_sincos (selftest.hip) and tests/sincos_sweep.c establish it over all 2^32 arguments:
//   bits      reproducible for every finite argument, given the one thing that is not IEEE arithmetic here -- (int)j, which is
//             this target's v_cvt_i32_f32: saturated at INT_MIN / INT_MAX (|x| >= ~3.4e9), 0 for a NaN.  A host restatement
//             has to write that out (tests/sincos_restatement.h does); inf and NaN give NaNs;
//   accuracy  within 2 of the project's ulp measure (error in ulps of the result; near a zero of the function, over 1e-12
//             absolute) for |x| < 512: the worst of all those arguments is 1.562 (sin) and 1.527 (cos);
//   beyond    the reduction degrades: 2.95 below 1024, 5.68 below 2048, 12.3 below 4096, 25.2 below 8192
//             (tests/golden/sincos_error.json holds the record per binade, with the arguments).  Past 8192 no accuracy is
//             promised -- j * part is no longer exact -- and past 2^23 or so the results are unrelated to the sine.
// The step never wraps yaw (world.hip: yaw -= look.x), so a caller that lets it grow is inside this statement, not outside it.
__device__ __forceinline__ void sincos_rd(float x, float &s, float &c) {
  const float j = __builtin_floorf(x * 0.636619772f + 0.5f);
  const float r = ((x - j * 1.5703125f) - j * 4.837512969970703125e-4f) - j * 7.54978995489188216e-8f;
  const float z = r * r;
  const float ps = ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * r + r;
  const float pc = ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z - 0.5f * z + 1.0f;
  const int q = (int)j & 3;
  s = q == 0 ? ps : (q == 1 ? pc : (q == 2 ? -ps : -pc));
  c = q == 0 ? pc : (q == 1 ? -ps : (q == 2 ? -pc : ps));
}

}  // namespace rdoom_dev
