// A player's orientation on the device, shared by the player step and the ray casts (world.hip) and the player cameras
// (frames.hip): one definition, for sincos_rd.hpp's reason -- the camera computed from a state, the look direction the step
// computes from it and the rays cast from it must read the same bits, so they are built from the same quaternion.
// (api_common.cpp's host copy of these cgmath formulas takes its sines from libm sinf / cosf, where these come from sincos_rd:
// it stays separate.)
#pragma once
#include <hip/hip_runtime.h>

#include "sincos_rd.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {

struct V3 {
  float x, y, z;
};
struct Quat {
  float s, x, y, z;
};

__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 rotate(Quat q, V3 v) {  // impl Mul<Vector3> for Quaternion (cgmath)
  const V3 qv{q.x, q.y, q.z};
  const V3 c = cross(qv, v);
  const V3 tmp{c.x + v.x * q.s, c.y + v.y * q.s, c.z + v.z * q.s};
  const V3 c2 = cross(qv, tmp);
  return {c2.x * 2.0f + v.x, c2.y * 2.0f + v.y, c2.z * 2.0f + v.z};
}
__device__ __forceinline__ Quat qmul(Quat a, Quat b) {  // impl Mul for Quaternion
  return {a.s * b.s - a.x * b.x - a.y * b.y - a.z * b.z, a.s * b.x + a.x * b.s + a.y * b.z - a.z * b.y,
          a.s * b.y + a.y * b.s + a.z * b.x - a.x * b.z, a.s * b.z + a.z * b.s + a.x * b.y - a.y * b.x};
}

// Quaternion::from(Euler { x: pitch, y: yaw, z: 0 }) (api_common.cpp's cgmath formulas), sin / cos from sincos_rd
__device__ __forceinline__ Quat player_orientation(float yaw, float pitch) {
  float sx, cx, sy, cy;
  sincos_rd(pitch * 0.5f, sx, cx);
  sincos_rd(yaw * 0.5f, sy, cy);
  const float sz = 0.0f, cz = 1.0f;  // (sinf / cosf of 0 * 0.5: exact on every implementation)
  return {-sx * sy * sz + cx * cy * cz, sx * cy * cz + sy * sz * cx, -sx * sz * cy + sy * cx * cz, sx * sy * cz + sz * cx * cy};
}

// the camera eye: the displacement of player.concat(camera) (api_common.cpp player_view), the camera 0.12 above the position
__device__ __forceinline__ V3 player_eye(Quat player, V3 pos) {
  const V3 rc = rotate(player, V3{0.0f * 1.0f, 0.12f * 1.0f, 0.0f * 1.0f});
  return {rc.x + pos.x, rc.y + pos.y, rc.z + pos.z};
}

}  // namespace rdoom_dev
