// The cameras of players whose state is on the device (include/rdoom.h "player frames"): player_frames_kernel derives each
// player's rdoom_pose, u_modelview per object, and the renderer's PoseConst / ObjectConst straight from rdoom_player_state, so
// that rdoom_batch_render_players renders what the step left in device memory without a host round trip.
//
// Arithmetic: the cgmath restatement of api_common.cpp (player_view, matrix_of, rdoom_object_modelviews_from_player) and
// renderer.hip's mat_mul_v1, operation for operation in binary32 with -ffp-contract=off and IEEE division.  Two differences,
// both documented in DESIGN section 12: sine and cosine come from sincos_rd (the world step's), not libm sinf / cosf, and the
// sky angle vr0 = atan2(pm[8], pm[10]) is evaluated in binary64 and rounded once (correctly rounded, where the host path's
// glibc atan2f is not always).  The projection is a constant of the frame size, computed on the host by
// rdoom_pose_from_player itself.
//
// Shape: one lane per (pose, object) pair, wave64; lane (p, 0) also writes pose p's constants.  A few MB per render at most:
// latency-bound, one launch, nothing in scratch.
#include <hip/hip_runtime.h>

#include <cstring>

#include "kernels.hpp"
#include "player_quat.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {
namespace {

constexpr uint32_t WAVE = 64;

struct View {  // Decomposed { scale s, rot r, disp d }
  float s;
  Quat r;
  V3 d;
};

// api_common.cpp player_view: (player.concat(camera)).inverse_transform(), orientation and eye from player_quat.hpp
__device__ __forceinline__ View player_view(float px, float py, float pz, float yaw, float pitch) {
  const Quat player = player_orientation(yaw, pitch);
  const Quat identity{1.0f, 0.0f, 0.0f, 0.0f};
  const float scale = 1.0f * 1.0f;
  const Quat rot = qmul(player, identity);
  const V3 disp = player_eye(player, V3{px, py, pz});
  const float s = 1.0f / scale;
  const float vv = (rot.x * rot.x + rot.y * rot.y) + rot.z * rot.z;
  const float mag2 = rot.s * rot.s + vv;
  const Quat r{rot.s / mag2, -rot.x / mag2, -rot.y / mag2, -rot.z / mag2};
  const V3 rd = rotate(r, disp);
  return View{s, r, V3{rd.x * -s, rd.y * -s, rd.z * -s}};
}

// api_common.cpp matrix_of: Matrix4::from(Decomposed)
__device__ __forceinline__ void matrix_of(const View &v, float out[16]) {
  const Quat &r = v.r;
  const float s = v.s;
  const float x2 = r.x + r.x, y2 = r.y + r.y, z2 = r.z + r.z;
  const float xx2 = x2 * r.x, xy2 = x2 * r.y, xz2 = x2 * r.z, yy2 = y2 * r.y, yz2 = y2 * r.z, zz2 = z2 * r.z;
  const float sy2 = y2 * r.s, sz2 = z2 * r.s, sx2 = x2 * r.s;
  const float m3[9] = {1.0f - yy2 - zz2, xy2 + sz2, xz2 - sy2, xy2 - sz2, 1.0f - xx2 - zz2, yz2 + sx2, xz2 + sy2, yz2 - sx2, 1.0f - xx2 - yy2};
#pragma unroll
  for (int c = 0; c < 3; c++) {
#pragma unroll
    for (int rr = 0; rr < 3; rr++) out[c * 4 + rr] = m3[c * 3 + rr] * s;
    out[c * 4 + 3] = 0.0f;
  }
  out[12] = v.d.x, out[13] = v.d.y, out[14] = v.d.z, out[15] = 1.0f;
}

// renderer.hip mat_mul_v1 (V1): PM = P * M, plain multiply / add, left to right
__device__ __forceinline__ void mat_mul_v1(const float *P, const float *M, float *pm) {
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int r = 0; r < 4; r++)
      pm[c * 4 + r] = ((P[0 * 4 + r] * M[c * 4 + 0] + P[1 * 4 + r] * M[c * 4 + 1]) + P[2 * 4 + r] * M[c * 4 + 2]) +
                      P[3 * 4 + r] * M[c * 4 + 3];
}

// sky.vert:10-12's angle, correctly rounded: binary64 atan2 (within an ulp of binary64), rounded once to binary32
__device__ __forceinline__ float sky_angle(float y, float x) { return (float)atan2((double)y, (double)x); }

__device__ __forceinline__ void store16(float *dst, const float *m) {  // 16-byte aligned destination
  float4 *d = reinterpret_cast<float4 *>(dst);
#pragma unroll
  for (int k = 0; k < 4; k++) d[k] = make_float4(m[4 * k], m[4 * k + 1], m[4 * k + 2], m[4 * k + 3]);
}

__global__ __launch_bounds__(WAVE) void player_frames_kernel(PlayerFrameArgs a) {
  const uint32_t gid = blockIdx.x * WAVE + threadIdx.x;
  if (gid >= a.n * a.lanes) return;
  const uint32_t p = gid / a.lanes, o = gid - p * a.lanes;
  const rdoom_player_state *st = a.states + p;
  const View view = player_view(st->pos[0], st->pos[1], st->pos[2], st->yaw, st->pitch);
  float M[16];
  matrix_of(view, M);
  if (o != 0) {  // rdoom_object_modelviews_from_player: the static world / an object at rest is the view itself
    const float *off = a.offsets + ((size_t)p * a.lanes + o) * 3;
    const float ox = off[0], oy = off[1], oz = off[2];
    if (!(ox == 0.0f && oy == 0.0f && oz == 0.0f)) {
      const Quat identity{1.0f, 0.0f, 0.0f, 0.0f};
      const V3 rd = rotate(view.r, V3{ox * view.s, oy * view.s, oz * view.s});
      matrix_of(View{view.s * 1.0f, qmul(view.r, identity), V3{rd.x + view.d.x, rd.y + view.d.y, rd.z + view.d.z}}, M);
    }
  }
  if (a.modelviews_out) {
    float *dst = a.modelviews_out + ((size_t)p * a.lanes + o) * 16;
#pragma unroll
    for (int k = 0; k < 16; k++) dst[k] = M[k];
  }
  float time = a.time;  // u_time: the render's, or this player's own clock (only lane (p, 0) writes it anywhere)
  if (o == 0 && a.times) time = a.times[p];
  if (o == 0 && a.poses_out) {
    rdoom_pose *dst = a.poses_out + p;
#pragma unroll
    for (int k = 0; k < 16; k++) dst->modelview[k] = M[k], dst->projection[k] = a.proj[k];
    dst->time = time, dst->_pad = 0.0f;
  }
  if (!a.pose_consts) return;
  float pm[16];
  mat_mul_v1(a.proj, M, pm);
  const float vr0 = sky_angle(pm[8], pm[10]), vr1 = pm[9] / pm[11];
  if (a.object_consts && o < a.n_render_objects) {
    ObjectConst *oc = a.object_consts + (size_t)p * a.n_render_objects + o;
    store16(oc->pm, pm);
    store16(oc->mv, M);
    *reinterpret_cast<float4 *>(&oc->vr0) = make_float4(vr0, vr1, 0.0f, 0.0f);
  }
  if (o != 0) return;
  // lane (p, 0): PoseConst p.  A level outside the set is never used: level 0 instead, and the first such pose is recorded
  // (as ~p, atomicMax: the smallest p wins; 0 = none) in the batch's error word, which the render cleared before this launch
  uint32_t level = a.levels ? a.levels[p] : 0u;
  if (level >= a.n_slices) {
    atomicMax(a.error_word, ~p);
    level = 0u;
  }
  PoseConst *pc = a.pose_consts + p;
  store16(pc->pm, pm);
  *reinterpret_cast<float4 *>(&pc->time) = make_float4(time, vr0, vr1, a.zk);
  if (a.lights) {  // (null: the clocked render, whose light kernel writes the table after this launch)
    const uint8_t *lights = a.lights + (size_t)level * a.lights_stride;
    uint4 *ld = reinterpret_cast<uint4 *>(pc->lights);
    if (((uintptr_t)lights & 15u) == 0u) {
      const uint4 *ls = reinterpret_cast<const uint4 *>(lights);
#pragma unroll
      for (int k = 0; k < 16; k++) ld[k] = ls[k];
    } else {
      for (int k = 0; k < 256; k++) pc->lights[k] = lights[k];
    }
  }
  store16(pc->mv, M);
  store16(pc->proj, a.proj);
  *reinterpret_cast<uint4 *>(&pc->level) = make_uint4(level, 0u, 0u, 0u);
}

}  // namespace

rdoom_status launch_player_frames(hipStream_t st, const PlayerFrameArgs &a) {
  const uint64_t lanes = (uint64_t)a.n * a.lanes;
  if (lanes == 0) return RDOOM_OK;
  if (lanes > 0xFFFFFFFFull - WAVE) return rdoom::fail(RDOOM_BAD_ARG, "%u players x %u objects: too many for one launch", a.n, a.lanes);
  hipLaunchKernelGGL(player_frames_kernel, dim3((uint32_t)((lanes + WAVE - 1) / WAVE)), dim3(WAVE), 0, st, a);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

rdoom_status player_projection(uint32_t width, uint32_t height, float proj[16], float *zk) {
  rdoom_pose pose;
  const float origin[3] = {0.0f, 0.0f, 0.0f};
  if (rdoom_status rs = rdoom_pose_from_player(origin, 0.0f, 0.0f, width, height, 0.0f, &pose)) return rs;
  std::memcpy(proj, pose.projection, sizeof pose.projection);
  *zk = proj[11] != 0.0f ? proj[10] / proj[11] : 0.0f;  // renderer.hip render_impl's S5 constant
  return RDOOM_OK;
}

}  // namespace rdoom_dev

// rdoom_poses_from_players_device and its clocked form: one time for every player (d_times null), or one per player
static rdoom_status poses_from_players(const rdoom_player_state *d_states, uint32_t n, uint32_t width, uint32_t height, float time,
                                       const float *d_times, const float *d_object_offsets, uint32_t n_objects,
                                       rdoom_pose *d_poses_out, float *d_object_modelviews_out, void *stream) {
  using namespace rdoom_dev;
  if (!d_states || !d_poses_out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (n == 0 || width == 0 || height == 0) return rdoom::fail(RDOOM_BAD_ARG, "n %u, frame %ux%u: none may be 0", n, width, height);
  if (d_object_modelviews_out && (!d_object_offsets || n_objects == 0))
    return rdoom::fail(RDOOM_BAD_ARG, "object modelviews need the object offsets and n_objects >= 1");
  if (n_objects > 4096u) return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u (at most 4096)", n_objects);
  PlayerFrameArgs a{};
  if (rdoom_status rs = player_projection(width, height, a.proj, &a.zk)) return rs;
  a.states = d_states, a.n = n, a.time = time, a.times = d_times;
  a.offsets = d_object_modelviews_out ? d_object_offsets : nullptr;
  a.lanes = d_object_modelviews_out ? n_objects : 1u;
  a.poses_out = d_poses_out, a.modelviews_out = d_object_modelviews_out;
  return launch_player_frames((hipStream_t)stream, a);
}

extern "C" rdoom_status rdoom_poses_from_players_device(const rdoom_player_state *d_states, uint32_t n, uint32_t width, uint32_t height,
                                                        float time, const float *d_object_offsets, uint32_t n_objects,
                                                        rdoom_pose *d_poses_out, float *d_object_modelviews_out, void *stream) {
  return poses_from_players(d_states, n, width, height, time, nullptr, d_object_offsets, n_objects, d_poses_out,
                            d_object_modelviews_out, stream);
}

extern "C" rdoom_status rdoom_poses_from_players_device_clocked(const rdoom_player_state *d_states, uint32_t n, uint32_t width,
                                                                uint32_t height, const float *d_times, const float *d_object_offsets,
                                                                uint32_t n_objects, rdoom_pose *d_poses_out,
                                                                float *d_object_modelviews_out, void *stream) {
  if (!d_times) return rdoom::fail(RDOOM_BAD_ARG, "d_times is null");
  return poses_from_players(d_states, n, width, height, 0.0f, d_times, d_object_offsets, n_objects, d_poses_out,
                            d_object_modelviews_out, stream);
}
