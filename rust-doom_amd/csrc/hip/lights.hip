// The sector lights of players whose clocks are on the device (include/rdoom.h "device light set"): light_tables_kernel evaluates
// Lights::fill_buffer_at (game/src/lights.rs:26-78) for every player's own time and level, so that neither rdoom_lightset_tables nor
// rdoom_batch_render_players_clocked asks the host for a table.
//
// Arithmetic: lights.rs restated as game_level.cpp restates it, operation for operation in binary32 with -ffp-contract=off, IEEE
// division and floor; the cast to a byte is Rust's `as u8` (truncate, saturate, NaN -> 0).  One difference, documented in DESIGN
// section 15: the sine of `noise` is the binary64 sine of the binary32 argument rounded once to binary32 -- the correctly rounded
// sine but for arguments whose binary64 sine lies within its own error of a binary32 midpoint -- where the host calls libm sinf.
//
// Shape: one wave64 per player, lane l evaluates entries 4l .. 4l + 3 and stores one dword, so a row is one 256-byte store of the
// wave.  Only the player, its level slot, its clock and the level's (first, count) are wave-uniform and come through scalar loads.
// The infos do NOT: lane l needs entries 4l .., so they are per-lane vector loads of 4 x 28 bytes at a 112-byte lane stride off
// that scalar base -- not coalesced; a level's list is at most 7 KB and stays in L2.  Lanes past the count store 0 without
// loading.  Only Random entries pay the binary64 sine.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "kernels.hpp"

#pragma clang fp contract(off)

struct rdoom_lightset {
  rdoom_dev::LightSetView view{};  // its pointers are views of the two arrays below
  rdoom::DeviceArray<rdoom_light_info> d_infos;
  rdoom::DeviceArray<uint2> d_ranges;
};

namespace rdoom_dev {
namespace {

constexpr uint32_t WAVE = 64;

__device__ __forceinline__ float fract(float x) { return x - floorf(x); }  // lights.rs:66-68

// lights.rs:62-64, the sine in binary64 and rounded once
__device__ __forceinline__ float noise(float sync, float time) {
  const float arg = (sync + time / 1000.0f) * 12.9898f + sync * 78.233f;
  return fract(1.0f + (float)sin((double)arg) * 43758.547f);
}

// lights.rs:33-59
__device__ __forceinline__ float light_level_at(const rdoom_light_info &info, float time) {
  if (!info.has_effect) return info.level;
  if (info.effect_kind == 0) {  // Glow
    const float scale = info.level - info.alt_level;
    const float phase = time * info.speed / scale;
    return fabsf(0.5f - fract(phase)) * 2.0f * scale + info.alt_level;
  }
  if (info.effect_kind == 1)  // Random
    return noise(info.sync, floorf(time * info.speed)) < info.duration ? info.alt_level : info.level;
  return fract(time * info.speed + info.sync * 3.5435f) < info.duration ? info.alt_level : info.level;  // Alternate
}

// lights.rs:28 `(clamp(level) * 255.0) as u8`: clamp lets a NaN through (both comparisons fail), and Rust's cast gives 0 for it
__device__ __forceinline__ uint32_t light_byte(float level) {
  const float c = level < 0.0f ? 0.0f : (level > 1.0f ? 1.0f : level);
  const float v = c * 255.0f;
  if (!(v > 0.0f)) return 0u;  // zero, negative zero, NaN
  return v >= 255.0f ? 255u : (uint32_t)v;
}

__global__ __launch_bounds__(WAVE) void light_tables_kernel(LightTableArgs a) {
  const uint32_t p = blockIdx.x, lane = threadIdx.x;
  uint32_t slot = a.levels ? a.levels[p] : 0u;
  slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
  if (slot >= a.set.n_levels) slot = a.fallback;
  uint32_t first = 0u, count = 0u;
  if (slot < a.set.n_levels) {
    const uint2 r = a.set.ranges[slot];
    first = r.x, count = r.y;
  }
  const float time = a.times[p];
  const uint32_t e0 = lane * 4u;
  uint32_t word = 0u;
  if (e0 < count) {
    const rdoom_light_info *infos = a.set.infos + first + e0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++)
      if (e0 + k < count) word |= light_byte(light_level_at(infos[k], time)) << (8u * k);
  }
  *reinterpret_cast<uint32_t *>(a.out + (size_t)p * a.stride + e0) = word;
}

}  // namespace

const LightSetView *lightset_view(const rdoom_lightset *set) { return set ? &set->view : nullptr; }

rdoom_status launch_light_tables(hipStream_t st, const LightTableArgs &a) {
  if (a.n == 0) return RDOOM_OK;
  hipLaunchKernelGGL(light_tables_kernel, dim3(a.n), dim3(WAVE), 0, st, a);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // namespace rdoom_dev

extern "C" {

rdoom_status rdoom_lightset_create(const rdoom_light_info *const *infos, const uint32_t *counts, uint32_t n_levels,
                                   rdoom_lightset **out) {
  if (!out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  *out = nullptr;
  if (!infos || !counts || n_levels == 0) return rdoom::fail(RDOOM_BAD_ARG, "a light set needs at least one level's info list");
  return rdoom::guarded([&]() -> rdoom_status {
    std::vector<rdoom_light_info> all;
    std::vector<uint2> ranges;
    for (uint32_t l = 0; l < n_levels; l++) {
      if (counts[l] > 255u) return rdoom::fail(RDOOM_BAD_ARG, "level %u has %u light infos (at most 255)", l, counts[l]);
      if (counts[l] && !infos[l]) return rdoom::fail(RDOOM_BAD_ARG, "level %u: %u light infos at a null pointer", l, counts[l]);
      ranges.push_back(make_uint2((uint32_t)all.size(), counts[l]));
      for (uint32_t i = 0; i < counts[l]; i++) {
        const rdoom_light_info &info = infos[l][i];
        if (info.has_effect && (info.effect_kind < 0 || info.effect_kind > 2))
          return rdoom::fail(RDOOM_BAD_ARG, "level %u, light %u: effect_kind %d is not 0 (Glow), 1 (Random) or 2 (Alternate)", l, i,
                             info.effect_kind);
        all.push_back(info);
      }
    }
    auto set = std::make_unique<rdoom_lightset>();
    HIP_TRY(hipGetDevice(&set->view.device));
    // (never a zero-byte allocation: a set whose levels all have no light keeps one unused info)
    if (rdoom_status s = set->d_infos.alloc(all.size() + 1u)) return s;
    if (rdoom_status s = set->d_ranges.alloc(ranges.size())) return s;
    if (!all.empty()) HIP_TRY(hipMemcpy(set->d_infos.get(), all.data(), sizeof(rdoom_light_info) * all.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(set->d_ranges.get(), ranges.data(), sizeof(uint2) * ranges.size(), hipMemcpyHostToDevice));
    set->view.infos = set->d_infos.get();
    set->view.ranges = set->d_ranges.get();
    set->view.n_levels = n_levels;
    *out = set.release();
    return RDOOM_OK;
  });
}

void rdoom_lightset_destroy(rdoom_lightset *set) { delete set; }

rdoom_status rdoom_lightset_tables(const rdoom_lightset *set, const uint32_t *d_levels, const float *d_times, uint32_t n,
                                   uint8_t *d_out, void *stream) {
  using namespace rdoom_dev;
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null light set");
  if (n == 0) return RDOOM_OK;
  if (!d_times || !d_out) return rdoom::fail(RDOOM_BAD_ARG, "d_times or d_out is null with %u players", n);
  if (((uintptr_t)d_out & 3u) != 0u) return rdoom::fail(RDOOM_BAD_ARG, "d_out must be 4-byte aligned");
  HIP_TRY(hipSetDevice(set->view.device));
  LightTableArgs a{};
  a.set = set->view, a.levels = d_levels, a.times = d_times, a.n = n, a.out = d_out, a.stride = 256u, a.fallback = 0xFFFFFFFFu;
  return launch_light_tables((hipStream_t)stream, a);
}

}  // extern "C"
