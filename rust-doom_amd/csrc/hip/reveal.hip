// Each player's set of seen lines, kept on the device (include/rdoom.h "seen lines"):
// rdoom_world_reveal_lines and rdoom_worldset_reveal_lines.  The maps drawn through the set are automap.hip's.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off and HIP divides
// correctly rounded, so an IEEE host evaluating the header's expressions gets the same bits (tests/reveal_restatement.c does).
//
// Shape: one 256-thread workgroup per player, so the state, the yaw, the level slot and the row of offsets are the workgroup's.
// The fan is taken 256 rays at a time; a pass over that many rays has two phases.
// Phase 1, T_r = the nearest blocking hit of every ray: sight.hpp's sight_limits, the one pass this unit and area.hip share, over
// this kernel's LDS arrays (its list is appended to by world_shared.hpp's append, as the map kernel's is).
// Phase 2, the bits.  Threads own lines and loop over the pass's (vel, T_r) in LDS, again a broadcast read.  A wave holds 64
// consecutive lines: its ballot of "some ray sees it" is two whole words of the row, which one lane each merges with the old
// word and stores.  Lines whose bit is already set are not tested again (bits are never cleared), and what the ballot adds is
// what was clear before, so its population count is the new-line count: no atomics anywhere.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "sight.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::near_line;
using rdoom_dev::Near;
using rdoom_dev::ray_hits;
using rdoom_dev::sincos_rd;
using rdoom_dev::wave_max;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = rdoom_dev::SIGHT_THREADS, WAVES = THREADS / WAVE;

struct RevealArgs {
  const rdoom_player_state *states;
  const float *offsets;  // n x n_objects x xyz, or null
  const float *dirs;     // n_rays x (right, forward): a caller's floats, dword aligned and no more
  uint32_t *seen;        // n x stride words
  uint32_t *new_out;     // n, or null
  rdoom_dev::LineTable lines;
  uint32_t n_objects, n_rays, stride;
  float max_range;
};

// the seen lines of player p among lines [first, first + n_lines) of the table
__device__ __forceinline__ void reveal_player(const RevealArgs &a, uint32_t p, uint32_t first, uint32_t n_lines) {
  __shared__ float4 list[THREADS];  // phase 1's blocking lines: w.x, w.z, d.x, d.z
  __shared__ float4 rays[THREADS];  // the pass's rays: vel.x, vel.z, T_r
  __shared__ float part[THREADS];   // phase 1's minima, one per thread
  __shared__ float wave_reach[WAVES];
  __shared__ uint32_t wave_count[WAVES];

  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const rdoom_player_state *st = a.states + p;
  const float px = st->pos[0], pz = st->pos[2];
  float s, c;
  sincos_rd(st->yaw, s, c);
  const float fx = -s, fz = -c;  // the map's forward; its right is (c, -s)
  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;
  uint32_t *row = a.seen + (size_t)p * a.stride;
  uint32_t fresh = 0;  // the bits this wave set that were clear: wave-uniform

  for (uint32_t ray0 = 0; ray0 < a.n_rays; ray0 += THREADS) {
    const uint32_t nr = a.n_rays - ray0 < THREADS ? a.n_rays - ray0 : THREADS;
    // the pass's rays, and the longest of them: no hit lies farther from the player than that
    float len2 = 0.0f;
    if (tid < nr) {
      const float dr = a.dirs[2 * (size_t)(ray0 + tid)], df = a.dirs[2 * (size_t)(ray0 + tid) + 1];
      const float dir_x = c * dr + fx * df, dir_z = fx * dr + fz * df;
      const float vx = dir_x * a.max_range, vz = dir_z * a.max_range;
      rays[tid] = make_float4(vx, vz, 1.0f, 0.0f);
      len2 = vx * vx + vz * vz;
    }
    len2 = wave_max(len2);
    if (lane == 0) wave_reach[wave] = len2;
    __syncthreads();
    const float reach = __builtin_sqrtf(__builtin_fmaxf(__builtin_fmaxf(wave_reach[0], wave_reach[1]), __builtin_fmaxf(wave_reach[2], wave_reach[3])));
    const float player_size = (__builtin_fabsf(px) + __builtin_fabsf(pz)) + reach;

    // ---- phase 1: T_r into rays[r].z
    rdoom_dev::sight_limits(a.lines, off, a.n_objects, first, n_lines, px, pz, reach, player_size, nr, list, rays, part, wave_count);

    // ---- phase 2: a thread per line, a wave per two words of the row
    for (uint32_t base = wave * WAVE; base < n_lines; base += THREADS) {
      const uint32_t l = base + lane;
      const bool writer = (lane & 31u) == 0 && l < n_lines;  // lanes 0 and 32 own the wave's two words
      const uint32_t old = writer ? row[l >> 5] : 0u;
      const uint32_t old_lo = __builtin_amdgcn_readlane(old, 0), old_hi = __builtin_amdgcn_readlane(old, 32);
      bool test = l < n_lines && !(((lane < 32 ? old_lo : old_hi) >> (lane & 31u)) & 1u);
      Near g{};
      if (test) {
        g = near_line(a.lines.seg[first + l], px, pz, reach, player_size);
        test = g.ok;
      }
      bool sees = false;
      if (__builtin_amdgcn_ballot_w64(test))
        for (uint32_t r = 0; r < nr; r++) {
          const float4 v = rays[r];
          float t;
          const bool hit = ray_hits(g.wx, g.wz, g.dx, g.dz, v.x, v.y, t);
          sees |= test & hit & (t <= v.z);
          if (!__builtin_amdgcn_ballot_w64(test & !sees)) break;  // every line of the wave that could be seen is
        }
      const uint64_t found = __builtin_amdgcn_ballot_w64(sees);
      fresh += (uint32_t)__builtin_popcountll(found);
      const uint32_t bits = (uint32_t)(found >> (lane & 32u));
      if (writer && bits) row[l >> 5] = old | bits;
    }
    __syncthreads();  // before the next pass overwrites the rays
  }

  if (a.new_out) {
    if (lane == 0) wave_count[wave] = fresh;
    __syncthreads();
    if (tid == 0) a.new_out[p] = (wave_count[0] + wave_count[1]) + (wave_count[2] + wave_count[3]);
  }
}

__global__ __launch_bounds__(THREADS) void reveal_lines_kernel(RevealArgs a, uint32_t n_lines) { reveal_player(a, blockIdx.x, 0u, n_lines); }

// the world set's: player p looks at level level_of[p]; a slot outside the set leaves the row alone and counts 0
__global__ __launch_bounds__(THREADS) void worldset_reveal_lines_kernel(RevealArgs a, const uint2 *__restrict__ levels,
                                                                        const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x;
  const uint32_t lv = level_of[p];
  uint32_t first = 0, n_lines = 0;
  if (lv < n_levels)
    with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) { first = levels[slot].x, n_lines = levels[slot].y; });
  reveal_player(a, p, first, n_lines);
}

// the arguments of a reveal, checked, as the kernel takes them.  noun: "world" or "world set"
rdoom_status reveal_args(const rdoom::MapSource &src, const char *noun, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs,
                         uint32_t n_rays, float max_range, const float *d_offsets, uint32_t n_objects, uint32_t *d_seen, uint32_t stride,
                         uint32_t *d_new_out, RevealArgs &a) {
  if (n && (!d_states || !d_seen || !d_dirs)) return rdoom::fail(RDOOM_BAD_ARG, "null states, seen rows or directions with n = %u", n);
  if (rdoom_status s = rdoom::check_fan(n_rays, max_range)) return s;
  if (rdoom_status s = rdoom::check_seen_stride(src, noun, stride)) return s;
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u players: too many for one launch", n);
  const rdoom::MapDevice &d = *src.map;
  a = RevealArgs{d_states, d_offsets, d_dirs, d_seen, d_new_out, {d.seg.get(), d.heights.get(), d.ids.get(), d.flags.get()}, n_objects, n_rays, stride, max_range};
  return RDOOM_OK;
}

}  // namespace

extern "C" {

rdoom_status rdoom_world_reveal_lines(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs,
                                      uint32_t n_rays, float max_range, const float *d_object_offsets, uint32_t n_objects, uint32_t *d_seen,
                                      uint32_t stride, uint32_t *d_new_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  RevealArgs a;
  if (rdoom_status s = reveal_args(src, "world", d_states, n, d_dirs, n_rays, max_range, d_object_offsets, n_objects, d_seen, stride, d_new_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(reveal_lines_kernel, dim3(n), dim3(THREADS), 0, stream, a, src.map->n_lines);
}

rdoom_status rdoom_worldset_reveal_lines(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                         const float *d_dirs, uint32_t n_rays, float max_range, const float *d_object_offsets,
                                         uint32_t n_objects, uint32_t *d_seen, uint32_t stride, uint32_t *d_new_out, void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  RevealArgs a;
  if (rdoom_status s = reveal_args(src, "world set", d_states, n, d_dirs, n_rays, max_range, d_object_offsets, n_objects, d_seen, stride, d_new_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_reveal_lines_kernel, dim3(n), dim3(THREADS), 0, stream, a, (const uint2 *)src.map->levels.get(), d_levels,
                               src.map->n_levels);
}

}  // extern "C"
