// Each player's set of seen lines, kept on the device (include/rdoom.h "seen lines"):
// rdoom_world_reveal_lines and rdoom_worldset_reveal_lines.  The maps drawn through the set are automap.hip's.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off and HIP divides
// correctly rounded, so an IEEE host evaluating the header's expressions gets the same bits (tests/reveal_restatement.c does).
//
// Shape: one 256-thread workgroup per player, so the state, the yaw, the level slot and the row of offsets are the workgroup's.
// The fan is taken 256 rays at a time; a pass over that many rays has two phases.
// Phase 1, T_r = the nearest blocking hit of every ray.  The threads stride over the level's lines, 256 at a time, and append
// those that block this player's sight and lie within reach -- a distance test, conservative under rounding (CULL_MARGIN) -- to
// a list in LDS as (w, d), by wave ballot as the map kernel appends its own.  Threads own rays and fold the minimum over the
// list, every lane of a wave reading the same entry; with fewer than 256 rays the spare threads take every k-th entry of the
// list for the same rays, and the partial minima meet in LDS.
// Phase 2, the bits.  Threads own lines and loop over the pass's (vel, T_r) in LDS, again a broadcast read.  A wave holds 64
// consecutive lines: its ballot of "some ray sees it" is two whole words of the row, which one lane each merges with the old
// word and stores.  Lines whose bit is already set are not tested again (bits are never cleared), and what the ballot adds is
// what was clear before, so its population count is the new-line count: no atomics anywhere.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::BOTH_SIDES;
using rdoom_dev::dist2;
using rdoom_dev::live_height;
using rdoom_dev::sincos_rd;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = 256, WAVES = THREADS / WAVE;
// The cull's rounding margin, relative to the magnitude of the coordinates involved: 2^-10.
constexpr float CULL_MARGIN = 9.765625e-4f;

struct RevealArgs {
  const rdoom_player_state *states;
  const float *offsets;  // n x n_objects x xyz, or null
  const float *dirs;     // n_rays x (right, forward): a caller's floats, dword aligned and no more
  uint32_t *seen;        // n x stride words
  uint32_t *new_out;     // n, or null
  const float4 *seg;
  const float4 *heights;
  const uint4 *ids;
  const uint32_t *flags;
  uint32_t n_objects, n_rays, stride;
  float max_range;
};

// the contract's ray against line: w = a - o, d = b - a, vel; true on a hit, t the ray's parameter
__device__ __forceinline__ bool ray_hits(float wx, float wz, float dx, float dz, float vx, float vz, float &t) {
  const float den = vx * dz - vz * dx;
  t = (wx * dz - wz * dx) / den;
  const float u = (wx * vz - wz * vx) / den;
  return den != 0.0f && u >= 0.0f && u <= 1.0f && t >= 0.0f && t <= 1.0f;
}

// what a thread reads of line l for player position (px, pz): w, d, and whether a ray no longer than `reach` can hit it at all
struct Near {
  float wx, wz, dx, dz;
  bool ok;
};
__device__ __forceinline__ Near near_line(const float4 e, float px, float pz, float reach, float player_size) {
  const float dx = e.z - e.x, dz = e.w - e.y;
  const float len2 = dx * dx + dz * dz;
  const float size = player_size + ((__builtin_fabsf(e.x) + __builtin_fabsf(e.y)) + (__builtin_fabsf(e.z) + __builtin_fabsf(e.w)));
  const float limit = reach + size * CULL_MARGIN;
  return Near{e.x - px, e.y - pz, dx, dz, len2 > 0.0f && dist2(px, pz, e.x, e.y, dx, dz, 1.0f / len2) <= limit * limit};
}

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
#pragma unroll
    for (uint32_t o = WAVE / 2; o; o >>= 1) len2 = __builtin_fmaxf(len2, __shfl_xor(len2, o));
    if (lane == 0) wave_reach[wave] = len2;
    __syncthreads();
    const float reach = __builtin_sqrtf(__builtin_fmaxf(__builtin_fmaxf(wave_reach[0], wave_reach[1]), __builtin_fmaxf(wave_reach[2], wave_reach[3])));
    const float player_size = (__builtin_fabsf(px) + __builtin_fabsf(pz)) + reach;

    // ---- phase 1: thread (slice, ray) folds entries slice, slice + slices, ... of the list into its ray's minimum
    const uint32_t slices = THREADS / nr, ray = tid % nr, slice = tid / nr;
    const float4 mine = rays[ray];
    float nearest = 1.0f;
    for (uint32_t base = 0; base < n_lines; base += THREADS) {
      const uint32_t l = base + tid;
      bool keep = false;
      Near g{};
      if (l < n_lines) {
        g = near_line(a.seg[first + l], px, pz, reach, player_size);
        keep = g.ok;
        if (keep && (a.flags[first + l] & BOTH_SIDES) == BOTH_SIDES) {  // two-sided: it blocks when its opening is empty
          const float4 h = a.heights[first + l];
          const uint4 o = a.ids[first + l];
          const float ff = live_height(h.x, o.x, off, a.n_objects), fc = live_height(h.y, o.y, off, a.n_objects);
          const float bf = live_height(h.z, o.z, off, a.n_objects), bc = live_height(h.w, o.w, off, a.n_objects);
          const float lo = ff > bf ? ff : bf, hi = fc < bc ? fc : bc;
          keep = !(hi > lo);
        }
      }
      const uint64_t kept = __builtin_amdgcn_ballot_w64(keep);
      const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(kept >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)kept, 0u));
      if (lane == 0) wave_count[wave] = (uint32_t)__builtin_popcountll(kept);
      __syncthreads();
      uint32_t at = 0, total = 0;
#pragma unroll
      for (uint32_t w = 0; w < WAVES; w++) {
        const uint32_t n = wave_count[w];
        at += w < wave ? n : 0u;
        total += n;
      }
      if (keep) list[at + before] = make_float4(g.wx, g.wz, g.dx, g.dz);  // at + before < total <= THREADS
      __syncthreads();
      if (total) {
        if (slice < slices)
          for (uint32_t e = slice; e < total; e += slices) {
            const float4 b = list[e];
            float t;
            if (ray_hits(b.x, b.y, b.z, b.w, mine.x, mine.y, t)) nearest = t < nearest ? t : nearest;
          }
        __syncthreads();  // before the next lines overwrite the list
      }
    }
    part[tid] = nearest;
    __syncthreads();
    if (tid < nr) {
      float t = part[tid];
      for (uint32_t k = 1; k < slices; k++) {
        const float other = part[k * nr + tid];
        t = other < t ? other : t;
      }
      rays[tid].z = t;
    }
    __syncthreads();

    // ---- phase 2: a thread per line, a wave per two words of the row
    for (uint32_t base = wave * WAVE; base < n_lines; base += THREADS) {
      const uint32_t l = base + lane;
      const bool writer = (lane & 31u) == 0 && l < n_lines;  // lanes 0 and 32 own the wave's two words
      const uint32_t old = writer ? row[l >> 5] : 0u;
      const uint32_t old_lo = __builtin_amdgcn_readlane(old, 0), old_hi = __builtin_amdgcn_readlane(old, 32);
      bool test = l < n_lines && !(((lane < 32 ? old_lo : old_hi) >> (lane & 31u)) & 1u);
      Near g{};
      if (test) {
        g = near_line(a.seg[first + l], px, pz, reach, player_size);
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
  if (!n_rays) return rdoom::fail(RDOOM_BAD_ARG, "n_rays is 0");
  if (!(max_range > 0.0f) || max_range == __builtin_inff())
    return rdoom::fail(RDOOM_BAD_ARG, "max_range %g is not a finite positive number", (double)max_range);
  if (rdoom_status s = rdoom::check_seen_stride(src, noun, stride)) return s;
  if (d_offsets && n_objects < src.game_objects)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u is smaller than the %s's %u objects", n_objects, noun, src.game_objects);
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u players: too many for one launch", n);
  const rdoom::MapDevice &d = *src.map;
  a = RevealArgs{d_states, d_offsets, d_dirs, d_seen, d_new_out, d.seg, d.heights, d.ids, d.flags, n_objects, n_rays, stride,
                 max_range};
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
  return rdoom::launch_checked(worldset_reveal_lines_kernel, dim3(n), dim3(THREADS), 0, stream, a, (const uint2 *)src.map->levels, d_levels,
                               src.map->n_levels);
}

}  // extern "C"
