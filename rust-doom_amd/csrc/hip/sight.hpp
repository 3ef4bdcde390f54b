// The sight pass the seen lines (reveal.hip) and the explored area (area.hip) share: T_r, the
// nearest blocking hit of every ray of a pass, and what it is made of -- the contract's ray against line, the cull of the lines
// out of reach and the test of a line that blocks sight in a player's game.  One definition each, so that a cell is seen exactly
// where a line would be seen through: the contract's binary32 operations in the contract's order, contraction off.
#pragma once
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {

constexpr uint32_t SIGHT_THREADS = 256, SIGHT_WAVES = SIGHT_THREADS / WAVE_LANES;  // the workgroup of a pass
// The cull's rounding margin, relative to the magnitude of the coordinates involved: 2^-10.
constexpr float SIGHT_CULL_MARGIN = 9.765625e-4f;

struct LineTable {  // MapDevice's arrays
  const float4 *seg;
  const float4 *heights;
  const uint4 *ids;
  const uint32_t *flags;
};

// the contract's ray against line: w = a - o, d = b - a, vel; true on a hit, t the ray's parameter
__device__ __forceinline__ bool ray_hits(float wx, float wz, float dx, float dz, float vx, float vz, float &t) {
  const float den = vx * dz - vz * dx;
  t = (wx * dz - wz * dx) / den;
  const float u = (wx * vz - wz * vx) / den;
  return den != 0.0f && u >= 0.0f && u <= 1.0f && t >= 0.0f && t <= 1.0f;
}

// what a thread reads of a line for player position (px, pz): w, d, and whether a ray no longer than `reach` can hit it at all --
// a distance test, conservative under rounding, so it cannot change a minimum
struct Near {
  float wx, wz, dx, dz;
  bool ok;
};
__device__ __forceinline__ Near near_line(const float4 e, float px, float pz, float reach, float player_size) {
  const float dx = e.z - e.x, dz = e.w - e.y;
  const float len2 = dx * dx + dz * dz;
  const float size = player_size + ((__builtin_fabsf(e.x) + __builtin_fabsf(e.y)) + (__builtin_fabsf(e.z) + __builtin_fabsf(e.w)));
  const float limit = reach + size * SIGHT_CULL_MARGIN;
  return Near{e.x - px, e.y - pz, dx, dz, len2 > 0.0f && dist2(px, pz, e.x, e.y, dx, dz, 1.0f / len2) <= limit * limit};
}

// whether line l of the table blocks sight in the game of the offsets row `off`: a two-sided line does when its opening is empty
__device__ __forceinline__ bool blocks_sight(const LineTable &t, uint32_t l, const float *off, uint32_t n_objects) {
  if ((t.flags[l] & BOTH_SIDES) != BOTH_SIDES) return true;
  const float4 h = t.heights[l];
  const uint4 o = t.ids[l];
  const float ff = live_height(h.x, o.x, off, n_objects), fc = live_height(h.y, o.y, off, n_objects);
  const float bf = live_height(h.z, o.z, off, n_objects), bc = live_height(h.w, o.w, off, n_objects);
  const float lo = ff > bf ? ff : bf, hi = fc < bc ? fc : bc;
  return !(hi > lo);
}

// The sight limits of a pass of nr <= 256 rays, by the 256 threads of a player's workgroup: on return rays[r].z = T_r, the nearest
// hit of ray r (rays[r].x, .y: its vel) among the blocking lines [first, first + n_lines) of the table, 1 where there is none.
// The threads stride over the lines, 256 at a time, and append those that block this player's sight and lie within `reach` to
// `list` as (w, d).  Threads own rays and fold the minimum over the list, every lane of a wave reading the same entry; with fewer
// than 256 rays the spare threads take every k-th entry of the list for the same rays (thread (slice, ray) folds entries slice,
// slice + slices, ...; 256 % nr threads have no slice), and the partial minima meet in `part`.  The arrays are the caller's LDS:
// list and rays of 256, part of 256, counts of 4.  rays is written before the call, behind a barrier; there is one after the last
// store here.  Every barrier is reached by every thread.
__device__ __forceinline__ void sight_limits(const LineTable &t, const float *off, uint32_t n_objects, uint32_t first, uint32_t n_lines,
                                             float px, float pz, float reach, float player_size, uint32_t nr, float4 *list, float4 *rays,
                                             float *part, uint32_t *counts) {
  const uint32_t tid = threadIdx.x, lane = tid & (WAVE_LANES - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE_LANES);
  const uint32_t slices = SIGHT_THREADS / nr, ray = tid % nr, slice = tid / nr;
  const float4 mine = rays[ray];
  float nearest = 1.0f;
  for (uint32_t base = 0; base < n_lines; base += SIGHT_THREADS) {
    const uint32_t l = base + tid;
    bool keep = false;
    Near g{};
    if (l < n_lines) {
      g = near_line(t.seg[first + l], px, pz, reach, player_size);
      keep = g.ok && blocks_sight(t, first + l, off, n_objects);
    }
    const Appended a = append<SIGHT_WAVES>(keep, lane, wave, counts, 0u);
    if (keep) list[a.slot] = make_float4(g.wx, g.wz, g.dx, g.dz);  // a.slot < a.total <= 256
    __syncthreads();
    if (a.total) {
      if (slice < slices)
        for (uint32_t e = slice; e < a.total; e += slices) {
          const float4 b = list[e];
          float hit;
          if (ray_hits(b.x, b.y, b.z, b.w, mine.x, mine.y, hit)) nearest = hit < nearest ? hit : nearest;
        }
      __syncthreads();  // before the next lines overwrite the list
    }
  }
  part[tid] = nearest;
  __syncthreads();
  if (tid < nr) {
    float least = part[tid];
    for (uint32_t k = 1; k < slices; k++) {
      const float other = part[k * nr + tid];
      least = other < least ? other : least;
    }
    rays[tid].z = least;
  }
  __syncthreads();
}

}  // namespace rdoom_dev
