// Players reset on the device at seeded random points of their level's walkable floor (include/rdoom.h "spawn"):
// rdoom_world_spawn_players, its world-set form, and the device copy of a level's spawn table.
//
// Arithmetic: the generator is 32-bit integers (Philox4x32-10; the two 32 x 32 -> 64 bit products of a round are a mul and a mulhi);
// the geometry is binary32, the contract's operations in the contract's order, nothing contracted, no division.  The sector at a
// point and a player's live heights are world_shared.hpp's, the definitions locate_players uses.
//
// Shape: one lane per player, one wave per workgroup.  A lane draws at most RDOOM_SPAWN_TRIES candidates -- the bound is the `for`'s
// own -- and each candidate costs one search of the cumulative areas, bounded by the level's ceil(log2(entries)) + 1, and at
// most nine descents.  No LDS, no atomics, no barriers: lanes leave the loop as they find their point.
#include <hip/hip_runtime.h>

#include <vector>

#include "../common.hpp"
#include "../host/game_world.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::descend;
using rdoom_dev::live_heights;
using rdoom_dev::sector_in_leaf;
using rdoom_dev::SectorLevel;
using rdoom_dev::SectorTables;
using rdoom_dev::SpawnArgs;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64;

struct SpawnLevel {  // a slot of SpawnDevice: its entries, the bound of the search, its start
  uint32_t first, count, steps;
  float4 start;
};

// Philox4x32-10 of counter x under key (k0, k1)
__device__ __forceinline__ uint4 philox(uint4 x, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (uint32_t round = 0; round < 10; round++) {
    const uint32_t h0 = __umulhi(0xD2511F53u, x.x), l0 = 0xD2511F53u * x.x;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, x.z), l1 = 0xCD9E8D57u * x.z;
    x = make_uint4(h1 ^ x.y ^ k0, l1, h0 ^ x.w ^ k1, l0);
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
  return x;
}
__device__ __forceinline__ float draw(uint32_t word) { return (float)(word >> 8) * 0x1p-24f; }

// (x, z) is clear for the player of `off`: in a sector with the clearance; floor: that sector's live floor
__device__ __forceinline__ bool clear_at(const SectorTables &t, const SectorLevel &lv, const float *off, uint32_t n_objects, float x, float z,
                                         float clearance, float &floor) {
  const uint32_t s = sector_in_leaf(t, lv.leaf0 + descend(t.nodes + lv.node0, x, z), x, z);
  if (s == RDOOM_SECTOR_NONE) return false;
  const float2 h = live_heights(t, lv, s, off, n_objects);
  floor = h.x;
  return h.y - h.x >= clearance;
}

// a floor `near` beside the candidate's `floor`: within the step, and not one the falling body would land on the edge of
__device__ __forceinline__ bool level_with(float near, float floor, float max_step, float landing) {
  const float rise = near - floor;
  return __builtin_fabsf(rise) <= max_step && !(rise > 0.0f && rise < landing);
}

// player p (its mask byte set) on a level of the tables
__device__ __forceinline__ void spawn(const SpawnArgs &a, uint32_t p, const SectorLevel &lv, const SpawnLevel &sp) {
  const SectorTables t{a.nodes, a.leaves, a.edges, a.sectors};
  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;
  const uint32_t episode = a.episode ? a.episode[p] : 0u;
  float x = sp.start.x, y = sp.start.y, z = sp.start.z, yaw = sp.start.w;
  uint32_t won = 0;
  if (sp.count) {
    const float *cumulative = a.cumulative + sp.first;
    const float total = cumulative[sp.count - 1];
    for (uint32_t tr = 1; tr <= RDOOM_SPAWN_TRIES; tr++) {
      const uint4 r = philox(make_uint4(p, episode, tr, 0u), a.key0, a.key1);
      const float target = draw(r.x) * total;
      uint32_t lo = 0, hi = sp.count;
      for (uint32_t step = 0; step < sp.steps && lo < hi; step++) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cumulative[mid] > target) hi = mid;
        else lo = mid + 1;
      }
      if (lo >= sp.count) lo = sp.count - 1;
      const float4 *corner = a.corners + (size_t)(sp.first + lo) * 3;
      const float4 ca = corner[0], cb = corner[1], cc = corner[2];
      float u1 = draw(r.y), u2 = draw(r.z);
      if (u1 + u2 > 1.0f) u1 = 1.0f - u1, u2 = 1.0f - u2;
      const float qx = (ca.x + u1 * (cb.x - ca.x)) + u2 * (cc.x - ca.x);
      const float qy = (ca.y + u1 * (cb.y - ca.y)) + u2 * (cc.y - ca.y);
      const float qz = (ca.z + u1 * (cb.z - ca.z)) + u2 * (cc.z - ca.z);
      float floor, near;
      const float landing = RDOOM_SPAWN_RISE - a.margin;
      if (!clear_at(t, lv, off, a.n_objects, qx, qz, a.clearance, floor)) continue;
      if (!(__builtin_fabsf(floor - qy) <= a.max_step)) continue;
      // the eight points a margin away: along x and z, then the diagonals
      const float diagonal = a.margin * 0.70710677f;
      bool around = true;
      for (uint32_t k = 0; k < 8 && around; k++) {
        const float r = k < 4 ? a.margin : diagonal;
        const float dx = (k & 1) ? -r : r, dz = k < 4 ? r : ((k & 2) ? -r : r);
        const float nx = (k < 4 && (k & 2)) ? qx : qx + dx;
        const float nz = k < 4 ? ((k & 2) ? qz + dx : qz) : qz + dz;
        around = clear_at(t, lv, off, a.n_objects, nx, nz, a.clearance, near) && level_with(near, floor, a.max_step, landing);
      }
      if (!around) continue;
      x = qx, y = floor + RDOOM_SPAWN_RISE, z = qz, yaw = draw(r.w) * 6.2831855f, won = tr;
      break;
    }
  }
  rdoom_player_state *st = a.states + p;
  st->pos[0] = x, st->pos[1] = y, st->pos[2] = z;
  st->vel[0] = 0.0f, st->vel[1] = 0.0f, st->vel[2] = 0.0f;
  st->yaw = yaw, st->pitch = 1e-8f, st->last_height_diff = 0.0f;
  st->flags = a.flags;
  if (a.tries_out) a.tries_out[p] = won;
}

__global__ __launch_bounds__(WAVE) void spawn_players_kernel(SpawnArgs a, SectorLevel lv, SpawnLevel sp) {
  const uint32_t p = blockIdx.x * WAVE + threadIdx.x;
  if (p >= a.n || (a.mask && !a.mask[p])) return;
  spawn(a, p, lv, sp);
}

__global__ __launch_bounds__(WAVE) void worldset_spawn_players_kernel(SpawnArgs a, const uint4 *__restrict__ sector_levels,
                                                                      const uint4 *__restrict__ spawn_levels,
                                                                      const float4 *__restrict__ starts,
                                                                      const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x * WAVE + threadIdx.x;
  if (p >= a.n || (a.mask && !a.mask[p])) return;
  const uint32_t slot = level_of[p];
  if (slot >= n_levels) {  // a slot outside the set: the state stays
    if (a.tries_out) a.tries_out[p] = 0u;
    return;
  }
  with_level(slot, [&](uint32_t use) __attribute__((always_inline)) {
    const uint4 r = sector_levels[use], s = spawn_levels[use];
    spawn(a, p, SectorLevel{r.x, r.y, r.z, r.w}, SpawnLevel{s.x, s.y, s.z, starts[use]});
  });
}

// ceil(log2(n)) + 1: the most steps the contract's search takes over n entries
uint32_t search_steps(uint32_t n) {
  uint32_t steps = 1;
  while (steps < 33 && (1ull << (steps - 1)) < n) steps++;
  return steps;
}

SpawnLevel level_of(const rdoom::game::World &h) {
  return SpawnLevel{0u, (uint32_t)h.spawn.size(), search_steps((uint32_t)h.spawn.size()),
                    make_float4(h.start_pos[0], h.start_pos[1], h.start_pos[2], h.start_yaw)};
}

// the arguments of a spawn, checked, as the kernel takes them.  noun: "world" or "world set"
rdoom_status spawn_args(const rdoom::MapSource &src, const char *noun, rdoom_player_state *d_states, uint32_t n, const float *d_offsets,
                        uint32_t n_objects, const uint8_t *d_mask, uint64_t seed, const uint32_t *d_episode, const rdoom_spawn_params *params,
                        uint32_t *d_tries_out, SpawnArgs &a) {
  if (!params) return rdoom::fail(RDOOM_BAD_ARG, "null params");
  if (n && !d_states) return rdoom::fail(RDOOM_BAD_ARG, "null states with n = %u", n);
  if (!(params->margin >= 0.0f)) return rdoom::fail(RDOOM_BAD_ARG, "margin %g is negative or not a number", (double)params->margin);
  if (!(params->clearance >= 0.0f)) return rdoom::fail(RDOOM_BAD_ARG, "clearance %g is negative or not a number", (double)params->clearance);
  if (!(params->max_step >= 0.0f)) return rdoom::fail(RDOOM_BAD_ARG, "max_step %g is negative or not a number", (double)params->max_step);
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  const rdoom::SectorDevice &sd = *src.sectors;
  const rdoom::SpawnDevice &pd = *src.spawn;
  a = SpawnArgs{d_states, d_offsets, d_mask, d_episode, d_tries_out, sd.nodes.get(), sd.edges.get(), sd.sectors.get(), sd.leaves.get(), pd.cumulative.get(),
                pd.corners.get(),
                n, n_objects, (uint32_t)(seed & 0xFFFFFFFFull), (uint32_t)(seed >> 32), params->margin, params->clearance, params->max_step,
                params->flags};
  return RDOOM_OK;
}

}  // namespace

namespace rdoom {

rdoom_status spawn_upload(const std::vector<const game::World *> &levels, SpawnDevice &out) {
  std::vector<float> cumulative;
  std::vector<float4> corners, starts;
  std::vector<uint4> slots;
  for (const game::World *w : levels) {
    const SpawnLevel l = level_of(*w);
    slots.push_back(make_uint4((uint32_t)cumulative.size(), l.count, l.steps, 0u));
    starts.push_back(l.start);
    for (const rdoom_spawn_entry &e : w->spawn) {
      cumulative.push_back(e.cumulative);
      for (const float *v : {e.a, e.b, e.c}) corners.push_back(make_float4(v[0], v[1], v[2], 0.0f));
    }
  }
  if (rdoom_status s = out.cumulative.upload(cumulative, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.corners.upload(corners, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.levels.upload(slots, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.starts.upload(starts, EMPTY_TABLE_BYTES)) return s;
  out.n_levels = (uint32_t)slots.size();
  if (!slots.empty()) out.level0 = slots[0], out.start0 = starts[0];
  return RDOOM_OK;
}

}  // namespace rdoom

static_assert(sizeof(rdoom_spawn_entry) == 40 && sizeof(rdoom_spawn_params) == 16 && sizeof(rdoom_spawn_table) == 32, "ABI sizes");

extern "C" {

rdoom_status rdoom_world_spawn_players(const rdoom_world *w, rdoom_player_state *d_states, uint32_t n, const float *d_object_offsets,
                                       uint32_t n_objects, const uint8_t *d_mask, uint64_t seed, const uint32_t *d_episode,
                                       const rdoom_spawn_params *params, uint32_t *d_tries_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  SpawnArgs a;
  if (rdoom_status s = spawn_args(src, "world", d_states, n, d_object_offsets, n_objects, d_mask, seed, d_episode, params, d_tries_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(spawn_players_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a,
                               SectorLevel{0u, 0u, 0u, src.max_sectors},
                               SpawnLevel{src.spawn->level0.x, src.spawn->level0.y, src.spawn->level0.z, src.spawn->start0});
}

rdoom_status rdoom_worldset_spawn_players(const rdoom_worldset *set, rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                          const float *d_object_offsets, uint32_t n_objects, const uint8_t *d_mask, uint64_t seed,
                                          const uint32_t *d_episode, const rdoom_spawn_params *params, uint32_t *d_tries_out, void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  SpawnArgs a;
  if (rdoom_status s = spawn_args(src, "world set", d_states, n, d_object_offsets, n_objects, d_mask, seed, d_episode, params, d_tries_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_spawn_players_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a,
                               (const uint4 *)src.sectors->levels.get(), (const uint4 *)src.spawn->levels.get(), (const float4 *)src.spawn->starts.get(), d_levels,
                               src.spawn->n_levels);
}

}  // extern "C"
