// The sector under every player and every player's filled top-down map (include/rdoom.h "sectors"):
// rdoom_world_locate_players, rdoom_world_draw_sector_maps, their world-set forms, and the device copy of a level's sector table
// and of the BSP that leads to it.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off, so an IEEE host
// evaluating the header's expressions gets the same values (tests/sector_restatement.c does).  A node's constant term
// d.x * o.y - d.y * o.x depends on the node alone and is computed once, at upload, by the same two products and one difference.
//
// The sector at a point is one definition, `child_of` (a step of the descent) + `sector_in_leaf` (the void and NaN rules) in
// world_shared.hpp, which both kernels here and the spawn kernel (spawn.hip) use.  locate_players: one lane per player, `descend` from the root.
// draw_sector_maps: one 256-thread workgroup per (player, 32 x 32 pixel tile), a wave per 8 rows of it, a thread four pixels of one
// column.  The contract makes the result a function of the point alone, so a wave walks down from the root TOGETHER for as long
// as every one of its 256 pixels takes the same child: the node index is then wave-uniform, its record one scalar load, and no
// margin is needed because the test is the pixels' own comparisons.  Where the pixels part, each goes on alone from the node the
// wave reached.  A leaf's record and edges are scalar loads again when the whole wave ended in one leaf (with_level's trick).
// No LDS, no atomics; a wave's stores are runs of 32 consecutive pixels of a row.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../common.hpp"
#include "../host/game_world.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::child_of;
using rdoom_dev::descend;
using rdoom_dev::live_heights;
using rdoom_dev::sector_in_leaf;
using rdoom_dev::SectorLevel;
using rdoom_dev::SectorTables;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = 256;
constexpr uint32_t TILE = 32;                       // pixels a side
constexpr uint32_t PIXELS = TILE * TILE / THREADS;  // per thread: column lane % 32, rows 8 * wave + lane / 32 + 2 k
constexpr uint32_t WAVE_ROWS = TILE / (THREADS / WAVE), ROW_STEP = WAVE / TILE;

struct LocateArgs {
  const rdoom_player_state *states;
  const float *offsets;  // n x n_objects x xyz, or null
  uint32_t *sector_out;
  float *heights_out;   // n x (floor, ceiling), or null: a caller's floats, dword aligned and no more
  uint32_t *visited;    // n rows of stride words, or null
  uint32_t *new_out;    // or null
  SectorTables t;
  uint32_t n, n_objects, stride;
};

// player p on a level of the tables (in_set false: a slot outside the set)
__device__ __forceinline__ void locate(const LocateArgs &a, uint32_t p, const SectorLevel &lv, bool in_set) {
  uint32_t s = RDOOM_SECTOR_NONE;
  if (in_set) {
    const float qx = a.states[p].pos[0], qz = a.states[p].pos[2];
    s = sector_in_leaf(a.t, lv.leaf0 + descend(a.t.nodes + lv.node0, qx, qz), qx, qz);
  }
  a.sector_out[p] = s;
  if (a.heights_out) {
    const float2 h = live_heights(a.t, lv, s, a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr, a.n_objects);
    a.heights_out[2 * (size_t)p] = h.x, a.heights_out[2 * (size_t)p + 1] = h.y;
  }
  uint32_t fresh = 0;
  if (a.visited && s < lv.n_sectors) {  // the row is this lane's alone
    uint32_t *word = a.visited + (size_t)p * a.stride + (s >> 5);
    const uint32_t old = *word, bit = 1u << (s & 31u);
    if (!(old & bit)) *word = old | bit, fresh = 1;
  }
  if (a.new_out) a.new_out[p] = fresh;
}

__global__ __launch_bounds__(WAVE) void locate_players_kernel(LocateArgs a, SectorLevel lv) {
  const uint32_t p = blockIdx.x * WAVE + threadIdx.x;
  if (p < a.n) locate(a, p, lv, true);
}

__global__ __launch_bounds__(WAVE) void worldset_locate_players_kernel(LocateArgs a, const uint4 *__restrict__ levels,
                                                                       const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x * WAVE + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t slot = level_of[p];
  if (slot >= n_levels) return locate(a, p, SectorLevel{}, false);
  with_level(slot, [&](uint32_t use) __attribute__((always_inline)) {
    const uint4 r = levels[use];
    locate(a, p, SectorLevel{r.x, r.y, r.z, r.w}, true);
  });
}

struct SectorMapArgs {
  const rdoom_player_state *states;
  const float *offsets;     // n x n_objects x xyz, or null
  const uint32_t *visited;  // n rows of stride words, or null: every sector shows
  uint16_t *sector_out;     // each n x height x width, or null
  float *floor_out, *ceiling_out;
  SectorTables t;
  uint32_t n_objects, stride, width, height, tiles_x, tiles;  // tiles: per map
  float scale;
  uint32_t view_flags;
};

// tile `tile` of player p's planes; in_set false: all none
__device__ __forceinline__ void draw_tile(const SectorMapArgs &a, uint32_t p, uint32_t tile, const SectorLevel &lv, bool in_set) {
  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const uint32_t x0 = (tile % a.tiles_x) * TILE, y0 = (tile / a.tiles_x) * TILE;
  const uint32_t i = x0 + (lane & (TILE - 1)), row0 = y0 + wave * WAVE_ROWS + lane / TILE;
  uint32_t sector[PIXELS];
#pragma unroll
  for (uint32_t k = 0; k < PIXELS; k++) sector[k] = RDOOM_SECTOR_NONE;
  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;

  if (in_set) {
    // the pixels' points: the map contract's, by the definition the line maps use (world_shared.hpp)
    const rdoom_dev::MapFrame frame = rdoom_dev::map_frame(a.states + p, a.width, a.height, a.scale, a.view_flags);
    const float u = rdoom_dev::map_u(frame, i);
    float qx[PIXELS], qz[PIXELS];
#pragma unroll
    for (uint32_t k = 0; k < PIXELS; k++) rdoom_dev::map_to_world(frame, u, rdoom_dev::map_v(frame, row0 + ROW_STEP * k), qx[k], qz[k]);

    // together from the root while all the wave's pixels take the same child: `shared` is wave-uniform, its record a scalar load
    const float4 *nodes = a.t.nodes + lv.node0;
    int32_t at[PIXELS];
    for (uint32_t shared = 0;;) {
      const float4 node = nodes[shared];
      bool agree = true;
#pragma unroll
      for (uint32_t k = 0; k < PIXELS; k++) at[k] = child_of(node, qx[k], qz[k]);
      const int32_t first = __builtin_amdgcn_readfirstlane(at[0]);
#pragma unroll
      for (uint32_t k = 0; k < PIXELS; k++) agree = agree && at[k] == first;
      if (__builtin_amdgcn_ballot_w64(!agree) != 0 || first <= 0) break;
      shared = (uint32_t)first;
    }
    // each pixel alone from where the wave parted, the four of a thread side by side so that their loads overlap
    for (bool more = true; more;) {
      more = false;
#pragma unroll
      for (uint32_t k = 0; k < PIXELS; k++)
        if (at[k] > 0) {
          at[k] = child_of(nodes[at[k]], qx[k], qz[k]);
          more = more || at[k] > 0;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < PIXELS; k++)
      with_level(lv.leaf0 + (uint32_t)-at[k], [&](uint32_t leaf) __attribute__((always_inline)) { sector[k] = sector_in_leaf(a.t, leaf, qx[k], qz[k]); });

    if (a.visited) {  // drawn through the player's visited sectors
      const uint32_t *row = a.visited + (size_t)p * a.stride;
#pragma unroll
      for (uint32_t k = 0; k < PIXELS; k++)
        if (sector[k] != RDOOM_SECTOR_NONE && !((row[sector[k] >> 5] >> (sector[k] & 31u)) & 1u)) sector[k] = RDOOM_SECTOR_NONE;
    }
  }

  if (i >= a.width) return;
  const size_t map = (size_t)p * a.height * a.width;
#pragma unroll
  for (uint32_t k = 0; k < PIXELS; k++) {
    const uint32_t row = row0 + ROW_STEP * k;
    if (row >= a.height) continue;
    const size_t at = map + (size_t)row * a.width + i;
    if (a.sector_out) a.sector_out[at] = sector[k] >= RDOOM_SECTOR_NONE16 ? (uint16_t)RDOOM_SECTOR_NONE16 : (uint16_t)sector[k];
    if (a.floor_out || a.ceiling_out) {
      const float2 h = live_heights(a.t, lv, sector[k], off, a.n_objects);
      if (a.floor_out) a.floor_out[at] = h.x;
      if (a.ceiling_out) a.ceiling_out[at] = h.y;
    }
  }
}

__global__ __launch_bounds__(THREADS) void draw_sector_maps_kernel(SectorMapArgs a, SectorLevel lv) {
  draw_tile(a, blockIdx.x / a.tiles, blockIdx.x % a.tiles, lv, true);
}

// the world set's: player p's map shows level level_of[p]; a slot outside the set gives planes of none
__global__ __launch_bounds__(THREADS) void worldset_draw_sector_maps_kernel(SectorMapArgs a, const uint4 *__restrict__ levels,
                                                                            const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x / a.tiles;
  const uint32_t slot = level_of[p];
  SectorLevel lv{};
  if (slot < n_levels) {
    const uint4 r = levels[slot];
    lv = SectorLevel{r.x, r.y, r.z, r.w};
  }
  draw_tile(a, p, blockIdx.x % a.tiles, lv, slot < n_levels);
}

SectorTables tables(const rdoom::SectorDevice &d) { return SectorTables{d.nodes.get(), d.leaves.get(), d.edges.get(), d.sectors.get()}; }

// what both calls check of the game's offsets and of the rows of visited bits.  noun: "world" or "world set"
rdoom_status check_rows(const rdoom::MapSource &src, const char *noun, const float *d_offsets, uint32_t n_objects, const uint32_t *d_visited,
                        uint32_t stride) {
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (d_visited && stride < rdoom::visited_words(src))
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a row of the %s's %u sectors takes", stride,
                       rdoom::visited_words(src), noun, src.max_sectors);
  return RDOOM_OK;
}

rdoom_status locate_args(const rdoom::MapSource &src, const char *noun, const rdoom_player_state *d_states, uint32_t n, const float *d_offsets,
                         uint32_t n_objects, uint32_t *d_sector_out, float *d_heights_out, uint32_t *d_visited, uint32_t stride,
                         uint32_t *d_new_out, LocateArgs &a) {
  if (n && (!d_states || !d_sector_out)) return rdoom::fail(RDOOM_BAD_ARG, "null states or sector output with n = %u", n);
  if (rdoom_status s = check_rows(src, noun, d_offsets, n_objects, d_visited, stride)) return s;
  a = LocateArgs{d_states, d_offsets, d_sector_out, d_heights_out, d_visited, d_new_out, tables(*src.sectors), n, n_objects, stride};
  return RDOOM_OK;
}

// the arguments of a draw, checked, as the kernel takes them
rdoom_status map_args(const rdoom::MapSource &src, const char *noun, const rdoom_player_state *d_states, uint32_t n, const float *d_offsets,
                      uint32_t n_objects, const rdoom_map_view *view, const uint32_t *d_visited, uint32_t stride, uint16_t *d_sector_out,
                      float *d_floor_out, float *d_ceiling_out, SectorMapArgs &a) {
  if (!view) return rdoom::fail(RDOOM_BAD_ARG, "null view");
  if (n && !d_states) return rdoom::fail(RDOOM_BAD_ARG, "null states with n = %u", n);
  if (n && !d_sector_out && !d_floor_out && !d_ceiling_out) return rdoom::fail(RDOOM_BAD_ARG, "no output plane: sector, floor and ceiling are all null");
  if (rdoom_status s = rdoom::check_view(view)) return s;
  if (view->flags & ~(RDOOM_MAP_ROTATE | RDOOM_MAP_TOP_DOWN)) return rdoom::fail(RDOOM_BAD_ARG, "map flags 0x%x: a sector map takes ROTATE and TOP_DOWN", view->flags);
  if (rdoom_status s = check_rows(src, noun, d_offsets, n_objects, d_visited, stride)) return s;
  const uint32_t tiles_x = (view->width + TILE - 1) / TILE, tiles_y = (view->height + TILE - 1) / TILE;
  if ((uint64_t)n * tiles_x * tiles_y > 0x7FFFFFFFull)
    return rdoom::fail(RDOOM_BAD_ARG, "%u maps of %u x %u tiles: too many for one launch", n, tiles_x, tiles_y);
  a = SectorMapArgs{d_states, d_offsets, d_visited, d_sector_out, d_floor_out, d_ceiling_out, tables(*src.sectors), n_objects, stride,
                    view->width, view->height, tiles_x, tiles_x * tiles_y, view->scale, view->flags};
  return RDOOM_OK;
}

}  // namespace

namespace rdoom {

rdoom_status sector_upload(const std::vector<const game::World *> &levels, SectorDevice &out) {
  std::vector<float4> nodes, edges, sectors;
  std::vector<uint4> leaves, slots;
  for (const game::World *w : levels) {
    const size_t n_nodes = w->nodes.size(), n_leaves = w->leaf_sector.size();
    if (n_nodes > 0x8000 || n_leaves > 0x8001)
      return rdoom::fail(RDOOM_BAD_LEVEL, "a BSP of %zu nodes and %zu leaves (at most 32768 and 32769)", n_nodes, n_leaves);
    slots.push_back(make_uint4((uint32_t)nodes.size(), (uint32_t)leaves.size(), (uint32_t)sectors.size(), (uint32_t)w->map_sectors.size()));
    const uint32_t edge0 = (uint32_t)edges.size();
    for (const game::WorldNode &n : w->nodes) {
      for (int32_t child : {n.positive, n.negative})
        if (child > 0 ? (size_t)child >= n_nodes : (size_t)-(int64_t)child >= n_leaves)
          return rdoom::fail(RDOOM_BAD_LEVEL, "a BSP child %d outside the level's %zu nodes and %zu leaves", child, n_nodes, n_leaves);
      const float dx = n.displace[0], dy = n.displace[1];
      const float constant = dx * n.origin[1] - dy * n.origin[0];
      const uint32_t children = ((uint32_t)n.positive & 0xFFFFu) | ((uint32_t)n.negative << 16);
      float bits;
      std::memcpy(&bits, &children, sizeof bits);
      nodes.push_back(make_float4(dx, dy, constant, bits));
    }
    for (size_t k = 0; k < n_leaves; k++) {
      const uint32_t s = w->leaf_sector[k];
      const rdoom_map_leaf_edges &r = w->leaf_edges[k];
      if ((s != RDOOM_SECTOR_NONE && s >= w->map_sectors.size()) || (size_t)r.first + r.count > w->map_edges.size())
        return rdoom::fail(RDOOM_BAD_LEVEL, "leaf %zu names a sector or edges outside the level's tables", k);
      leaves.push_back(make_uint4(s, edge0 + r.first, r.count, 0u));
    }
    for (const rdoom_map_edge &e : w->map_edges) edges.push_back(make_float4(e.a[0], e.a[1], e.d[0], e.d[1]));
    for (const rdoom_map_sector &s : w->map_sectors) {
      float floor_id, ceiling_id;
      std::memcpy(&floor_id, &s.floor_id, sizeof floor_id);
      std::memcpy(&ceiling_id, &s.ceiling_id, sizeof ceiling_id);
      sectors.push_back(make_float4(s.floor, s.ceiling, floor_id, ceiling_id));
    }
  }
  if (rdoom_status s = out.nodes.upload(nodes, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.leaves.upload(leaves, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.edges.upload(edges, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.sectors.upload(sectors, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.levels.upload(slots, EMPTY_TABLE_BYTES)) return s;
  out.n_levels = (uint32_t)slots.size();
  return RDOOM_OK;
}

}  // namespace rdoom

static_assert(sizeof(rdoom_map_sector) == 28 && sizeof(rdoom_map_edge) == 16 && sizeof(rdoom_map_leaf_edges) == 8, "ABI sizes");

extern "C" {

rdoom_status rdoom_world_locate_players(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const float *d_object_offsets,
                                        uint32_t n_objects, uint32_t *d_sector_out, float *d_heights_out, uint32_t *d_visited, uint32_t stride,
                                        uint32_t *d_new_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  LocateArgs a;
  if (rdoom_status s = locate_args(src, "world", d_states, n, d_object_offsets, n_objects, d_sector_out, d_heights_out, d_visited, stride, d_new_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(locate_players_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a, SectorLevel{0u, 0u, 0u, src.max_sectors});
}

rdoom_status rdoom_worldset_locate_players(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                           const float *d_object_offsets, uint32_t n_objects, uint32_t *d_sector_out, float *d_heights_out,
                                           uint32_t *d_visited, uint32_t stride, uint32_t *d_new_out, void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  LocateArgs a;
  if (rdoom_status s = locate_args(src, "world set", d_states, n, d_object_offsets, n_objects, d_sector_out, d_heights_out, d_visited, stride, d_new_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_locate_players_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a,
                               (const uint4 *)src.sectors->levels.get(), d_levels, src.sectors->n_levels);
}

rdoom_status rdoom_world_draw_sector_maps(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const float *d_object_offsets,
                                          uint32_t n_objects, const rdoom_map_view *view, const uint32_t *d_visited, uint32_t stride,
                                          uint16_t *d_sector_out, float *d_floor_out, float *d_ceiling_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  SectorMapArgs a;
  if (rdoom_status s = map_args(src, "world", d_states, n, d_object_offsets, n_objects, view, d_visited, stride, d_sector_out, d_floor_out, d_ceiling_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(draw_sector_maps_kernel, dim3(n * a.tiles), dim3(THREADS), 0, stream, a, SectorLevel{0u, 0u, 0u, src.max_sectors});
}

rdoom_status rdoom_worldset_draw_sector_maps(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                             const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view,
                                             const uint32_t *d_visited, uint32_t stride, uint16_t *d_sector_out, float *d_floor_out,
                                             float *d_ceiling_out, void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  SectorMapArgs a;
  if (rdoom_status s = map_args(src, "world set", d_states, n, d_object_offsets, n_objects, view, d_visited, stride, d_sector_out, d_floor_out, d_ceiling_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_draw_sector_maps_kernel, dim3(n * a.tiles), dim3(THREADS), 0, stream, a,
                               (const uint4 *)src.sectors->levels.get(), d_levels, src.sectors->n_levels);
}

}  // extern "C"
