// Walking distance to a goal over a whole level (include/rdoom.h "goal distance"): the level's sector, floor and
// ceiling planes on its explored-area grid (rdoom_world_draw_area_planes), the cell of that grid a player stands in
// (rdoom_world_area_cells), and their world-set forms.  The flood of those planes, rdoom_flood_grids, is flood.hip's.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off.  The grid formulas
// are world_shared.hpp's, the ones area.hip indexes with; the sector at a point is `descend` + `sector_in_leaf` and the heights are
// `live_heights`, the ones sectors.hip uses.
//
// draw_area_planes: one thread per cell, 256 to a workgroup, no LDS.  area_cells: one lane per player.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::AreaCellArgs;
using rdoom_dev::AreaPlaneArgs;
using rdoom_dev::descend;
using rdoom_dev::Grid;
using rdoom_dev::grid_of;
using rdoom_dev::live_heights;
using rdoom_dev::point_cell;
using rdoom_dev::sector_in_leaf;
using rdoom_dev::SectorLevel;
using rdoom_dev::SectorTables;

constexpr uint32_t WAVE = 64;

// ---- the planes of a level on its grid ----
constexpr uint32_t PLANE_THREADS = 256;

// cell `i` of row p's planes; in_set false: none
__device__ __forceinline__ void plane_cell(const AreaPlaneArgs &a, uint32_t p, uint32_t i, float4 bounds, const SectorLevel &lv, bool in_set) {
  if (i >= a.width * a.height) return;
  const SectorTables t{a.nodes, a.leaves, a.edges, a.sectors};
  uint32_t s = RDOOM_SECTOR_NONE;
  if (in_set) {
    const uint32_t iz = i / a.width, ix = i - iz * a.width;
    Grid g;
    grid_of(bounds, a.cell, g);
    bool show = ix < g.gw && iz < g.gh;
    if (show && a.area) {  // drawn through the player's explored area: free and not a wall
      const uint32_t *free_row = a.area + (size_t)p * 2 * a.stride;
      const uint32_t at = iz * g.pitch + (ix >> 5);  // < the level's words <= stride
      show = ((free_row[at] & ~free_row[a.stride + at]) >> (ix & 31u)) & 1u;
    }
    if (show) {
      const float x = ((float)(g.ix0 + (int32_t)ix) + 0.5f) * a.cell, z = ((float)(g.iz0 + (int32_t)iz) + 0.5f) * a.cell;
      s = sector_in_leaf(t, lv.leaf0 + descend(a.nodes + lv.node0, x, z), x, z);
    }
  }
  const size_t at = (size_t)p * a.width * a.height + i;
  if (a.sector_out) a.sector_out[at] = s >= RDOOM_SECTOR_NONE16 ? (uint16_t)RDOOM_SECTOR_NONE16 : (uint16_t)s;
  if (a.floor_out || a.ceiling_out) {
    const float2 h = live_heights(t, lv, s, a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr, a.n_objects);
    if (a.floor_out) a.floor_out[at] = h.x;
    if (a.ceiling_out) a.ceiling_out[at] = h.y;
  }
}

__global__ __launch_bounds__(PLANE_THREADS) void draw_area_planes_kernel(AreaPlaneArgs a, float4 bounds, SectorLevel lv) {
  plane_cell(a, blockIdx.x / a.blocks, (blockIdx.x % a.blocks) * PLANE_THREADS + threadIdx.x, bounds, lv, true);
}

// the world set's: row p shows level level_of[p]; a slot outside the set gives planes of none
__global__ __launch_bounds__(PLANE_THREADS) void worldset_draw_area_planes_kernel(AreaPlaneArgs a, const float4 *__restrict__ bounds,
                                                                                  const uint4 *__restrict__ levels,
                                                                                  const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x / a.blocks;
  const uint32_t slot = level_of[p];
  const bool in_set = slot < n_levels;
  SectorLevel lv{};
  float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (in_set) {
    const uint4 r = levels[slot];
    lv = SectorLevel{r.x, r.y, r.z, r.w};
    b = bounds[slot];
  }
  plane_cell(a, p, (blockIdx.x % a.blocks) * PLANE_THREADS + threadIdx.x, b, lv, in_set);
}

// ---- the cell a player is in ----
__device__ __forceinline__ void player_cell(const AreaCellArgs &a, uint32_t p, float4 bounds, bool in_set) {
  int32_t cx = -1, cz = -1;
  if (in_set) {
    Grid g;
    grid_of(bounds, a.cell, g);
    uint32_t ix, iz;
    if (point_cell(g, a.cell, a.states[p].pos[0], a.states[p].pos[2], ix, iz)) cx = (int32_t)ix, cz = (int32_t)iz;
  }
  a.cells_out[2 * (size_t)p] = cx, a.cells_out[2 * (size_t)p + 1] = cz;
}

__global__ __launch_bounds__(WAVE) void area_cells_kernel(AreaCellArgs a, float4 bounds) {
  const uint32_t p = blockIdx.x * WAVE + threadIdx.x;
  if (p < a.n) player_cell(a, p, bounds, true);
}

__global__ __launch_bounds__(WAVE) void worldset_area_cells_kernel(AreaCellArgs a, const float4 *__restrict__ bounds,
                                                                   const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x * WAVE + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t slot = level_of[p];
  const bool in_set = slot < n_levels;
  player_cell(a, p, in_set ? bounds[slot] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), in_set);
}

// ---- the host's side ----
// the arguments of a draw, checked, as the kernel takes them.  noun: "world" or "world set"
rdoom_status plane_args(const rdoom::MapSource &src, const rdoom_world *w, const rdoom_worldset *set, const char *noun, uint32_t n,
                        const float *d_offsets, uint32_t n_objects, float cell, uint32_t width, uint32_t height, const uint32_t *d_area,
                        uint32_t stride, uint16_t *d_sector_out, float *d_floor_out, float *d_ceiling_out, AreaPlaneArgs &a) {
  if (n && !d_sector_out && !d_floor_out && !d_ceiling_out) return rdoom::fail(RDOOM_BAD_ARG, "no output plane: sector, floor and ceiling are all null");
  rdoom_area_grid most;
  if (rdoom_status s = rdoom::handle_grid(w, set, src.n_levels, cell, most)) return s;
  if (width < most.gw || height < most.gh || width > RDOOM_AREA_MAX_SIDE || height > RDOOM_AREA_MAX_SIDE)
    return rdoom::fail(RDOOM_BAD_ARG, "planes of %u x %u cells: the %s's grid at cell %g takes %u x %u, a side is at most %u", width, height, noun,
                       (double)cell, most.gw, most.gh, RDOOM_AREA_MAX_SIDE);
  const uint32_t blocks = (width * height + PLANE_THREADS - 1) / PLANE_THREADS;
  if ((uint64_t)n * blocks > 0x7FFFFFFFull)
    return rdoom::fail(RDOOM_BAD_ARG, "%u rows of %u x %u cells: too many for one launch", n, width, height);
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (d_area && stride < most.words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a plane of the %s's grid takes at cell %g", stride, most.words,
                       noun, (double)cell);
  const rdoom::SectorDevice &d = *src.sectors;
  a = AreaPlaneArgs{d_offsets, d_area, d_sector_out, d_floor_out, d_ceiling_out, d.nodes.get(), d.edges.get(), d.sectors.get(), d.leaves.get(), n_objects, stride,
                    width, height, blocks, cell};
  return RDOOM_OK;
}

rdoom_status cell_args(const rdoom::MapSource &src, const rdoom_world *w, const rdoom_worldset *set, const rdoom_player_state *d_states,
                       uint32_t n, float cell, int32_t *d_cells_out, AreaCellArgs &a) {
  if (n && (!d_states || !d_cells_out)) return rdoom::fail(RDOOM_BAD_ARG, "null states or cell output with n = %u", n);
  rdoom_area_grid most;
  if (rdoom_status s = rdoom::handle_grid(w, set, src.n_levels, cell, most)) return s;
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u players: too many for one launch", n);
  a = AreaCellArgs{d_states, d_cells_out, n, cell};
  return RDOOM_OK;
}

}  // namespace

extern "C" {

rdoom_status rdoom_world_draw_area_planes(const rdoom_world *w, uint32_t n, const float *d_object_offsets, uint32_t n_objects, float cell,
                                          uint32_t width, uint32_t height, const uint32_t *d_area, uint32_t area_stride,
                                          uint16_t *d_sector_out, float *d_floor_out, float *d_ceiling_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  AreaPlaneArgs a;
  if (rdoom_status s = plane_args(src, w, nullptr, "world", n, d_object_offsets, n_objects, cell, width, height, d_area, area_stride, d_sector_out,
                                  d_floor_out, d_ceiling_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(draw_area_planes_kernel, dim3(n * a.blocks), dim3(PLANE_THREADS), 0, stream, a, src.bounds[0],
                               SectorLevel{0u, 0u, 0u, src.max_sectors});
}

rdoom_status rdoom_worldset_draw_area_planes(const rdoom_worldset *set, const uint32_t *d_levels, uint32_t n, const float *d_object_offsets,
                                             uint32_t n_objects, float cell, uint32_t width, uint32_t height, const uint32_t *d_area,
                                             uint32_t area_stride, uint16_t *d_sector_out, float *d_floor_out, float *d_ceiling_out,
                                             void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  AreaPlaneArgs a;
  if (rdoom_status s = plane_args(src, nullptr, set, "world set", n, d_object_offsets, n_objects, cell, width, height, d_area, area_stride,
                                  d_sector_out, d_floor_out, d_ceiling_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_draw_area_planes_kernel, dim3(n * a.blocks), dim3(PLANE_THREADS), 0, stream, a,
                               (const float4 *)src.map->bounds.get(), (const uint4 *)src.sectors->levels.get(), d_levels, src.n_levels);
}

rdoom_status rdoom_world_area_cells(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, float cell, int32_t *d_cells_out,
                                    void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  AreaCellArgs a;
  if (rdoom_status s = cell_args(src, w, nullptr, d_states, n, cell, d_cells_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(area_cells_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a, src.bounds[0]);
}

rdoom_status rdoom_worldset_area_cells(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                       float cell, int32_t *d_cells_out, void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  AreaCellArgs a;
  if (rdoom_status s = cell_args(src, nullptr, set, d_states, n, cell, d_cells_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_area_cells_kernel, dim3((n + WAVE - 1) / WAVE), dim3(WAVE), 0, stream, a,
                               (const float4 *)src.map->bounds.get(), d_levels, src.n_levels);
}

}  // extern "C"
