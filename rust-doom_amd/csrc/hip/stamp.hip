// A level's solid things stamped into the area planes (include/rdoom.h "solid things on the grid"):
// rdoom_world_stamp_things and rdoom_worldset_stamp_things.  The planes are goal.hip's (rdoom_world_draw_area_planes), the thing
// set is things.hip's (thingset.hpp), the grid and the cell of a point are world_shared.hpp's.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off, so an IEEE host
// evaluating the header's expressions gets the same bytes (tests/stamp_ref.py does).
//
// Shape: thingmap.hip's.  One 256-thread workgroup per (row, 64 x 16 cell tile).  A lane is a column and a wave holds one row of
// the tile at a time, rows wave + 4 k: its plane stores are runs of 64 consecutive words.  The threads stride over the level's
// things, 256 at a time; a thread reads its thing's record in two 16-byte loads, its word of the level's solid row and its word of
// the player's hidden row, and keeps a candidate when the box of its disc can meet the tile's box of cell centres, or when the
// thing's own cell is in the tile (the cull compares what the fold compares, on the nearest point of the box: rounding is
// monotone, so it needs no margin -- DESIGN section 32).  The kept things go into a list in LDS (world_shared.hpp's append) as
// (x, z, r2, live height) and a word that carries the index and the own cell, and each thread folds its four cells over the list:
// being blocked is an OR and the index a minimum, so the order of the list and where it is cut do not matter, and a list that
// would outgrow LDS is folded and emptied in between.  The vertical window needs the cell's own floor: it is evaluated in the
// fold, and the floors are loaded when the first non-empty list is folded.  A tile whose list stayed empty, stamped in place with
// no index plane, neither loads nor stores a plane word.  Plain vector stores, no atomics; every barrier is reached by every
// thread: the loops run on values every thread computes alike.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../common.hpp"
#include "kernels.hpp"
#include "thingset.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::Grid;
using rdoom_dev::grid_of;
using rdoom_dev::live_height;
using rdoom_dev::point_cell;
using rdoom_dev::StampArgs;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = 256, WAVES = THREADS / WAVE;
constexpr uint32_t TILE_X = rdoom_dev::STAMP_TILE_X, TILE_Y = rdoom_dev::STAMP_TILE_Y;
constexpr uint32_t CELLS = TILE_X * TILE_Y / THREADS;  // per thread: rows wave + 4 k of column lane
constexpr uint32_t LIST_CAP = 768;                     // things the LDS list holds: 768 x 20 bytes = 15 KiB
constexpr uint32_t INDEX_BITS = 20, INDEX_MASK = (1u << INDEX_BITS) - 1u;  // a level of a set holds at most 2^20 things
constexpr uint32_t OWN = 1u << 10;                     // above the ten bits of a cell of the tile: the thing's own cell is in the tile
constexpr uint32_t NO_THING = 0xFFFFFFFFu;
constexpr uint32_t PLUS_INF = 0x7F800000u, MINUS_INF = 0xFF800000u;
static_assert(TILE_X == WAVE && TILE_Y == WAVES * CELLS && TILE_X * TILE_Y <= OWN, "a lane is a column; a cell of the tile takes ten bits");

// row p's tile `tile` against things [first, first + n_things) of the set, whose solid bits are row `level` of a.solid, on the
// grid of `bounds`.  A slot outside the set comes here with no thing and in_set false: its words are passed through
__device__ __forceinline__ void stamp_tile(const StampArgs &a, uint32_t p, uint32_t tile, float4 bounds, uint32_t first, uint32_t n_things,
                                           uint32_t level, bool in_set) {
  __shared__ float4 list[LIST_CAP];     // x, z, r2, the live height
  __shared__ uint32_t tags[LIST_CAP];   // the index, and above it OWN | the own cell of the tile
  __shared__ uint32_t wave_kept[WAVES];

  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  Grid g;
  grid_of(bounds, a.cell, g);
  const uint32_t x0 = (tile % a.tiles_x) * TILE_X, y0 = (tile / a.tiles_x) * TILE_Y;
  const uint32_t ix = x0 + lane, row0 = y0 + wave;  // below 2^13 + 64: the sides are at most RDOOM_AREA_MAX_SIDE
  // the centres of this thread's cells, draw_area_planes' own expression
  const float xc = ((float)(g.ix0 + (int32_t)ix) + 0.5f) * a.cell;
  float zc[CELLS];
  uint32_t mine[CELLS], best[CELLS], fw[CELLS];  // the cell of the tile as a tag carries it; the lowest blocking index; the floor's word
#pragma unroll
  for (uint32_t k = 0; k < CELLS; k++) {
    zc[k] = ((float)(g.iz0 + (int32_t)(row0 + WAVES * k)) + 0.5f) * a.cell;
    mine[k] = OWN | (wave + WAVES * k) << 6 | lane;
    best[k] = NO_THING, fw[k] = 0u;
  }
  // the tile's box of cell centres: the centres of its first and last column and row, by the same expression, which grows with
  // the cell's number -- every centre of the tile lies between them
  const float xlo = ((float)(g.ix0 + (int32_t)x0) + 0.5f) * a.cell, xhi = ((float)(g.ix0 + (int32_t)(x0 + TILE_X - 1)) + 0.5f) * a.cell;
  const float zlo = ((float)(g.iz0 + (int32_t)y0) + 0.5f) * a.cell, zhi = ((float)(g.iz0 + (int32_t)(y0 + TILE_Y - 1)) + 0.5f) * a.cell;

  const size_t plane = (size_t)p * a.height * a.width;
  const bool column = ix < a.width, in_level = in_set && ix < g.gw;  // a cell of row r is the level's when r < gh as well
  const uint32_t *solid = a.solid ? a.solid + (size_t)level * a.stride : nullptr;
  const uint32_t *hidden = a.hidden ? a.hidden + (size_t)p * a.stride : nullptr;
  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;
  const uint4 *const record = reinterpret_cast<const uint4 *>(a.things + first);  // two words of 16 bytes a thing

  bool loaded = false;  // the floors of this thread's cells are in fw: the workgroup's, set when a non-empty list is folded
  uint32_t count = 0;
  for (uint32_t base = 0; base < n_things; base += THREADS) {
    const uint32_t t = base + tid;  // t < 2^20 + 256
    bool keep = false;
    float4 entry = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t tag = 0u;
    if (t < n_things) {
      const uint4 lo = record[2 * (size_t)t], hi = record[2 * (size_t)t + 1];
      const uint32_t firm = solid ? solid[t >> 5] : ~0u, gone = hidden ? hidden[t >> 5] : 0u;  // word t / 32 < ceil(T / 32) <= stride
      const bool candidate = ((firm >> (t & 31u)) & 1u) && !((gone >> (t & 31u)) & 1u);
      const float x = __uint_as_float(lo.x), z = __uint_as_float(lo.y), radius = __uint_as_float(lo.w);
      const float r = radius + a.grow;
      const float r2 = r * r;
      // the nearest point of the tile's box: on an axis the thing is beside, the difference the fold takes at the box's edge --
      // no larger than any cell's of the tile -- and 0 on an axis it is within.  "Not beyond" rather than "within": a distance
      // that is not a number keeps the thing, and so does an r * r that overflows
      const float ax = xlo - x, bx = x - xhi, az = zlo - z, bz = z - zhi;
      const float dx = ax > 0.0f ? ax : (bx > 0.0f ? bx : 0.0f), dz = az > 0.0f ? az : (bz > 0.0f ? bz : 0.0f);
      const bool reaches = !(dx * dx + dz * dz > r2);
      uint32_t cx, cz;
      const bool own = point_cell(g, a.cell, x, z, cx, cz) && cx - x0 < TILE_X && cz - y0 < TILE_Y;
      keep = candidate && (reaches || own);
      entry = make_float4(x, z, r2, live_height(__uint_as_float(lo.z), hi.x, off, a.n_objects));
      tag = t | (own ? OWN | (cz - y0) << 6 | (cx - x0) : 0u) << INDEX_BITS;
    }
    const rdoom_dev::Appended kept = rdoom_dev::append<WAVES>(keep, lane, wave, wave_kept, count);
    if (keep) list[kept.slot] = entry, tags[kept.slot] = tag;  // count <= LIST_CAP - THREADS here, so kept.slot < LIST_CAP
    count += kept.total;
    const bool fold = count > LIST_CAP - THREADS || base + THREADS >= n_things;  // the next 256 might not fit, or there are none
    __syncthreads();
    if (fold) {
      if (count && !loaded) {
        loaded = true;
#pragma unroll
        for (uint32_t k = 0; k < CELLS; k++) {
          const uint32_t row = row0 + WAVES * k;
          if (column && row < a.height) fw[k] = a.floor[plane + (size_t)row * a.width + ix];
        }
      }
      for (uint32_t e = 0; e < count; e++) {
        const float4 s = list[e];
        const uint32_t w = tags[e], i = w & INDEX_MASK, own = w >> INDEX_BITS;
        const float ex = xc - s.x;
        const float exex = ex * ex;
#pragma unroll
        for (uint32_t k = 0; k < CELLS; k++) {
          const float ez = zc[k] - s.y;
          const float dy = __uint_as_float(fw[k]) - s.w;
          const bool covers = exex + ez * ez <= s.z || own == mine[k];
          const bool blocks = covers && dy >= a.below && dy <= a.above;
          best[k] = blocks && i < best[k] ? i : best[k];
        }
      }
      count = 0;
      __syncthreads();  // before the next things overwrite the list
    }
  }

  const bool in_place = a.floor_out == a.floor;  // the host allows it only together with the ceiling's
  if (!loaded && in_place && !a.index_out) return;  // nothing kept, nothing to copy: the workgroup's, behind the last barrier
  if (!column) return;
#pragma unroll
  for (uint32_t k = 0; k < CELLS; k++) {
    const uint32_t row = row0 + WAVES * k;
    if (row >= a.height) continue;
    const size_t at = plane + (size_t)row * a.width + ix;
    const bool blocked = in_level && row < g.gh && best[k] != NO_THING;
    if (a.floor_out) {
      if (blocked) a.floor_out[at] = PLUS_INF, a.ceiling_out[at] = MINUS_INF;
      else if (!in_place) a.floor_out[at] = loaded ? fw[k] : a.floor[at], a.ceiling_out[at] = a.ceiling[at];
    }
    if (a.index_out) a.index_out[at] = blocked ? (int32_t)best[k] : -1;
  }
}

__global__ __launch_bounds__(THREADS) void stamp_things_kernel(StampArgs a, float4 bounds, uint2 things) {
  stamp_tile(a, blockIdx.x / a.tiles, blockIdx.x % a.tiles, bounds, things.x, things.y, 0u, true);
}

// the world set's: row p is level level_of[p] of both sets; a slot outside them has no thing, and its words are passed through
__global__ __launch_bounds__(THREADS) void worldset_stamp_things_kernel(StampArgs a, const float4 *__restrict__ bounds,
                                                                        const uint2 *__restrict__ thing_levels,
                                                                        const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x / a.tiles;
  const uint32_t lv = level_of[p];
  const bool in_set = lv < n_levels;
  uint32_t first = 0, n_things = 0;
  float4 b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (in_set)
    with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) {
      first = thing_levels[slot].x, n_things = thing_levels[slot].y;
      b = bounds[slot];
    });
  stamp_tile(a, p, blockIdx.x % a.tiles, b, first, n_things, in_set ? lv : 0u, in_set);
}

// whether the bytes [a, a + bytes) and [b, b + bytes) meet
bool overlap(const void *a, const void *b, unsigned __int128 bytes) {
  const unsigned __int128 x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && x < y + bytes && y < x + bytes;
}

// what needs no handle, in the header's order
rdoom_status stamp_free_args(uint32_t n, uint32_t width, uint32_t height, const rdoom_stamp_params *params, const float *d_floor,
                             const float *d_ceiling, const float *d_floor_out, const float *d_ceiling_out, const int32_t *d_index_out) {
  if (!params) return rdoom::fail(RDOOM_BAD_ARG, "null params");
  if (!(params->grow >= 0.0f) || !std::isfinite(params->grow)) return rdoom::fail(RDOOM_BAD_ARG, "grow %g is not a finite number >= 0", (double)params->grow);
  if (!(params->block_below >= 0.0f) || !(params->block_above >= 0.0f))
    return rdoom::fail(RDOOM_BAD_ARG, "a vertical window of %g below and %g above (each >= 0)", (double)params->block_below,
                       (double)params->block_above);
  if (params->flags) return rdoom::fail(RDOOM_BAD_ARG, "flags %#x: none is defined", params->flags);
  if (!d_floor_out && !d_ceiling_out && !d_index_out) return rdoom::fail(RDOOM_BAD_ARG, "every output is null: nothing to stamp");
  if (!d_floor_out != !d_ceiling_out) return rdoom::fail(RDOOM_BAD_ARG, "one output plane without the other: floor and ceiling go together");
  if (n && (!d_floor || !d_ceiling)) return rdoom::fail(RDOOM_BAD_ARG, "null floor or ceiling with n = %u", n);
  const unsigned __int128 bytes = (unsigned __int128)n * width * height * 4u;
  const bool in_place = d_floor_out && d_floor_out == d_floor && d_ceiling_out == d_ceiling;
  const void *outs[3] = {d_floor_out, d_ceiling_out, d_index_out}, *ins[2] = {d_floor, d_ceiling};
  for (int o = 0; o < 3; o++) {
    for (int i = 0; i < 2; i++)
      if (overlap(outs[o], ins[i], bytes) && !(in_place && o == i))
        return rdoom::fail(RDOOM_BAD_ARG, "an output overlaps an input: only floor_out == floor together with ceiling_out == ceiling is in place");
    for (int q = o + 1; q < 3; q++)
      if (overlap(outs[o], outs[q], bytes)) return rdoom::fail(RDOOM_BAD_ARG, "two outputs overlap");
  }
  if (!width || !height) return rdoom::fail(RDOOM_BAD_ARG, "planes of %u x %u cells: a side is 0", width, height);
  if (width > RDOOM_AREA_MAX_SIDE || height > RDOOM_AREA_MAX_SIDE)
    return rdoom::fail(RDOOM_BAD_ARG, "planes of %u x %u cells: a side is at most %u", width, height, RDOOM_AREA_MAX_SIDE);
  return RDOOM_OK;
}

// what reads the handle and then the thing set, in the header's order; the kernel's arguments.  noun: "world" or "world set"
rdoom_status stamp_args(const rdoom::MapSource &src, const rdoom_world *w, const rdoom_worldset *set, const char *noun, const char *the_noun,
                        const rdoom_thingset *things, const uint32_t *d_levels, bool needs_levels, uint32_t n, const float *d_offsets,
                        uint32_t n_objects, float cell, uint32_t width, uint32_t height, const uint32_t *d_solid, const uint32_t *d_hidden,
                        uint32_t stride, const rdoom_stamp_params *params, const float *d_floor, const float *d_ceiling, float *d_floor_out,
                        float *d_ceiling_out, int32_t *d_index_out, StampArgs &a) {
  if (rdoom_status s = rdoom::check_device(&src, the_noun)) return s;
  rdoom_area_grid most;
  if (rdoom_status s = rdoom::handle_grid(w, set, src.n_levels, cell, most)) return s;
  if (width < most.gw || height < most.gh)
    return rdoom::fail(RDOOM_BAD_ARG, "planes of %u x %u cells: the %s's grid at cell %g takes %u x %u", width, height, noun, (double)cell, most.gw,
                       most.gh);
  if (needs_levels && n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const uint32_t tiles_x = (width + TILE_X - 1) / TILE_X, tiles_y = (height + TILE_Y - 1) / TILE_Y;
  if ((uint64_t)n * tiles_x * tiles_y > 0x7FFFFFFFull)
    return rdoom::fail(RDOOM_BAD_ARG, "%u rows of %u x %u tiles: too many for one launch", n, tiles_x, tiles_y);
  if (!things) return rdoom::fail(RDOOM_BAD_ARG, "null thing set");
  if (things->n_levels != src.n_levels)
    return rdoom::fail(RDOOM_BAD_ARG, "a thing set of %u levels for a %s of %u", things->n_levels, noun, src.n_levels);
  if (things->device != src.device)
    return rdoom::fail(RDOOM_BAD_ARG, "the thing set lives on device %d, the %s on device %d", things->device, noun, src.device);
  if ((d_solid || d_hidden) && stride < things->words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a row of the thing set's bits takes", stride, things->words);
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (d_offsets && n_objects <= things->max_object_id)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u is not above the thing set's largest object_id %u", n_objects, things->max_object_id);
  a = StampArgs{things->d_things.get(), d_offsets, d_solid, d_hidden, (const uint32_t *)d_floor, (const uint32_t *)d_ceiling,
                (uint32_t *)d_floor_out, (uint32_t *)d_ceiling_out, d_index_out, n_objects, stride, width, height, tiles_x, tiles_x * tiles_y,
                cell, params->grow, -params->block_below, params->block_above};
  return RDOOM_OK;
}

}  // namespace

static_assert(sizeof(rdoom_stamp_params) == 16 && sizeof(rdoom_thing) == 32, "ABI sizes");
static_assert(RDOOM_AREA_MAX_SIDE + TILE_X <= 0x7FFFFFFFu, "a cell's number fits an int32");

extern "C" {

rdoom_status rdoom_world_stamp_things(const rdoom_world *w, const rdoom_thingset *things, uint32_t n, const float *d_object_offsets,
                                      uint32_t n_objects, float cell, uint32_t width, uint32_t height, const uint32_t *d_solid,
                                      const uint32_t *d_hidden, uint32_t stride, const rdoom_stamp_params *params, const float *d_floor,
                                      const float *d_ceiling, float *d_floor_out, float *d_ceiling_out, int32_t *d_index_out, void *stream) {
  if (rdoom_status s = stamp_free_args(n, width, height, params, d_floor, d_ceiling, d_floor_out, d_ceiling_out, d_index_out)) return s;
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  StampArgs a;
  if (rdoom_status s = stamp_args(src, w, nullptr, "world", "the world", things, nullptr, false, n, d_object_offsets, n_objects, cell, width, height,
                                  d_solid, d_hidden, stride, params, d_floor, d_ceiling, d_floor_out, d_ceiling_out, d_index_out, a))
    return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(stamp_things_kernel, dim3(n * a.tiles), dim3(THREADS), 0, stream, a, src.bounds[0], things->level0);
}

rdoom_status rdoom_worldset_stamp_things(const rdoom_worldset *set, const rdoom_thingset *things, const uint32_t *d_levels, uint32_t n,
                                         const float *d_object_offsets, uint32_t n_objects, float cell, uint32_t width, uint32_t height,
                                         const uint32_t *d_solid, const uint32_t *d_hidden, uint32_t stride, const rdoom_stamp_params *params,
                                         const float *d_floor, const float *d_ceiling, float *d_floor_out, float *d_ceiling_out,
                                         int32_t *d_index_out, void *stream) {
  if (rdoom_status s = stamp_free_args(n, width, height, params, d_floor, d_ceiling, d_floor_out, d_ceiling_out, d_index_out)) return s;
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  const rdoom::MapSource src = rdoom::map_source(set);
  StampArgs a;
  if (rdoom_status s = stamp_args(src, nullptr, set, "world set", "the world set", things, d_levels, true, n, d_object_offsets, n_objects, cell,
                                  width, height, d_solid, d_hidden, stride, params, d_floor, d_ceiling, d_floor_out, d_ceiling_out, d_index_out, a))
    return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_stamp_things_kernel, dim3(n * a.tiles), dim3(THREADS), 0, stream, a, (const float4 *)src.map->bounds.get(),
                               (const uint2 *)things->d_levels.get(), d_levels, src.map->n_levels);
}

}  // extern "C"
