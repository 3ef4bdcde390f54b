// Every player's top-down map, drawn on the device from its game state (include/rdoom.h "top-down maps"):
// rdoom_world_draw_maps, rdoom_worldset_draw_maps, their _seen forms (a map drawn through a player's set of seen lines, which
// reveal.hip keeps) and the device copy of a level's line table.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off and HIP divides
// correctly rounded, so an IEEE host evaluating the header's expressions gets the same bytes (tests/automap_restatement.c does).
// The yaw's sine and cosine are sincos_rd's, the step's and the cameras' (player_quat.hpp).
//
// Shape: one 256-thread workgroup per (player, 32 x 32 pixel tile).  The threads stride over the level's lines, 256 at a time,
// and keep those that can touch the tile -- a distance test against the tile's centre, conservative under rounding (cull_margin)
// -- in a list in LDS, appended with a wave ballot and a prefix over the four waves (world_shared.hpp's append, which the sight
// pass of reveal.hip and area.hip calls too); a kept line's class is computed then, once, from the player's object offsets.
// Each thread then folds its four pixels over the list: the pixel value is a maximum, so the order of the list and where it is
// cut do not matter, and a list that would outgrow LDS is folded and emptied in between.
// A wave holds two rows of 32 pixels: its byte stores are two runs of 32 consecutive bytes.
#include <hip/hip_runtime.h>

#include <vector>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::BOTH_SIDES;
using rdoom_dev::dist2;
using rdoom_dev::live_height;
using rdoom_dev::Segment;
using rdoom_dev::segment;
using rdoom_dev::SIDE_BACK;
using rdoom_dev::SIDE_FRONT;
using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = 256, WAVES = THREADS / WAVE;
constexpr uint32_t TILE = 32;                             // pixels a side
constexpr uint32_t PIXELS = TILE * TILE / THREADS;        // per thread: rows (tid / 32) + 8 k of column tid % 32
constexpr uint32_t ROW_STEP = THREADS / TILE;
constexpr uint32_t LIST_CAP = 512;                        // lines the LDS list holds: 512 x 24 bytes = 12 KiB
constexpr uint32_t LINE_SECRET = 0x20u, LINE_HIDDEN = 0x80u;
// Half the diagonal of a tile's pixel centres, in pixels: 15.5 * sqrt(2) = 21.92, rounded up.
constexpr float TILE_RADIUS = 22.0f;
// The cull's rounding margin, relative to the magnitude of the coordinates involved: 2^-16, sixteen times the 2^-20 that bounds
// the error of a computed distance.
constexpr float CULL_MARGIN = 1.52587890625e-5f;

struct MapArgs {
  const rdoom_player_state *states;
  const float *offsets;  // n x n_objects x xyz, or null
  uint8_t *out;
  const uint32_t *seen;  // n rows of seen_stride words, a bit per line of the player's level (reveal.hip), or null: every line
  uint32_t seen_stride;
  const float4 *seg;
  const float4 *heights;
  const uint4 *ids;
  const uint32_t *flags;
  uint32_t n_objects, width, height, tiles_x, tiles;  // tiles: per map
  float scale, rad, w2, marker;                       // rad = half_width * scale, w2 = rad * rad
  uint32_t view_flags;
};

// the map of player p, tile `tile`, from lines [first, first + n_lines) of the table; blank: no lines and no marker
__device__ __forceinline__ void draw_tile(const MapArgs &a, uint32_t p, uint32_t tile, uint32_t first, uint32_t n_lines, bool blank) {
  __shared__ float4 list_seg[LIST_CAP];  // a.x, a.z, d.x, d.z
  __shared__ float2 list_aux[LIST_CAP];  // inv, the class (as bits)
  __shared__ uint32_t wave_kept[WAVES];

  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const rdoom_dev::MapFrame frame = rdoom_dev::map_frame(a.states + p, a.width, a.height, a.scale, a.view_flags);
  const float px = frame.px, pz = frame.pz, fx = frame.fx, fz = frame.fz;  // (fx, fz): the forward ray_fan's -z turns into
  const bool show_flat = a.view_flags & RDOOM_MAP_SHOW_FLAT, show_hidden = a.view_flags & RDOOM_MAP_SHOW_HIDDEN;

  const uint32_t x0 = (tile % a.tiles_x) * TILE, y0 = (tile / a.tiles_x) * TILE;
  const uint32_t i = x0 + (tid & (TILE - 1)), row0 = y0 + tid / TILE;
  float qx[PIXELS], qz[PIXELS];
  uint32_t best[PIXELS];
  const float u = rdoom_dev::map_u(frame, i);
#pragma unroll
  for (uint32_t k = 0; k < PIXELS; k++) {
    rdoom_dev::map_to_world(frame, u, rdoom_dev::map_v(frame, row0 + ROW_STEP * k), qx[k], qz[k]);
    best[k] = RDOOM_MAP_NONE;
  }

  // the tile's centre, the radius around it that holds every pixel centre, and the magnitude the margin scales with
  float cx, cz;
  {
    const float ci = (float)(x0 + TILE / 2), cj = frame.top_down ? (float)a.height - (float)(y0 + TILE / 2) : (float)(y0 + TILE / 2);
    rdoom_dev::map_to_world(frame, (ci - frame.hw) * a.scale, (cj - frame.hh) * a.scale, cx, cz);
  }
  const float reach = TILE_RADIUS * a.scale + a.rad;
  const float player_size = (__builtin_fabsf(px) + __builtin_fabsf(pz)) + (float)(a.width + a.height) * a.scale;

  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;
  const auto live = [&](float height, uint32_t object) __attribute__((always_inline)) { return live_height(height, object, off, a.n_objects); };
  const uint32_t *seen = a.seen ? a.seen + (size_t)p * a.seen_stride : nullptr;

  uint32_t count = 0;
  for (uint32_t base = 0; base < n_lines; base += THREADS) {
    const uint32_t l = base + tid;
    bool keep = false;
    Segment g{};
    uint32_t cls = RDOOM_MAP_ONE_SIDED;
    if (l < n_lines) {
      const float4 e = a.seg[first + l];
      const uint32_t fl = a.flags[first + l];
      g = segment(e.x, e.y, e.z, e.w);
      const float size = player_size + ((__builtin_fabsf(e.x) + __builtin_fabsf(e.y)) + (__builtin_fabsf(e.z) + __builtin_fabsf(e.w)));
      const float limit = reach + size * CULL_MARGIN;
      keep = g.ok && dist2(cx, cz, g.ax, g.az, g.dx, g.dz, g.inv) <= limit * limit && (show_hidden || !(fl & LINE_HIDDEN));
      if (keep && seen) keep = (fl & RDOOM_LINE_MAPPED) || ((seen[l >> 5] >> (l & 31u)) & 1u);  // drawn through the seen set
      if (keep && (fl & BOTH_SIDES) == BOTH_SIDES && !(fl & LINE_SECRET)) {
        const float4 h = a.heights[first + l];
        const uint4 o = a.ids[first + l];
        const float ff = live(h.x, o.x), fc = live(h.y, o.y), bf = live(h.z, o.z), bc = live(h.w, o.w);
        cls = (fc <= ff || bc <= bf) ? RDOOM_MAP_CLOSED
                                     : (ff != bf ? RDOOM_MAP_FLOOR_STEP : (fc != bc ? RDOOM_MAP_CEILING_STEP : RDOOM_MAP_FLAT));
        keep = cls != RDOOM_MAP_FLAT || show_flat;
      }
    }
    const rdoom_dev::Appended kept = rdoom_dev::append<WAVES>(keep, lane, wave, wave_kept, count);
    if (keep) {  // count <= LIST_CAP - THREADS here, so kept.slot < LIST_CAP
      list_seg[kept.slot] = make_float4(g.ax, g.az, g.dx, g.dz);
      list_aux[kept.slot] = make_float2(g.inv, __uint_as_float(cls));
    }
    count += kept.total;
    const bool fold = count > LIST_CAP - THREADS || base + THREADS >= n_lines;  // the next 256 might not fit, or there are none
    __syncthreads();
    if (fold) {
      for (uint32_t e = 0; e < count; e++) {
        const float4 sg = list_seg[e];
        const float2 aux = list_aux[e];
        const uint32_t line_cls = __float_as_uint(aux.y);
#pragma unroll
        for (uint32_t k = 0; k < PIXELS; k++) {
          const bool covers = dist2(qx[k], qz[k], sg.x, sg.y, sg.z, sg.w, aux.x) <= a.w2;
          best[k] = covers && line_cls > best[k] ? line_cls : best[k];
        }
      }
      count = 0;
      __syncthreads();  // before the next lines overwrite the list
    }
  }

  if (a.marker > 0.0f && !blank) {
    const float m = a.marker * a.scale;
    const Segment g = segment(px, pz, px + fx * (2.0f * m), pz + fz * (2.0f * m));
    const float m2 = m * m;
#pragma unroll
    for (uint32_t k = 0; k < PIXELS; k++)
      if (g.ok && dist2(qx[k], qz[k], g.ax, g.az, g.dx, g.dz, g.inv) <= m2) best[k] = RDOOM_MAP_PLAYER;
  }

  if (i < a.width) {
    uint8_t *map = a.out + (size_t)p * a.height * a.width;
#pragma unroll
    for (uint32_t k = 0; k < PIXELS; k++) {
      const uint32_t row = row0 + ROW_STEP * k;
      if (row < a.height) map[(size_t)row * a.width + i] = (uint8_t)best[k];
    }
  }
}

__global__ __launch_bounds__(THREADS) void draw_maps_kernel(MapArgs a, uint32_t n_lines) {
  draw_tile(a, blockIdx.x / a.tiles, blockIdx.x % a.tiles, 0u, n_lines, false);
}

// the world set's: player p's map shows level level_of[p]; a slot outside the set gives an all-zero map
__global__ __launch_bounds__(THREADS) void worldset_draw_maps_kernel(MapArgs a, const uint2 *__restrict__ levels,
                                                                     const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x / a.tiles;
  const uint32_t lv = level_of[p];
  uint32_t first = 0, n_lines = 0;
  if (lv < n_levels)
    with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) { first = levels[slot].x, n_lines = levels[slot].y; });
  draw_tile(a, p, blockIdx.x % a.tiles, first, n_lines, lv >= n_levels);
}

constexpr uint32_t KNOWN_FLAGS = RDOOM_MAP_ROTATE | RDOOM_MAP_SHOW_FLAT | RDOOM_MAP_SHOW_HIDDEN | RDOOM_MAP_TOP_DOWN;

// the arguments of a draw, checked, as the kernel takes them.  noun: "world" or "world set"
rdoom_status map_args(const rdoom::MapSource &src, const char *noun, const rdoom_player_state *d_states, uint32_t n,
                      const float *d_offsets, uint32_t n_objects, const rdoom_map_view *view, const uint32_t *d_seen, uint32_t stride,
                      uint8_t *d_out, MapArgs &a) {
  if (!view) return rdoom::fail(RDOOM_BAD_ARG, "null view");
  if (n && (!d_states || !d_out)) return rdoom::fail(RDOOM_BAD_ARG, "null states or output with n = %u", n);
  if (rdoom_status s = rdoom::check_view(view)) return s;
  const float inf = __builtin_inff();
  if (!(view->half_width > 0.0f) || view->half_width == inf)
    return rdoom::fail(RDOOM_BAD_ARG, "half_width %g is not a finite positive number", (double)view->half_width);
  if (!(view->marker >= 0.0f) || view->marker == inf)
    return rdoom::fail(RDOOM_BAD_ARG, "marker %g is not a finite non-negative number", (double)view->marker);
  if (view->flags & ~KNOWN_FLAGS) return rdoom::fail(RDOOM_BAD_ARG, "unknown map flags 0x%x", view->flags);
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (d_seen)
    if (rdoom_status s = rdoom::check_seen_stride(src, noun, stride)) return s;
  const uint32_t tiles_x = (view->width + TILE - 1) / TILE, tiles_y = (view->height + TILE - 1) / TILE;
  if ((uint64_t)n * tiles_x * tiles_y > 0x7FFFFFFFull)
    return rdoom::fail(RDOOM_BAD_ARG, "%u maps of %u x %u tiles: too many for one launch", n, tiles_x, tiles_y);
  const float rad = view->half_width * view->scale;
  const rdoom::MapDevice &d = *src.map;
  a = MapArgs{d_states, d_offsets, d_out, d_seen, stride, d.seg.get(), d.heights.get(), d.ids.get(), d.flags.get(), n_objects, view->width, view->height, tiles_x,
              tiles_x * tiles_y, view->scale, rad, rad * rad, view->marker, view->flags};
  return RDOOM_OK;
}

}  // namespace

namespace rdoom {

rdoom_status map_upload(const std::vector<rdoom_map_line> &lines, const std::vector<uint2> &levels, MapDevice &out) {
  std::vector<float4> seg, heights;
  std::vector<uint4> ids;
  std::vector<uint32_t> flags;
  for (const rdoom_map_line &l : lines) {
    seg.push_back(make_float4(l.a[0], l.a[1], l.b[0], l.b[1]));
    heights.push_back(make_float4(l.front.floor, l.front.ceiling, l.back.floor, l.back.ceiling));
    ids.push_back(make_uint4(l.front.floor_id, l.front.ceiling_id, l.back.floor_id, l.back.ceiling_id));
    flags.push_back((l.flags & 0xFFFFu) | (l.front.present ? SIDE_FRONT : 0u) | (l.back.present ? SIDE_BACK : 0u));
  }
  if (rdoom_status s = out.seg.upload(seg, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.heights.upload(heights, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.ids.upload(ids, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.flags.upload(flags, EMPTY_TABLE_BYTES)) return s;
  std::vector<float4> bounds;
  for (const uint2 &r : levels) bounds.push_back(line_bounds(lines.data() + r.x, r.y));
  if (rdoom_status s = out.levels.upload(levels, EMPTY_TABLE_BYTES)) return s;
  if (rdoom_status s = out.bounds.upload(bounds, EMPTY_TABLE_BYTES)) return s;
  out.n_lines = (uint32_t)lines.size(), out.n_levels = (uint32_t)levels.size();
  return RDOOM_OK;
}

}  // namespace rdoom

static_assert(sizeof(rdoom_map_side) == 20 && sizeof(rdoom_map_line) == 68 && sizeof(rdoom_map_view) == 24, "ABI sizes");

extern "C" {

rdoom_status rdoom_world_draw_maps_seen(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const float *d_object_offsets,
                                        uint32_t n_objects, const rdoom_map_view *view, const uint32_t *d_seen, uint32_t stride,
                                        uint8_t *d_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  MapArgs a;
  if (rdoom_status s = map_args(src, "world", d_states, n, d_object_offsets, n_objects, view, d_seen, stride, d_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(draw_maps_kernel, dim3(n * a.tiles), dim3(THREADS), 0, stream, a, src.map->n_lines);
}

rdoom_status rdoom_worldset_draw_maps_seen(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                           uint32_t n, const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view,
                                           const uint32_t *d_seen, uint32_t stride, uint8_t *d_out, void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  MapArgs a;
  if (rdoom_status s = map_args(src, "world set", d_states, n, d_object_offsets, n_objects, view, d_seen, stride, d_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_draw_maps_kernel, dim3(n * a.tiles), dim3(THREADS), 0, stream, a, (const uint2 *)src.map->levels.get(),
                               d_levels, src.map->n_levels);
}

// the omniscient maps: the _seen forms with no set
rdoom_status rdoom_world_draw_maps(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const float *d_object_offsets,
                                   uint32_t n_objects, const rdoom_map_view *view, uint8_t *d_out, void *stream) {
  return rdoom_world_draw_maps_seen(w, d_states, n, d_object_offsets, n_objects, view, nullptr, 0, d_out, stream);
}

rdoom_status rdoom_worldset_draw_maps(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                      const float *d_object_offsets, uint32_t n_objects, const rdoom_map_view *view, uint8_t *d_out,
                                      void *stream) {
  return rdoom_worldset_draw_maps_seen(set, d_states, d_levels, n, d_object_offsets, n_objects, view, nullptr, 0, d_out, stream);
}

}  // extern "C"
