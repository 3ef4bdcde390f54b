// Every player's thing marks on the automap grid (include/rdoom.h "thing maps"): rdoom_thingset_draw_maps.  The
// thing set is things.hip's (thingset.hpp); the pixel-to-world mapping is the line maps' (world_shared.hpp), so a mark lies on
// draw_maps' pixels exactly.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off, so an IEEE host
// evaluating the header's expressions gets the same bytes (tests/thingmap_ref.py does).
//
// Shape: automap.hip's.  One 256-thread workgroup per (player, 32 x 32 pixel tile).  The threads stride over the level's things, 256
// at a time; a thread reads its thing's record in two 16-byte loads, decides whether the thing is drawn for this player -- its
// category's code, its bit of the hidden row, its bit of the known row -- and keeps it when its disc can reach the tile: a
// distance test against the tile's centre, conservative under rounding (CULL_MARGIN).  The kept things go into a list in LDS
// (world_shared.hpp's append) as (x, z, r2, key), and each thread folds its four pixels over the list: the pixel value is the
// maximum key, so the order of the list and where it is cut do not matter, and a list that would outgrow LDS is folded and emptied
// in between.  A wave holds two rows of 32 pixels: its byte stores are two runs of 32 consecutive bytes, its index stores two runs
// of 128.  Plain vector stores, no atomics.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "thingset.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::with_level;

constexpr uint32_t WAVE = 64, THREADS = 256, WAVES = THREADS / WAVE;
constexpr uint32_t TILE = 32;                       // pixels a side
constexpr uint32_t PIXELS = TILE * TILE / THREADS;  // per thread: rows (tid / 32) + 8 k of column tid % 32
constexpr uint32_t ROW_STEP = THREADS / TILE;
constexpr uint32_t LIST_CAP = 768;                  // things the LDS list holds: 768 x 16 bytes = 12 KiB
constexpr uint32_t INDEX_BITS = 20, INDEX_MASK = (1u << INDEX_BITS) - 1u;  // a level of a set holds at most 2^20 things
// Half the diagonal of a tile's pixel centres, in pixels: 15.5 * sqrt(2) = 21.92, rounded up.
constexpr float TILE_RADIUS = 22.0f;
// The cull's rounding margin, relative to the magnitude of the coordinates involved: 2^-16, sixteen times the 2^-20 that bounds
// the error of a computed distance.
constexpr float CULL_MARGIN = 1.52587890625e-5f;

struct ThingMapArgs {
  const rdoom_player_state *states;
  const rdoom_thing *things;   // the set's records, level after level
  const uint2 *levels;         // a slot's (first record, number of records)
  const uint32_t *level_of;    // a slot per player, or null: slot 0
  const uint32_t *hidden;      // n rows of stride words, or null: nothing is hidden
  const uint32_t *known;       // n rows of stride words, or null: everything is known
  uint8_t *out;                // n x height x width, or null
  int32_t *index_out;          // n x height x width, or null
  uint32_t n_levels, stride, width, height, tiles_x, tiles;  // tiles: per map
  float scale, rp;             // rp = min_radius * scale
  uint32_t view_flags, over;
  uint32_t codes_lo, codes_hi; // the eight codes, category c in byte c % 4 of word c / 4
};

__global__ __launch_bounds__(THREADS) void draw_thing_maps_kernel(ThingMapArgs a) {
  __shared__ float4 list[LIST_CAP];  // x, z, r2, the key (as bits)
  __shared__ uint32_t wave_kept[WAVES];

  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const uint32_t p = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  // the things of the player's level; a slot outside the set has none
  const uint32_t lv = a.level_of ? a.level_of[p] : 0u;
  uint32_t first = 0, n_things = 0;
  if (lv < a.n_levels)
    with_level(lv, [&](uint32_t slot) __attribute__((always_inline)) { first = a.levels[slot].x, n_things = a.levels[slot].y; });

  const rdoom_dev::MapFrame frame = rdoom_dev::map_frame(a.states + p, a.width, a.height, a.scale, a.view_flags);
  const uint32_t x0 = (tile % a.tiles_x) * TILE, y0 = (tile / a.tiles_x) * TILE;
  const uint32_t i = x0 + (tid & (TILE - 1)), row0 = y0 + tid / TILE;
  float qx[PIXELS], qz[PIXELS];
  uint32_t best[PIXELS];  // the largest key so far; 0: nothing covers (a drawn thing's code is at least 1)
  const float u = rdoom_dev::map_u(frame, i);
#pragma unroll
  for (uint32_t k = 0; k < PIXELS; k++) {
    rdoom_dev::map_to_world(frame, u, rdoom_dev::map_v(frame, row0 + ROW_STEP * k), qx[k], qz[k]);
    best[k] = 0u;
  }

  // the tile's centre, the radius around it that holds every pixel centre, and the magnitude the margin scales with
  float cx, cz;
  {
    const float ci = (float)(x0 + TILE / 2), cj = frame.top_down ? (float)a.height - (float)(y0 + TILE / 2) : (float)(y0 + TILE / 2);
    rdoom_dev::map_to_world(frame, (ci - frame.hw) * a.scale, (cj - frame.hh) * a.scale, cx, cz);
  }
  const float reach = TILE_RADIUS * a.scale;
  const float player_size = (__builtin_fabsf(frame.px) + __builtin_fabsf(frame.pz)) + (float)(a.width + a.height) * a.scale;

  const uint32_t *hidden = a.hidden ? a.hidden + (size_t)p * a.stride : nullptr;
  const uint32_t *known = a.known ? a.known + (size_t)p * a.stride : nullptr;
  const uint4 *const record = reinterpret_cast<const uint4 *>(a.things + first);  // two words of 16 bytes a thing

  uint32_t count = 0;
  for (uint32_t base = 0; base < n_things; base += THREADS) {
    const uint32_t t = base + tid;  // t < 2^20 + 256
    bool keep = false;
    float4 entry = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (t < n_things) {
      const uint4 lo = record[2 * (size_t)t], hi = record[2 * (size_t)t + 1];
      const uint32_t category = hi.w & 7u;  // the low half of the word is `category`, whose low byte the create call holds to 0 .. 7
      const uint32_t code = ((category & 4u ? a.codes_hi : a.codes_lo) >> ((category & 3u) * 8u)) & 0xFFu;
      const uint32_t gone = hidden ? hidden[t >> 5] : 0u, met = known ? known[t >> 5] : ~0u;  // word t / 32 < ceil(T / 32) <= stride
      const bool drawn = code != 0u && !((gone >> (t & 31u)) & 1u) && ((met >> (t & 31u)) & 1u);
      const float x = __uint_as_float(lo.x), z = __uint_as_float(lo.y), radius = __uint_as_float(lo.w);
      const float r = radius > a.rp ? radius : a.rp;
      const float dx = x - cx, dz = z - cz;
      const float size = player_size + ((__builtin_fabsf(x) + __builtin_fabsf(z)) + r);
      const float limit = (reach + r) + size * CULL_MARGIN;
      // "not beyond" rather than "within": a distance that is not a number keeps the thing, and the fold's own comparison, the
      // contract's, decides.  An r * r that overflows comes with a limit * limit that does
      keep = drawn && !(dx * dx + dz * dz > limit * limit);
      entry = make_float4(x, z, r * r, __uint_as_float(code << INDEX_BITS | (INDEX_MASK - t)));
    }
    const rdoom_dev::Appended kept = rdoom_dev::append<WAVES>(keep, lane, wave, wave_kept, count);
    if (keep) list[kept.slot] = entry;  // count <= LIST_CAP - THREADS here, so kept.slot < LIST_CAP
    count += kept.total;
    const bool fold = count > LIST_CAP - THREADS || base + THREADS >= n_things;  // the next 256 might not fit, or there are none
    __syncthreads();
    if (fold) {
      for (uint32_t e = 0; e < count; e++) {
        const float4 g = list[e];
        const uint32_t key = __float_as_uint(g.w);
#pragma unroll
        for (uint32_t k = 0; k < PIXELS; k++) {
          const float ex = qx[k] - g.x, ez = qz[k] - g.y;
          const bool covers = ex * ex + ez * ez <= g.z;
          best[k] = covers && key > best[k] ? key : best[k];
        }
      }
      count = 0;
      __syncthreads();  // before the next things overwrite the list
    }
  }

  if (i < a.width) {
    const size_t map = (size_t)p * a.height * a.width;
#pragma unroll
    for (uint32_t k = 0; k < PIXELS; k++) {
      const uint32_t row = row0 + ROW_STEP * k;
      if (row < a.height) {
        const size_t at = map + (size_t)row * a.width + i;
        if (a.out && (best[k] || !a.over)) a.out[at] = (uint8_t)(best[k] >> INDEX_BITS);
        if (a.index_out) a.index_out[at] = best[k] ? (int32_t)(INDEX_MASK - (best[k] & INDEX_MASK)) : -1;
      }
    }
  }
}

constexpr uint32_t KNOWN_VIEW_FLAGS = RDOOM_MAP_ROTATE | RDOOM_MAP_SHOW_FLAT | RDOOM_MAP_SHOW_HIDDEN | RDOOM_MAP_TOP_DOWN;

}  // namespace

static_assert(sizeof(rdoom_thing_marks) == 16 && sizeof(rdoom_thing) == 32, "ABI sizes");
static_assert(RDOOM_MAP_THING + RDOOM_THING_UNKNOWN <= 0xFFu && RDOOM_MAP_THING > RDOOM_MAP_PLAYER, "the default codes are bytes clear of the line classes");

extern "C" {

rdoom_status rdoom_thingset_draw_maps(const rdoom_thingset *things, const rdoom_player_state *d_states, const uint32_t *d_levels,
                                      uint32_t n, const rdoom_map_view *view, const rdoom_thing_marks *marks, const uint32_t *d_hidden,
                                      const uint32_t *d_known, uint32_t stride, uint8_t *d_out, int32_t *d_index_out, void *stream) {
  // what needs no thing set
  if (!view || !marks) return rdoom::fail(RDOOM_BAD_ARG, "null view or marks");
  if (n && !d_states) return rdoom::fail(RDOOM_BAD_ARG, "null states with n = %u", n);
  if (!d_out && !d_index_out) return rdoom::fail(RDOOM_BAD_ARG, "both outputs are null: nothing to draw");
  if (rdoom_status s = rdoom::check_view(view)) return s;
  if (view->flags & ~KNOWN_VIEW_FLAGS) return rdoom::fail(RDOOM_BAD_ARG, "unknown map flags 0x%x", view->flags);
  if (!(marks->min_radius >= 0.0f) || !std::isfinite(marks->min_radius))
    return rdoom::fail(RDOOM_BAD_ARG, "min_radius %g is not a finite number >= 0", (double)marks->min_radius);
  if (marks->flags & ~RDOOM_THING_MARKS_OVER) return rdoom::fail(RDOOM_BAD_ARG, "unknown thing mark flags 0x%x", marks->flags);
  const uint32_t tiles_x = (view->width + TILE - 1) / TILE, tiles_y = (view->height + TILE - 1) / TILE;
  if ((uint64_t)n * tiles_x * tiles_y > 0x7FFFFFFFull)
    return rdoom::fail(RDOOM_BAD_ARG, "%u maps of %u x %u tiles: too many for one launch", n, tiles_x, tiles_y);
  // what reads it
  if (!things) return rdoom::fail(RDOOM_BAD_ARG, "null thing set");
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != things->device)
    return rdoom::fail(RDOOM_BAD_ARG, "the thing set lives on device %d, the current device is %d", things->device, cur);
  if (!d_levels && things->n_levels > 1)
    return rdoom::fail(RDOOM_BAD_ARG, "null levels with a thing set of %u levels", things->n_levels);
  if ((d_hidden || d_known) && stride < things->words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a row of the thing set's bits takes", stride, things->words);
  if (!n) return RDOOM_OK;
  uint32_t codes[2] = {0u, 0u};
  for (uint32_t c = 0; c < 8; c++) codes[c / 4] |= (uint32_t)marks->codes[c] << (c % 4 * 8);
  const ThingMapArgs a{d_states,       things->d_things.get(), (const uint2 *)things->d_levels.get(), d_levels,     d_hidden,
                       d_known,        d_out,                  d_index_out,                           things->n_levels, stride,
                       view->width,    view->height,           tiles_x,                               tiles_x * tiles_y, view->scale,
                       marks->min_radius * view->scale, view->flags, marks->flags & RDOOM_THING_MARKS_OVER, codes[0], codes[1]};
  return rdoom::launch_checked(draw_thing_maps_kernel, dim3(n * a.tiles), dim3(THREADS), 0, stream, a);
}

}  // extern "C"
