// Each player's explored area, kept on the device (include/rdoom.h "explored area"): the grid of a level,
// rdoom_world_reveal_area, rdoom_world_draw_area_maps and their world-set forms.
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off and HIP divides
// correctly rounded, so an IEEE host evaluating the header's expressions gets the same bits (tests/area_restatement.c does).  The
// grid formulas are one host-and-device function: the host checks the limits with it, the kernels index with it.
//
// reveal_area: one 256-thread workgroup per player, the fan taken 256 rays at a time.  A pass over that many rays:
// Sight limits.  T_r of every ray: sight.hpp's sight_limits, the one pass this unit and reveal.hip share, over this kernel's LDS
// arrays.
// Window.  The samples of the pass fall into a window of the grid that is known before any is taken: the word-aligned columns and the
// rows between the cells of pos -+ the largest |vel| component of the pass, clipped to the grid (axis_window: exact, no margin is
// needed).  The two bit planes of the window live in LDS, WINDOW_WORDS words for both; a window with more rows than that holds is
// taken in horizontal bands, each a zero - sample - merge cycle over the same rays that keeps the samples of its rows; a chunk of
// steps whose two ends lie above or below the band is passed over.
// Sample.  Threads own (ray, chunk of CHUNK steps) items, consecutive threads consecutive rays; a thread walks its steps while
// t <= T_r, gathers the bits that fall into one word in a register and ORs the word into LDS when the word changes.
// Merge.  A thread per window word: the global word is loaded, the bits it lacks are counted and, if there are any, the OR is stored.
// A player's row belongs to one workgroup, so nothing global is atomic and the count is exact.
// Every barrier is reached by every thread: the pass, band and list loops run on values every thread computes alike from LDS words
// read after a barrier.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "player_quat.hpp"
#include "sight.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::sincos_rd;
using rdoom_dev::wave_max;
using rdoom_dev::wave_sum;

constexpr uint32_t WAVE = 64, THREADS = rdoom_dev::SIGHT_THREADS, WAVES = THREADS / WAVE;
constexpr uint32_t WINDOW_WORDS = 4096;  // the LDS window, both planes: 16 KiB of the unit's 25
constexpr uint32_t CHUNK = 32;           // the steps of a sampling item

// ---- the grid of a level (the contract's formulas; host and device): world_shared.hpp's, which goal.hip reads too ----
using rdoom_dev::cell_of;
using rdoom_dev::CELL_LIMIT;
using rdoom_dev::Grid;
using rdoom_dev::grid_of;
using rdoom_dev::point_cell;

struct AreaArgs {
  const rdoom_player_state *states;
  const float *offsets;  // n x n_objects x xyz, or null
  const float *dirs;     // n_rays x (right, forward): a caller's floats, dword aligned and no more
  uint32_t *area;        // n x 2 x stride words
  uint32_t *new_out;     // n x 2, or null
  rdoom_dev::LineTable lines;
  uint32_t n_objects, n_rays, stride, n_steps;
  float max_range, cell;
};

// The cells [lo, hi] of the grid axis (first cell c0, n cells) that a sample o + t * vel can fall into when |vel| <= reach on this
// axis: t * vel is within -+reach (|t| <= 1, reach is a binary32 and rounding is monotone), so the sum is within round(o - reach) and
// round(o + reach), and cx() is monotone.  Exact: no margin.  false: no cell (a NaN, or beside the grid).
__device__ __forceinline__ bool axis_window(float o, float reach, float cell, int32_t c0, uint32_t n, uint32_t &lo, uint32_t &hi) {
  const float a = (o - reach) / cell, b = (o + reach) / cell;
  if (!(a == a && b == b)) return false;
  const int32_t first = a <= -CELL_LIMIT ? -0x40000000 - 2 : (a >= CELL_LIMIT ? 0x40000000 : (int32_t)__builtin_floorf(a));
  const int32_t last = b <= -CELL_LIMIT ? -0x40000000 - 2 : (b >= CELL_LIMIT ? 0x40000000 : (int32_t)__builtin_floorf(b));
  const int32_t end = c0 + (int32_t)n - 1;  // c0 is within -+(2^30 + 1), n <= 8192
  const int32_t from = first > c0 ? first : c0, to = last < end ? last : end;
  if (from > to) return false;
  lo = (uint32_t)(from - c0), hi = (uint32_t)(to - c0);
  return true;
}

// The accumulation kernel is short of scalar registers, not of vector ones: a workgroup-uniform float that every sample reads is
// kept in a vector register, which costs nothing there and saves a scalar spill
__device__ __forceinline__ float in_vgpr(float v) {
  asm("" : "+v"(v));
  return v;
}

// the explored area of player p among lines [first, first + n_lines) of the table, on the grid of `bounds`
__device__ __forceinline__ void reveal_area_player(const AreaArgs &a, uint32_t p, float4 bounds, uint32_t first, uint32_t n_lines) {
  __shared__ uint32_t window[WINDOW_WORDS];  // a band's FREE plane, then its WALL plane
  __shared__ float4 list[THREADS];           // the blocking lines at hand: w.x, w.z, d.x, d.z
  __shared__ float4 rays[THREADS];           // the pass's rays: vel.x, vel.z, T_r
  __shared__ float part[THREADS];            // the minima, one per thread
  __shared__ float wave_reach[3][WAVES];     // |vel|^2, |vel.x|, |vel.z|: the largest of each wave
  __shared__ uint32_t wave_count[2][WAVES];

  const uint32_t tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const rdoom_player_state *st = a.states + p;
  const float px = in_vgpr(st->pos[0]), pz = in_vgpr(st->pos[2]);
  float s, c;
  sincos_rd(in_vgpr(st->yaw), s, c);
  const float fx = -s, fz = -c;  // the map's forward; its right is (c, -s)
  const float *off = a.offsets ? a.offsets + (size_t)p * a.n_objects * 3 : nullptr;
  uint32_t *free_row = a.area + (size_t)p * 2 * a.stride, *wall_row = free_row + a.stride;
  Grid g;
  grid_of(bounds, a.cell, g);
  const float cell = in_vgpr(a.cell), steps_f = in_vgpr((float)a.n_steps);
  const uint32_t n_chunks = (a.n_steps + CHUNK) / CHUNK;  // of the n_steps + 1 samples of a ray
  uint32_t fresh_free = 0, fresh_wall = 0;                // the bits this thread set that were clear

  for (uint32_t ray0 = 0; ray0 < a.n_rays; ray0 += THREADS) {
    const uint32_t nr = a.n_rays - ray0 < THREADS ? a.n_rays - ray0 : THREADS;
    // the pass's rays, the longest of them (no hit lies farther from the player) and their largest components (no sample does)
    float len2 = 0.0f, ax = 0.0f, az = 0.0f;
    if (tid < nr) {
      const float dr = a.dirs[2 * (size_t)(ray0 + tid)], df = a.dirs[2 * (size_t)(ray0 + tid) + 1];
      const float dir_x = c * dr + fx * df, dir_z = fx * dr + fz * df;
      const float vx = dir_x * a.max_range, vz = dir_z * a.max_range;
      rays[tid] = make_float4(vx, vz, 1.0f, 0.0f);
      len2 = vx * vx + vz * vz, ax = __builtin_fabsf(vx), az = __builtin_fabsf(vz);
    }
    len2 = wave_max(len2), ax = wave_max(ax), az = wave_max(az);
    if (lane == 0) wave_reach[0][wave] = len2, wave_reach[1][wave] = ax, wave_reach[2][wave] = az;
    __syncthreads();
    const float reach = __builtin_sqrtf(__builtin_fmaxf(__builtin_fmaxf(wave_reach[0][0], wave_reach[0][1]), __builtin_fmaxf(wave_reach[0][2], wave_reach[0][3])));
    const float reach_x = __builtin_fmaxf(__builtin_fmaxf(wave_reach[1][0], wave_reach[1][1]), __builtin_fmaxf(wave_reach[1][2], wave_reach[1][3]));
    const float reach_z = __builtin_fmaxf(__builtin_fmaxf(wave_reach[2][0], wave_reach[2][1]), __builtin_fmaxf(wave_reach[2][2], wave_reach[2][3]));
    const float player_size = (__builtin_fabsf(px) + __builtin_fabsf(pz)) + reach;

    // ---- sight limits: T_r into rays[r].z
    rdoom_dev::sight_limits(a.lines, off, a.n_objects, first, n_lines, px, pz, reach, player_size, nr, list, rays, part, wave_count[0]);

    // ---- the window of the pass: columns c_lo .. c_hi as whole words, rows r_lo .. r_hi, in bands of band_rows
    uint32_t c_lo = 0, c_hi = 0, r_lo = 0, r_hi = 0;
    const bool any = axis_window(px, reach_x, cell, g.ix0, g.gw, c_lo, c_hi) & axis_window(pz, reach_z, cell, g.iz0, g.gh, r_lo, r_hi);
    const uint32_t word0 = c_lo >> 5, w_pitch = (c_hi >> 5) - word0 + 1;  // w_pitch <= pitch <= 256
    const uint32_t band_rows = (WINDOW_WORDS / 2) / w_pitch;               // >= 8
    const uint32_t w_rows = any ? r_hi - r_lo + 1 : 0u;
    const uint32_t items = nr * n_chunks;
    const bool banded = w_rows > band_rows;

    for (uint32_t b0 = 0; b0 < w_rows; b0 += band_rows) {
      const uint32_t row0 = r_lo + b0, rows = w_rows - b0 < band_rows ? w_rows - b0 : band_rows;
      const uint32_t plane = rows * w_pitch;  // <= WINDOW_WORDS / 2
      for (uint32_t i = tid; i < 2 * plane; i += THREADS) window[i] = 0u;
      __syncthreads();

      // the word of the band's FREE plane that holds the cell of (x, z), and the cell's bit in it; false: none of this band's
      auto locate = [&](float x, float z, uint32_t &word, uint32_t &bit) {
        uint32_t ix, iz;
        const bool in_grid = point_cell(g, cell, x, z, ix, iz);
        const uint32_t col = (ix >> 5) - word0, row = iz - row0;
        word = row * w_pitch + col, bit = 1u << (ix & 31u);
        return in_grid && col < w_pitch && row < rows;
      };
      for (uint32_t item = tid; item < items; item += THREADS) {
        const uint32_t chunk = item / nr, r = item - chunk * nr;
        const float4 v = rays[r];
        const uint32_t k0 = chunk * CHUNK;
        uint32_t k1 = k0 + CHUNK < a.n_steps + 1 ? k0 + CHUNK : a.n_steps + 1;
        if (banded) {
          // z grows or falls with t (each operation is monotone), so the rows of the chunk's samples lie between those of its first
          // t and of a t at or beyond its last: a chunk whose two ends lie on the same side of the band has no sample in it
          const float t_end = __builtin_fminf((float)(k1 - 1) / steps_f, v.z);
          int32_t ra, rb;
          const bool known = cell_of(pz + ((float)k0 / steps_f) * v.y, cell, ra) & cell_of(pz + t_end * v.y, cell, rb);
          const int32_t lo = g.iz0 + (int32_t)row0, hi = lo + (int32_t)rows - 1;  // the band's rows as cx() values
          if (known && ((ra < lo && rb < lo) || (ra > hi && rb > hi))) k1 = k0;
        }
        uint32_t held = 0xFFFFFFFFu, bits = 0;  // the word the bits gathered so far belong to
        for (uint32_t k = k0; k < k1; k++) {
          const float t = (float)k / steps_f;
          if (!(t <= v.z)) break;  // t grows with k
          uint32_t word, bit;
          if (locate(px + t * v.x, pz + t * v.y, word, bit)) {
            if (word != held) {
              if (bits) atomicOr(&window[held], bits);
              held = word, bits = 0;
            }
            bits |= bit;
          }
        }
        if (bits) atomicOr(&window[held], bits);
        if (chunk == 0 && v.z < 1.0f) {
          uint32_t word, bit;
          if (locate(px + v.z * v.x, pz + v.z * v.y, word, bit)) atomicOr(&window[plane + word], bit);
        }
      }
      __syncthreads();

      for (uint32_t i = tid; i < plane; i += THREADS) {
        const uint32_t row = i / w_pitch, col = i - row * w_pitch;
        const uint32_t at = (row0 + row) * g.pitch + word0 + col;  // < gh * pitch = the level's words <= stride
        const uint32_t f = window[i], w = window[plane + i];
        if (f) {
          const uint32_t old = free_row[at], add = f & ~old;
          fresh_free += (uint32_t)__builtin_popcount(add);
          if (add) free_row[at] = old | f;
        }
        if (w) {
          const uint32_t old = wall_row[at], add = w & ~old;
          fresh_wall += (uint32_t)__builtin_popcount(add);
          if (add) wall_row[at] = old | w;
        }
      }
      __syncthreads();  // before the next band zeroes the window, and so that the next pass reads the words stored here
    }
  }

  if (a.new_out) {
    fresh_free = wave_sum(fresh_free), fresh_wall = wave_sum(fresh_wall);
    if (lane == 0) wave_count[0][wave] = fresh_free, wave_count[1][wave] = fresh_wall;
    __syncthreads();
    if (tid < 2) a.new_out[2 * (size_t)p + tid] = (wave_count[tid][0] + wave_count[tid][1]) + (wave_count[tid][2] + wave_count[tid][3]);
  }
}

__global__ __launch_bounds__(THREADS) void reveal_area_kernel(AreaArgs a, float4 bounds, uint32_t n_lines) {
  reveal_area_player(a, blockIdx.x, bounds, 0u, n_lines);
}

// the world set's: player p looks at level level_of[p]; a slot outside the set leaves the row alone and counts 0
__global__ __launch_bounds__(THREADS) void worldset_reveal_area_kernel(AreaArgs a, const uint2 *__restrict__ levels,
                                                                       const float4 *__restrict__ bounds,
                                                                       const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x;
  const uint32_t lv = __builtin_amdgcn_readfirstlane(level_of[p]);  // the workgroup's: every thread takes the same branch
  if (lv >= n_levels) {
    if (a.new_out && threadIdx.x < 2) a.new_out[2 * (size_t)p + threadIdx.x] = 0u;
    return;
  }
  reveal_area_player(a, p, bounds[lv], levels[lv].x, levels[lv].y);
}

// ---- the maps drawn through the rows: a thread per pixel ----
struct AreaMapArgs {
  const rdoom_player_state *states;
  const uint32_t *area;  // n x 2 x stride words
  uint8_t *out;          // n x height x width
  uint32_t stride, width, height, blocks;  // blocks: per map
  float scale, cell;
  uint32_t view_flags;
};

__device__ __forceinline__ void draw_area_pixel(const AreaMapArgs &a, uint32_t p, uint32_t pixel, float4 bounds, bool in_set) {
  if (pixel >= a.width * a.height) return;
  uint8_t value = RDOOM_AREA_UNKNOWN;
  if (in_set) {
    const uint32_t row = pixel / a.width, i = pixel - row * a.width;
    const rdoom_dev::MapFrame f = rdoom_dev::map_frame(a.states + p, a.width, a.height, a.scale, a.view_flags);
    float qx, qz;
    rdoom_dev::map_to_world(f, rdoom_dev::map_u(f, i), rdoom_dev::map_v(f, row), qx, qz);
    Grid g;
    grid_of(bounds, a.cell, g);
    uint32_t ix, iz;
    if (point_cell(g, a.cell, qx, qz, ix, iz)) {
      const uint32_t *free_row = a.area + (size_t)p * 2 * a.stride;
      const uint32_t at = iz * g.pitch + (ix >> 5);  // < the level's words <= stride
      value = (uint8_t)(((free_row[at] >> (ix & 31u)) & 1u) | (((free_row[a.stride + at] >> (ix & 31u)) & 1u) << 1));
    }
  }
  a.out[(size_t)p * a.width * a.height + pixel] = value;
}

__global__ __launch_bounds__(THREADS) void draw_area_maps_kernel(AreaMapArgs a, float4 bounds) {
  draw_area_pixel(a, blockIdx.x / a.blocks, (blockIdx.x % a.blocks) * THREADS + threadIdx.x, bounds, true);
}

__global__ __launch_bounds__(THREADS) void worldset_draw_area_maps_kernel(AreaMapArgs a, const float4 *__restrict__ bounds,
                                                                          const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t p = blockIdx.x / a.blocks;
  const uint32_t lv = level_of[p];
  const bool in_set = lv < n_levels;
  draw_area_pixel(a, p, (blockIdx.x % a.blocks) * THREADS + threadIdx.x, in_set ? bounds[lv] : make_float4(0.0f, 0.0f, 0.0f, 0.0f), in_set);
}

// ---- the host's side ----
rdoom_status check_cell(float cell) {
  if (!(cell > 0.0f) || cell == __builtin_inff()) return rdoom::fail(RDOOM_BAD_ARG, "cell %g is not a finite positive number", (double)cell);
  return RDOOM_OK;
}

// the grid of level `slot` of the handle at a checked cell, within the contract's limits.  noun: "world" or "world set"
rdoom_status level_grid(const rdoom::MapSource &src, const char *noun, uint32_t slot, float cell, rdoom_area_grid &out) {
  Grid g;
  const bool ok = grid_of(src.bounds[slot], cell, g);
  if (!ok || g.gw > RDOOM_AREA_MAX_SIDE || g.gh > RDOOM_AREA_MAX_SIDE || (uint64_t)g.gh * g.pitch > RDOOM_AREA_MAX_WORDS) {
    if (!ok) return rdoom::fail(RDOOM_BAD_ARG, "at cell %g the grid of the %s's level %u is over its limits: a bound is 2^30 cells or more from 0", (double)cell, noun, slot);
    return rdoom::fail(RDOOM_BAD_ARG, "at cell %g the grid of the %s's level %u is over its limits: %u x %u cells, %llu words (at most %u a side and %u words)",
                       (double)cell, noun, slot, g.gw, g.gh, (unsigned long long)g.gh * g.pitch, RDOOM_AREA_MAX_SIDE, RDOOM_AREA_MAX_WORDS);
  }
  out = rdoom_area_grid{g.ix0, g.iz0, g.gw, g.gh, g.pitch, g.gh * g.pitch};
  return RDOOM_OK;
}

// the handle's area words at a checked cell: the largest level's, every level within the limits
rdoom_status area_words(const rdoom::MapSource &src, const char *noun, float cell, uint32_t &words) {
  words = 0;
  for (uint32_t slot = 0; slot < src.n_levels; slot++) {
    rdoom_area_grid g;
    if (rdoom_status s = level_grid(src, noun, slot, cell, g)) return s;
    words = g.words > words ? g.words : words;
  }
  return RDOOM_OK;
}

rdoom_status check_area_rows(const rdoom::MapSource &src, const char *noun, float cell, uint32_t stride) {
  if (rdoom_status s = check_cell(cell)) return s;
  uint32_t words;
  if (rdoom_status s = area_words(src, noun, cell, words)) return s;
  if (stride < words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a plane of the %s's grid takes at cell %g", stride, words, noun,
                       (double)cell);
  return RDOOM_OK;
}

// the arguments of a reveal, checked, as the kernel takes them.  noun: "world" or "world set"
rdoom_status reveal_args(const rdoom::MapSource &src, const char *noun, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs,
                         uint32_t n_rays, float max_range, const float *d_offsets, uint32_t n_objects, float cell, uint32_t n_steps,
                         uint32_t *d_area, uint32_t stride, uint32_t *d_new_out, AreaArgs &a) {
  if (n && (!d_states || !d_area || !d_dirs)) return rdoom::fail(RDOOM_BAD_ARG, "null states, area rows or directions with n = %u", n);
  if (rdoom_status s = rdoom::check_fan(n_rays, max_range)) return s;
  if (!n_steps || n_steps > RDOOM_AREA_MAX_STEPS) return rdoom::fail(RDOOM_BAD_ARG, "n_steps %u (1 .. %u)", n_steps, RDOOM_AREA_MAX_STEPS);
  if (rdoom_status s = check_area_rows(src, noun, cell, stride)) return s;
  if (rdoom_status s = rdoom::check_offsets(d_offsets, n_objects, src.game_objects, noun)) return s;
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u players: too many for one launch", n);
  const rdoom::MapDevice &d = *src.map;
  a = AreaArgs{d_states, d_offsets, d_dirs, d_area, d_new_out, {d.seg.get(), d.heights.get(), d.ids.get(), d.flags.get()}, n_objects, n_rays, stride, n_steps,
               max_range, cell};
  return RDOOM_OK;
}

rdoom_status map_args(const rdoom::MapSource &src, const char *noun, const rdoom_player_state *d_states, uint32_t n, const rdoom_map_view *view,
                      const uint32_t *d_area, uint32_t stride, float cell, uint8_t *d_out, AreaMapArgs &a) {
  if (!view) return rdoom::fail(RDOOM_BAD_ARG, "null view");
  if (n && (!d_states || !d_area || !d_out)) return rdoom::fail(RDOOM_BAD_ARG, "null states, area rows or output with n = %u", n);
  if (rdoom_status s = rdoom::check_view(view)) return s;
  if (view->flags & ~(RDOOM_MAP_ROTATE | RDOOM_MAP_TOP_DOWN)) return rdoom::fail(RDOOM_BAD_ARG, "map flags 0x%x: an area map takes ROTATE and TOP_DOWN", view->flags);
  if (rdoom_status s = check_area_rows(src, noun, cell, stride)) return s;
  const uint32_t blocks = (view->width * view->height + THREADS - 1) / THREADS;
  if ((uint64_t)n * blocks > 0x7FFFFFFFull) return rdoom::fail(RDOOM_BAD_ARG, "%u maps of %u blocks of pixels: too many for one launch", n, blocks);
  a = AreaMapArgs{d_states, d_area, d_out, stride, view->width, view->height, blocks, view->scale, cell, view->flags};
  return RDOOM_OK;
}

}  // namespace

static_assert(sizeof(rdoom_area_grid) == 24, "ABI sizes");

extern "C" {

rdoom_status rdoom_world_area_grid(const rdoom_world *w, float cell, rdoom_area_grid *out) {
  if (!w || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (rdoom_status s = check_cell(cell)) return s;
  return level_grid(rdoom::map_source(w), "world", 0u, cell, *out);
}

rdoom_status rdoom_worldset_level_area_grid(const rdoom_worldset *set, uint32_t slot, float cell, rdoom_area_grid *out) {
  if (!set || !out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  const rdoom::MapSource src = rdoom::map_source(set);
  if (slot >= src.n_levels) return rdoom::fail(RDOOM_BAD_ARG, "slot %u of a set of %u levels", slot, src.n_levels);
  if (rdoom_status s = check_cell(cell)) return s;
  return level_grid(src, "world set", slot, cell, *out);
}

rdoom_status rdoom_world_area_words(const rdoom_world *w, float cell, uint32_t *words_out) {
  if (!w || !words_out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (rdoom_status s = check_cell(cell)) return s;
  return area_words(rdoom::map_source(w), "world", cell, *words_out);
}

rdoom_status rdoom_worldset_area_words(const rdoom_worldset *set, float cell, uint32_t *words_out) {
  if (!set || !words_out) return rdoom::fail(RDOOM_BAD_ARG, "null argument");
  if (rdoom_status s = check_cell(cell)) return s;
  return area_words(rdoom::map_source(set), "world set", cell, *words_out);
}

rdoom_status rdoom_world_reveal_area(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const float *d_dirs, uint32_t n_rays,
                                     float max_range, const float *d_object_offsets, uint32_t n_objects, float cell, uint32_t n_steps,
                                     uint32_t *d_area, uint32_t stride, uint32_t *d_new_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  AreaArgs a;
  if (rdoom_status s = reveal_args(src, "world", d_states, n, d_dirs, n_rays, max_range, d_object_offsets, n_objects, cell, n_steps, d_area, stride,
                                   d_new_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(reveal_area_kernel, dim3(n), dim3(THREADS), 0, stream, a, src.bounds[0], src.map->n_lines);
}

rdoom_status rdoom_worldset_reveal_area(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                        const float *d_dirs, uint32_t n_rays, float max_range, const float *d_object_offsets, uint32_t n_objects,
                                        float cell, uint32_t n_steps, uint32_t *d_area, uint32_t stride, uint32_t *d_new_out, void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  AreaArgs a;
  if (rdoom_status s = reveal_args(src, "world set", d_states, n, d_dirs, n_rays, max_range, d_object_offsets, n_objects, cell, n_steps, d_area,
                                   stride, d_new_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_reveal_area_kernel, dim3(n), dim3(THREADS), 0, stream, a, (const uint2 *)src.map->levels.get(),
                               (const float4 *)src.map->bounds.get(), d_levels, src.map->n_levels);
}

rdoom_status rdoom_world_draw_area_maps(const rdoom_world *w, const rdoom_player_state *d_states, uint32_t n, const rdoom_map_view *view,
                                        const uint32_t *d_area, uint32_t stride, float cell, uint8_t *d_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  AreaMapArgs a;
  if (rdoom_status s = map_args(src, "world", d_states, n, view, d_area, stride, cell, d_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(draw_area_maps_kernel, dim3(n * a.blocks), dim3(THREADS), 0, stream, a, src.bounds[0]);
}

rdoom_status rdoom_worldset_draw_area_maps(const rdoom_worldset *set, const rdoom_player_state *d_states, const uint32_t *d_levels, uint32_t n,
                                           const rdoom_map_view *view, const uint32_t *d_area, uint32_t stride, float cell, uint8_t *d_out,
                                           void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  AreaMapArgs a;
  if (rdoom_status s = map_args(src, "world set", d_states, n, view, d_area, stride, cell, d_out, a)) return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_draw_area_maps_kernel, dim3(n * a.blocks), dim3(THREADS), 0, stream, a, (const float4 *)src.map->bounds.get(),
                               d_levels, src.map->n_levels);
}

}  // extern "C"
