// Waypoints and frontiers (include/rdoom.h "waypoints and frontiers"): a flood's distance field walked downhill
// from a start (rdoom_flood_descend; down an octile field, include/rdoom.h "octile distance" and DESIGN section 26,
// rdoom_flood_descend_octile), and the frontier of every player's explored area with its nearest cell
// (rdoom_world_area_frontiers, rdoom_worldset_area_frontiers).
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off.  The grid formulas
// and the open and move comparisons are world_shared.hpp's, the ones flood.hip floods with.  Costs and distances are integers.
//
// flood_descend: one wavefront per row, four rows to a 256-thread workgroup.  Lanes 0 .. 3 (octile: 0 .. 7) each test one
// neighbour of the current cell, in the contract's order: its distance, the two cells' floors and ceilings, the comparisons -- for
// a diagonal the four axial moves through the two cells between them.  A ballot's lowest set bit is the contract's first
// qualifying neighbour, one scalar for the whole wave, so the walk's state -- the cell, its distance, the moves made -- is
// wave-uniform.
// Termination: the loop's bound is computed before the loop as min(max_moves, D(start) - stop_dist); every iteration makes one
// move to a cell whose distance is one less (octile: at least one less, a cost is at least 1), or breaks.  No barrier, no LDS, no
// atomic; nothing waits on anything.
//
// area_frontiers: one 1024-thread workgroup per row.  A thread takes a 32-cell word of the bit planes at a time: the cells with an
// unknown neighbour come from the FREE and WALL words of the row above, the row itself and the row below, the shifts carrying in
// the neighbouring word's edge bit, everything masked to the level's gw x gh; distances are loaded only where that mask has a bit.
// The nearest frontier cell is the minimum of the 64-bit key D << 32 | iz * width + ix, taken per wave by shuffles and across the
// sixteen waves through LDS.  The kernel writes every output word itself: no global read-modify-write, no initialisation pass.
// Termination: the loops run over the row's words, a count fixed by the arguments; the one barrier is reached by every thread.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::allowed;
using rdoom_dev::DescendArgs;
using rdoom_dev::DescendOctileArgs;
using rdoom_dev::FrontierArgs;
using rdoom_dev::Grid;
using rdoom_dev::grid_of;
using rdoom_dev::WalkLimits;

constexpr uint32_t WAVE = 64;
constexpr uint32_t UNREACHED = RDOOM_FLOOD_GRID_UNREACHED;

// ---- the walk down a field ----
constexpr uint32_t DESCEND_THREADS = 256, DESCEND_ROWS = DESCEND_THREADS / WAVE;
constexpr uint32_t MAX_PATH = 1u << 22;

// neighbour k's offset, in the contract's order: 0 .. 3 are (column - 1, column + 1, row - 1, row + 1), and with OCTILE 4 .. 7 the
// offsets (-1, -1), (+1, -1), (-1, +1), (+1, +1)
template <bool OCTILE>
__device__ __forceinline__ int32_t column_step(uint32_t k) {
  return OCTILE && k >= 4 ? ((k & 1u) ? 1 : -1) : (k == 0 ? -1 : (k == 1 ? 1 : 0));
}
template <bool OCTILE>
__device__ __forceinline__ int32_t row_step(uint32_t k) {
  return OCTILE && k >= 4 ? ((k & 2u) ? 1 : -1) : (k == 2 ? -1 : (k == 3 ? 1 : 0));
}

// the wave's row walked.  Without OCTILE a move costs 1 and `axial` is the literal; stop_dist is in cost units
template <bool TOWARDS, bool OCTILE>
__device__ __forceinline__ void descend_row(const DescendArgs &a, uint32_t axial, uint32_t diagonal) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t p = blockIdx.x * DESCEND_ROWS + threadIdx.x / WAVE;  // the wave's row
  if (p >= a.n) return;
  const uint32_t W = a.width, H = a.height;
  const size_t grid = (size_t)p * W * H;
  const float *floor = a.floor + grid, *ceiling = a.ceiling + grid;
  const uint32_t *dist = a.dist + grid;
  int32_t *path = a.path_out ? a.path_out + (size_t)p * a.path_len * 2 : nullptr;  // (column, row) pairs, 4-byte aligned as the ABI says
  const WalkLimits lim{a.max_step, a.max_drop, a.clearance};

  int32_t col = a.starts[2 * (size_t)p], row = a.starts[2 * (size_t)p + 1];
  const bool inside = (uint32_t)col < W && (uint32_t)row < H;
  uint32_t d = inside ? dist[(uint32_t)row * W + (uint32_t)col] : UNREACHED;
  uint32_t m = 0;
  if (d == UNREACHED) col = -1, row = -1;
  else {
    const int32_t dc = column_step<OCTILE>(lane), dr = row_step<OCTILE>(lane);  // the neighbour this lane tests
    const uint32_t cost = OCTILE && lane >= 4 ? diagonal : axial;               // and what the move to it costs
    const uint32_t bound = d > a.stop_dist ? min(a.max_moves, d - a.stop_dist) : 0u;
    for (; m < bound && (!OCTILE || d > a.stop_dist); m++) {  // (a move that costs 1: the bound says it all)
      bool ok = false;
      const uint32_t bc = (uint32_t)(col + dc), br = (uint32_t)(row + dr);  // (outside: far above W, H)
      if (lane < (OCTILE ? 8u : 4u) && bc < W && br < H) {
        const uint32_t at = (uint32_t)row * W + (uint32_t)col, b = br * W + bc;
        const uint32_t db = dist[b];
        if constexpr (!OCTILE) {  // (its own expression, not the one below with a cost of 1: that one compiles to more)
          const float fa = floor[at], ga = ceiling[at], fb = floor[b], gb = ceiling[b];
          ok = db == d - 1u && (TOWARDS ? allowed(fa, ga, fb, gb, lim) : allowed(fb, gb, fa, ga, lim));
        } else if (db <= d && d - db == cost) {  // D(b) + cost == D(a), in integers: an unreached b is above every D(a) walked from
          // the move of the field's relation between cells x and y, y the one nearer the seed
          auto move = [&](uint32_t x, uint32_t y) {
            return TOWARDS ? allowed(floor[x], ceiling[x], floor[y], ceiling[y], lim) : allowed(floor[y], ceiling[y], floor[x], ceiling[x], lim);
          };
          if (lane < 4) ok = move(at, b);
          else {
            const uint32_t s1 = (uint32_t)row * W + bc, s2 = br * W + (uint32_t)col;  // inside the grid with a and b
            ok = move(at, s1) && move(s1, b) && move(at, s2) && move(s2, b);
          }
        }
      }
      const uint64_t qualify = __builtin_amdgcn_ballot_w64(ok);
      if (qualify == 0) break;  // (only on a field that was not flooded from these planes)
      const uint32_t k = (uint32_t)__builtin_ctzll(qualify);
      col += column_step<OCTILE>(k), row += row_step<OCTILE>(k);
      d -= OCTILE && k >= 4 ? diagonal : axial;
      if (path && lane == 0 && m < a.path_len) path[2 * (size_t)m] = col, path[2 * (size_t)m + 1] = row;
    }
  }
  if (lane == 0) {
    a.cells_out[2 * (size_t)p] = col, a.cells_out[2 * (size_t)p + 1] = row;
    a.moves_out[p] = m;
  }
  if (path)  // the entries no move filled: words 2 * min(m, path_len) on, disjoint from the ones lane 0 stored in the loop
    for (size_t k = 2 * (size_t)min(m, a.path_len) + lane; k < 2 * (size_t)a.path_len; k += WAVE) path[k] = -1;  // a lane a word
}

__global__ __launch_bounds__(DESCEND_THREADS) void flood_descend_kernel(DescendArgs a) { descend_row<false, false>(a, 1u, 1u); }
__global__ __launch_bounds__(DESCEND_THREADS) void flood_descend_towards_kernel(DescendArgs a) { descend_row<true, false>(a, 1u, 1u); }
__global__ __launch_bounds__(DESCEND_THREADS) void flood_descend_octile_kernel(DescendOctileArgs a) {
  descend_row<false, true>(a, a.axial_cost, a.diagonal_cost);
}
__global__ __launch_bounds__(DESCEND_THREADS) void flood_descend_octile_towards_kernel(DescendOctileArgs a) {
  descend_row<true, true>(a, a.axial_cost, a.diagonal_cost);
}

// ---- the frontier of an explored area ----
constexpr uint32_t THREADS = 1024;
constexpr uint64_t NO_KEY = ~0ull;

// the cells of word wx of grid row iz that are unknown in `rows` (FREE plane, WALL plane `stride` words on) and inside the grid;
// a word outside the grid has none.  (iz, wx: modulo 2^32, so -1 is outside)
__device__ __forceinline__ uint32_t unknown_word(const uint32_t *rows, uint32_t stride, const Grid &g, uint32_t iz, uint32_t wx) {
  if (iz >= g.gh || wx >= g.pitch) return 0u;
  const uint32_t at = iz * g.pitch + wx;  // < the level's words <= stride
  const uint32_t left = g.gw - wx * 32u;  // the cells of the grid row from this word on: >= 1
  return ~(rows[at] | rows[stride + at]) & (left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u);
}

// row p's frontier in grid g; in_set false: none
__device__ __forceinline__ void frontier_row(const FrontierArgs &a, uint32_t p, const Grid &g, bool in_set) {
  __shared__ uint64_t wave_key[THREADS / WAVE];
  __shared__ uint32_t wave_count[THREADS / WAVE];

  const uint32_t tid = threadIdx.x;
  const uint32_t W = a.width, H = a.height;
  const size_t plane = (size_t)p * W * H;
  const uint32_t *rows = a.area + (size_t)p * 2 * a.stride;
  const uint32_t *dist = a.dist + plane;
  uint8_t *mask = a.mask_out ? a.mask_out + plane : nullptr;

  uint64_t key = NO_KEY;
  uint32_t count = 0;
  // the words of the padded extent when a mask is written (it is written in full), else those of the grid
  const uint32_t words_x = mask ? (W + 31u) / 32u : (in_set ? g.pitch : 0u), words_z = mask ? H : (in_set ? g.gh : 0u);
  for (uint32_t w = tid; w < words_x * words_z; w += THREADS) {
    const uint32_t iz = w / words_x, wx = w - iz * words_x;
    uint32_t front = 0;
    if (in_set && iz < g.gh && wx < g.pitch) {
      const uint32_t here = unknown_word(rows, a.stride, g, iz, wx);
      const uint32_t near = (here << 1) | (unknown_word(rows, a.stride, g, iz, wx - 1u) >> 31) | (here >> 1) |
                            (unknown_word(rows, a.stride, g, iz, wx + 1u) << 31) | unknown_word(rows, a.stride, g, iz - 1u, wx) |
                            unknown_word(rows, a.stride, g, iz + 1u, wx);
      const uint32_t left = g.gw - wx * 32u;
      const uint32_t cand = near & (left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u);
      const uint32_t base = iz * W + wx * 32u;  // a set bit j is cell wx * 32 + j < gw <= W
#pragma unroll
      for (uint32_t j0 = 0; j0 < 32u; j0 += 4u) {
        const uint32_t four = (cand >> j0) & 15u;
        if (four == 0) continue;
        uint32_t d[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) d[j] = (four >> j) & 1u ? dist[base + j0 + j] : UNREACHED;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++)
          if (d[j] != UNREACHED) {
            front |= 1u << (j0 + j);
            const uint64_t k = (uint64_t)d[j] << 32 | (base + j0 + j);
            key = k < key ? k : key;
          }
      }
      count += __popc(front);
    }
    if (mask) {
      const uint32_t ix0 = wx * 32u;
      uint8_t *out = mask + (size_t)iz * W + ix0;
      const bool aligned = ((uintptr_t)out & 3u) == 0;
#pragma unroll
      for (uint32_t j0 = 0; j0 < 32u; j0 += 4u) {
        const uint32_t four = (front >> j0) & 15u;
        if (aligned && ix0 + j0 + 4u <= W) {  // four bytes at once
          *(uint32_t *)(out + j0) = (four & 1u) | (four & 2u) << 7 | (four & 4u) << 14 | (four & 8u) << 21;
        } else {
#pragma unroll
          for (uint32_t j = 0; j < 4u; j++)
            if (ix0 + j0 + j < W) out[j0 + j] = (uint8_t)((four >> j) & 1u);
        }
      }
    }
  }

  // the smallest key and the sum of the counts: per wave by shuffles, then across the waves through LDS
  for (uint32_t step = WAVE / 2; step; step >>= 1) {
    const uint64_t other = __shfl_down(key, step, WAVE);
    key = other < key ? other : key;
    count += __shfl_down(count, step, WAVE);
  }
  if ((tid & (WAVE - 1)) == 0) wave_key[tid / WAVE] = key, wave_count[tid / WAVE] = count;
  __syncthreads();
  if (tid == 0) {
    uint64_t best = NO_KEY;
    uint32_t total = 0;
    for (uint32_t w = 0; w < THREADS / WAVE; w++) {
      best = wave_key[w] < best ? wave_key[w] : best;
      total += wave_count[w];
    }
    const bool none = best == NO_KEY;
    const uint32_t at = (uint32_t)best;  // iz * width + ix
    a.cell_out[2 * (size_t)p] = none ? -1 : (int32_t)(at % W), a.cell_out[2 * (size_t)p + 1] = none ? -1 : (int32_t)(at / W);
    if (a.dist_out) a.dist_out[p] = none ? UNREACHED : (uint32_t)(best >> 32);
    if (a.count_out) a.count_out[p] = total;
  }
}

__global__ __launch_bounds__(THREADS) void area_frontiers_kernel(FrontierArgs a, float4 bounds) {
  Grid g;
  grid_of(bounds, a.cell, g);
  frontier_row(a, blockIdx.x, g, true);
}

// the world set's: row p is on level level_of[p]; a slot outside the set has no frontier
__global__ __launch_bounds__(THREADS) void worldset_area_frontiers_kernel(FrontierArgs a, const float4 *__restrict__ bounds,
                                                                          const uint32_t *__restrict__ level_of, uint32_t n_levels) {
  const uint32_t slot = level_of[blockIdx.x];
  const bool in_set = slot < n_levels;
  Grid g{};
  if (in_set) grid_of(bounds[slot], a.cell, g);
  frontier_row(a, blockIdx.x, g, in_set);
}

// ---- the host's side ----
// what both walks check of the path, and the arguments they share as the kernels take them
rdoom_status descend_args(const float *d_floor, const float *d_ceiling, const uint32_t *d_dist, uint32_t n, uint32_t width, uint32_t height,
                          const int32_t *d_starts, float max_step, float max_drop, float clearance, uint32_t max_moves, uint32_t stop_dist,
                          int32_t *d_cells_out, uint32_t *d_moves_out, int32_t *d_path_out, uint32_t path_len, DescendArgs &a) {
  if (d_path_out && (path_len == 0 || path_len > MAX_PATH))
    return rdoom::fail(RDOOM_BAD_ARG, "a path of %u entries: 1 to %u", path_len, MAX_PATH);
  a = DescendArgs{d_floor, d_ceiling, d_dist, d_starts, d_cells_out, d_moves_out, d_path_out, n, width, height, d_path_out ? path_len : 0u,
                  max_moves, stop_dist, max_step, max_drop, clearance};
  return RDOOM_OK;
}

// the arguments of a frontier call, checked, as the kernel takes them.  noun: "world" or "world set"
rdoom_status frontier_args(const rdoom::MapSource &src, const rdoom_world *w, const rdoom_worldset *set, const char *noun, uint32_t n, float cell,
                           uint32_t width, uint32_t height, const uint32_t *d_area, uint32_t stride, const uint32_t *d_dist, int32_t *d_cell_out,
                           uint32_t *d_dist_out, uint32_t *d_count_out, uint8_t *d_mask_out, FrontierArgs &a) {
  if (n && (!d_area || !d_dist || !d_cell_out)) return rdoom::fail(RDOOM_BAD_ARG, "null area, distances or cell output with n = %u", n);
  rdoom_area_grid most;
  if (rdoom_status s = rdoom::handle_grid(w, set, src.n_levels, cell, most)) return s;
  if (width < most.gw || height < most.gh || width > RDOOM_AREA_MAX_SIDE || height > RDOOM_AREA_MAX_SIDE)
    return rdoom::fail(RDOOM_BAD_ARG, "distances of %u x %u cells: the %s's grid at cell %g takes %u x %u, a side is at most %u", width, height, noun,
                       (double)cell, most.gw, most.gh, RDOOM_AREA_MAX_SIDE);
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u rows: too many for one launch", n);
  if (stride < most.words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a plane of the %s's grid takes at cell %g", stride, most.words,
                       noun, (double)cell);
  a = FrontierArgs{d_area, d_dist, d_cell_out, d_dist_out, d_count_out, d_mask_out, stride, width, height, cell};
  return RDOOM_OK;
}

}  // namespace

extern "C" {

rdoom_status rdoom_flood_descend(const float *d_floor, const float *d_ceiling, const uint32_t *d_dist, uint32_t n, uint32_t width,
                                 uint32_t height, const int32_t *d_starts, const rdoom_flood_params *params, uint32_t max_moves,
                                 uint32_t stop_dist, int32_t *d_cells_out, uint32_t *d_moves_out, int32_t *d_path_out, uint32_t path_len,
                                 void *stream) {
  if (rdoom_status s = rdoom::check_flood_grids(params, n, d_floor && d_ceiling && d_dist && d_starts && d_cells_out && d_moves_out,
                                                "floor, ceiling, distances, starts, cell output or move output", width, height))
    return s;
  DescendArgs a;
  if (rdoom_status s = descend_args(d_floor, d_ceiling, d_dist, n, width, height, d_starts, params->max_step, params->max_drop, params->clearance,
                                    max_moves, stop_dist, d_cells_out, d_moves_out, d_path_out, path_len, a))
    return s;
  if (!n) return RDOOM_OK;
  const dim3 blocks((n + DESCEND_ROWS - 1) / DESCEND_ROWS);
  if (params->flags & RDOOM_FLOOD_TOWARDS) return rdoom::launch_checked(flood_descend_towards_kernel, blocks, dim3(DESCEND_THREADS), 0, stream, a);
  return rdoom::launch_checked(flood_descend_kernel, blocks, dim3(DESCEND_THREADS), 0, stream, a);
}

rdoom_status rdoom_flood_descend_octile(const float *d_floor, const float *d_ceiling, const uint32_t *d_dist, uint32_t n, uint32_t width,
                                        uint32_t height, const int32_t *d_starts, const rdoom_flood_octile_params *params,
                                        uint32_t max_moves, uint32_t stop_dist, int32_t *d_cells_out, uint32_t *d_moves_out,
                                        int32_t *d_path_out, uint32_t path_len, void *stream) {
  if (rdoom_status s = rdoom::check_flood_octile(params, n, d_floor && d_ceiling && d_dist && d_starts && d_cells_out && d_moves_out,
                                                 "floor, ceiling, distances, starts, cell output or move output", width, height))
    return s;
  DescendOctileArgs a{{}, params->axial_cost, params->diagonal_cost};
  if (rdoom_status s = descend_args(d_floor, d_ceiling, d_dist, n, width, height, d_starts, params->max_step, params->max_drop, params->clearance,
                                    max_moves, stop_dist, d_cells_out, d_moves_out, d_path_out, path_len, a))
    return s;
  if (!n) return RDOOM_OK;
  const dim3 blocks((n + DESCEND_ROWS - 1) / DESCEND_ROWS);
  if (params->flags & RDOOM_FLOOD_TOWARDS)
    return rdoom::launch_checked(flood_descend_octile_towards_kernel, blocks, dim3(DESCEND_THREADS), 0, stream, a);
  return rdoom::launch_checked(flood_descend_octile_kernel, blocks, dim3(DESCEND_THREADS), 0, stream, a);
}

rdoom_status rdoom_world_area_frontiers(const rdoom_world *w, uint32_t n, float cell, uint32_t width, uint32_t height, const uint32_t *d_area,
                                        uint32_t area_stride, const uint32_t *d_dist, int32_t *d_cell_out, uint32_t *d_dist_out,
                                        uint32_t *d_count_out, uint8_t *d_mask_out, void *stream) {
  if (!w) return rdoom::fail(RDOOM_BAD_ARG, "null world");
  const rdoom::MapSource src = rdoom::map_source(w);
  FrontierArgs a;
  if (rdoom_status s = frontier_args(src, w, nullptr, "world", n, cell, width, height, d_area, area_stride, d_dist, d_cell_out, d_dist_out,
                                     d_count_out, d_mask_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(area_frontiers_kernel, dim3(n), dim3(THREADS), 0, stream, a, src.bounds[0]);
}

rdoom_status rdoom_worldset_area_frontiers(const rdoom_worldset *set, const uint32_t *d_levels, uint32_t n, float cell, uint32_t width,
                                           uint32_t height, const uint32_t *d_area, uint32_t area_stride, const uint32_t *d_dist,
                                           int32_t *d_cell_out, uint32_t *d_dist_out, uint32_t *d_count_out, uint8_t *d_mask_out,
                                           void *stream) {
  if (!set) return rdoom::fail(RDOOM_BAD_ARG, "null world set");
  if (n && !d_levels) return rdoom::fail(RDOOM_BAD_ARG, "null levels with n = %u", n);
  const rdoom::MapSource src = rdoom::map_source(set);
  FrontierArgs a;
  if (rdoom_status s = frontier_args(src, nullptr, set, "world set", n, cell, width, height, d_area, area_stride, d_dist, d_cell_out, d_dist_out,
                                     d_count_out, d_mask_out, a))
    return s;
  if (rdoom_status s = rdoom::check_device(&src, "the world set")) return s;
  if (!n) return RDOOM_OK;
  return rdoom::launch_checked(worldset_area_frontiers_kernel, dim3(n), dim3(THREADS), 0, stream, a, (const float4 *)src.map->bounds.get(), d_levels,
                               src.n_levels);
}

}  // extern "C"
