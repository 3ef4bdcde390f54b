// Walking distance to a goal over a whole level (include/rdoom.h "goal distance"): the level's sector, floor and
// ceiling planes on its explored-area grid (rdoom_world_draw_area_planes), the cell of that grid a player stands in
// (rdoom_world_area_cells), their world-set forms, and a flood of grids of any size from a seed or towards it (rdoom_flood_grids,
// rdoom_flood_grid_max_cells).
//
// Arithmetic: binary32, the contract's operations in the contract's order; the build passes -ffp-contract=off.  The grid formulas
// are world_shared.hpp's, the ones area.hip indexes with; the sector at a point is `descend` + `sector_in_leaf` and the heights are
// `live_heights`, the ones sectors.hip uses.
//
// draw_area_planes: one thread per cell, 256 to a workgroup, no LDS.  area_cells: one lane per player.
//
// flood_grids: one 1024-thread workgroup per grid, always in global memory, so a grid of any size takes the same code.  A cell's
// word of d_dist_out holds its distance in the low 28 bits (PENDING: not reached so far) and, while the kernel runs, in the top four
// bits whether the cell may be entered from its left, right, upper, lower neighbour -- for RDOOM_FLOOD_TOWARDS whether the cell may
// be LEFT for that neighbour, which is the same relation followed backwards.  The bits are computed once from the floats; a last
// pass stores the clean distances and counts them.  Between the two, section 20's passes: in the row phase a thread owns runs of
// `seg` cells of a row and carries a distance along each left to right and back; in the column phase runs of a column, down and up;
// a barrier between the phases.  In a phase only a run's owner writes its cells.  What it reads of a neighbouring run -- the one
// cell before and the one after, aligned 32-bit words read and written by relaxed workgroup-scope atomic accesses, so a word is
// never torn -- may be mid-pass: values only fall and every value ever stored is the length of a real path, so any schedule ends
// at the same fixed point, the shortest distances.
// Visibility: the rule relied on is the AMDGPU memory model's for workgroup scope outside threadgroup-split mode.  The waves of a
// workgroup run on one CU and share its vector L1, which takes that CU's vector memory accesses in the order they were issued and
// which every store writes through; so a workgroup-scope release or acquire of global memory needs no cache maintenance and no wait
// on the vector-memory counter, and the compiler emits none: __syncthreads() is that fence pair around s_barrier and comes out as
// a bare s_barrier (with a wait for LDS only).  A word stored by a wave before the barrier was issued to the L1 before any load a
// wave issues after it, so that load reads it.  The relaxed workgroup-scope atomics (sc0 loads and stores) keep every access to a
// cell's word on that path -- the vector L1, never the scalar cache, never a register copy carried across a barrier.  No other
// workgroup touches the grid.
// Termination: the loop condition is one LDS word (two, used alternately) every thread reads between two barriers, so it is
// workgroup-uniform, every thread reaches every barrier, and the `for` has the hard bound cells + 1 -- a pass relaxes every move
// at least once (a Bellman-Ford round), a distance is below the number of cells, so pass number `cells` at the latest changes
// nothing.  A closed or outside seed leaves every cell PENDING: the first pass changes nothing and is the last.  Nothing waits for
// another workgroup: no grid-wide barrier, no spin on global memory, no global read-modify-write.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::AreaCellArgs;
using rdoom_dev::allowed;
using rdoom_dev::AreaPlaneArgs;
using rdoom_dev::descend;
using rdoom_dev::FloodGridArgs;
using rdoom_dev::Grid;
using rdoom_dev::is_open;
using rdoom_dev::grid_of;
using rdoom_dev::live_heights;
using rdoom_dev::point_cell;
using rdoom_dev::sector_in_leaf;
using rdoom_dev::SectorLevel;
using rdoom_dev::SectorTables;
using rdoom_dev::WalkLimits;

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

// ---- the flood ----
constexpr uint32_t THREADS = 1024;
constexpr uint32_t MAX_CELLS = 1u << 22;
constexpr uint32_t DIST_BITS = 28, DIST_MASK = (1u << DIST_BITS) - 1u;
constexpr uint32_t PENDING = DIST_MASK;  // a cell not reached so far, while the kernel runs
constexpr uint32_t FROM_LEFT = 1u << DIST_BITS, FROM_RIGHT = 2u << DIST_BITS, FROM_ABOVE = 4u << DIST_BITS, FROM_BELOW = 8u << DIST_BITS;
constexpr uint32_t MAX_SEG = 64;
constexpr uint32_t BATCH = 8;  // the words of a run loaded side by side before they are walked
static_assert(MAX_CELLS < PENDING && MAX_CELLS <= RDOOM_AREA_MAX_SIDE * RDOOM_AREA_MAX_SIDE, "flood_grids: a distance fits its 28 bits");

// a cell's word, read and written whole
__device__ __forceinline__ uint32_t word_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void word_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// a batch of a run walked in one direction: words w[0 .. m) of cells at, at + step, ..., the distance of the cell before them in
// `carry`
template <uint32_t BIT>
__device__ __forceinline__ bool walk(uint32_t *dist, const uint32_t (&w)[BATCH], uint32_t m, uint32_t at, int32_t step, uint32_t &carry) {
  bool fell = false;
#pragma unroll
  for (uint32_t j = 0; j < BATCH; j++) {
    if (j < m) {
      uint32_t d = w[j] & DIST_MASK;
      if ((w[j] & BIT) && carry + 1u < d) {
        d = carry + 1u;
        word_store(dist + (at + (int32_t)j * step), (w[j] & ~DIST_MASK) | d);
        fell = true;
      }
      carry = d;
    }
  }
  return fell;
}

// One run: cells base + k * stride, k < len, forwards with the distance of the cell before the run (if there is one) carried in
// through the FWD bits, then backwards from the cell after it through the BWD bits.  True when a distance fell.
template <uint32_t FWD, uint32_t BWD>
__device__ __forceinline__ bool sweep(uint32_t *dist, uint32_t base, uint32_t stride, uint32_t len, bool before, bool after) {
  bool fell = false;
  uint32_t carry = before ? word_load(dist + (base - stride)) & DIST_MASK : PENDING;
  for (uint32_t k0 = 0; k0 < len; k0 += BATCH) {
    const uint32_t m = min(BATCH, len - k0), at = base + k0 * stride;
    uint32_t w[BATCH];
#pragma unroll
    for (uint32_t j = 0; j < BATCH; j++) w[j] = j < m ? word_load(dist + (at + j * stride)) : 0u;
    fell |= walk<FWD>(dist, w, m, at, (int32_t)stride, carry);
  }
  const uint32_t last = base + (len - 1u) * stride;
  carry = after ? word_load(dist + (last + stride)) & DIST_MASK : PENDING;
  for (uint32_t k0 = 0; k0 < len; k0 += BATCH) {
    const uint32_t m = min(BATCH, len - k0), at = last - k0 * stride;
    uint32_t w[BATCH];
#pragma unroll
    for (uint32_t j = 0; j < BATCH; j++) w[j] = j < m ? word_load(dist + (at - j * stride)) : 0u;
    fell |= walk<BWD>(dist, w, m, at, -(int32_t)stride, carry);
  }
  return fell;
}

__global__ __launch_bounds__(THREADS) void flood_grids_kernel(FloodGridArgs a) {
  __shared__ uint32_t changed[2];
  __shared__ uint32_t wave_count[THREADS / WAVE];

  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  const uint32_t W = a.width, H = a.height, cells = a.cells;
  const size_t grid = (size_t)p * cells;
  const float *floor = a.floor + grid, *ceiling = a.ceiling + grid;
  uint32_t *dist = a.dist_out + grid;

  uint32_t seed = 0xFFFFFFFFu;  // outside the grid: no cell
  {
    const int32_t sc = a.seeds ? a.seeds[2 * (size_t)p] : (int32_t)(W / 2u);
    const int32_t sr = a.seeds ? a.seeds[2 * (size_t)p + 1] : (int32_t)(H / 2u);
    if ((uint32_t)sc < W && (uint32_t)sr < H) seed = (uint32_t)sr * W + (uint32_t)sc;
  }

  // staging: the four move bits of every cell, the seed's 0.  Forwards a bit says the neighbour's move INTO the cell is allowed,
  // towards the seed that the cell's move into the neighbour is
  const bool towards = a.towards != 0;  // (a kernel argument: uniform)
  const WalkLimits lim{a.max_step, a.max_drop, a.clearance};
  for (uint32_t i = tid; i < cells; i += THREADS) {
    const uint32_t r = i / W, c = i - r * W;
    const float f = floor[i], g = ceiling[i];
    const bool open = is_open(f, g, lim.clearance);
    uint32_t m = 0;
    if (open) {
      auto move = [&](uint32_t other) { return towards ? allowed(f, g, floor[other], ceiling[other], lim) : allowed(floor[other], ceiling[other], f, g, lim); };
      if (c > 0 && move(i - 1)) m |= FROM_LEFT;
      if (c + 1 < W && move(i + 1)) m |= FROM_RIGHT;
      if (r > 0 && move(i - W)) m |= FROM_ABOVE;
      if (r + 1 < H && move(i + W)) m |= FROM_BELOW;
    }
    word_store(dist + i, m | ((open && i == seed) ? 0u : PENDING));
  }
  if (tid == 0) changed[0] = 0, changed[1] = 0;
  __syncthreads();

  const uint32_t seg = a.seg;
  const uint32_t runs_per_row = (W + seg - 1) / seg, runs_per_column = (H + seg - 1) / seg;
  const uint32_t row_runs = H * runs_per_row, column_runs = W * runs_per_column;
  for (uint32_t pass = 0; pass <= cells; pass++) {  // (the hard bound; the flag ends it long before)
    uint32_t *flag = &changed[pass & 1u];
    bool fell = false;
    for (uint32_t run = tid; run < row_runs; run += THREADS) {
      const uint32_t r = run / runs_per_row, c0 = (run - r * runs_per_row) * seg;
      const uint32_t len = min(seg, W - c0);
      fell |= sweep<FROM_LEFT, FROM_RIGHT>(dist, r * W + c0, 1u, len, c0 > 0, c0 + len < W);
    }
    __syncthreads();
    if (tid == 0) changed[(pass + 1u) & 1u] = 0;  // the next pass's: last read before the barrier above
    for (uint32_t run = tid; run < column_runs; run += THREADS) {  // consecutive lanes: consecutive columns
      const uint32_t k = run / W, c = run - k * W, r0 = k * seg;
      const uint32_t len = min(seg, H - r0);
      fell |= sweep<FROM_ABOVE, FROM_BELOW>(dist, r0 * W + c, W, len, r0 > 0, r0 + len < H);
    }
    if (fell) *flag = 1;
    __syncthreads();
    if (*flag == 0) break;  // one word, read by every thread after the barrier: uniform
  }

  // out: the clean distances, a thread the words it staged; the count by shuffles, then across the waves through LDS
  uint32_t reached = 0;
  for (uint32_t i = tid; i < cells; i += THREADS) {
    const uint32_t d = word_load(dist + i) & DIST_MASK;
    word_store(dist + i, d == PENDING ? RDOOM_FLOOD_GRID_UNREACHED : d);
    reached += d != PENDING;
  }
  if (a.count_out) {  // (a kernel argument: uniform)
    for (uint32_t step = WAVE / 2; step; step >>= 1) reached += __shfl_down(reached, step, WAVE);
    if ((tid & (WAVE - 1)) == 0) wave_count[tid / WAVE] = reached;
    __syncthreads();
    if (tid == 0) {
      uint32_t total = 0;
      for (uint32_t w = 0; w < THREADS / WAVE; w++) total += wave_count[w];
      a.count_out[p] = total;
    }
  }
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
  if (d_offsets && n_objects < src.game_objects)
    return rdoom::fail(RDOOM_BAD_ARG, "n_objects %u is smaller than the %s's %u objects", n_objects, noun, src.game_objects);
  if (d_area && stride < most.words)
    return rdoom::fail(RDOOM_BAD_ARG, "a stride of %u words is smaller than the %u a plane of the %s's grid takes at cell %g", stride, most.words,
                       noun, (double)cell);
  const rdoom::SectorDevice &d = *src.sectors;
  a = AreaPlaneArgs{d_offsets, d_area, d_sector_out, d_floor_out, d_ceiling_out, d.nodes, d.edges, d.sectors, d.leaves, n_objects, stride,
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

// what rdoom_flood_grids and rdoom_flood_descend (path.hip) check of the arguments they share
rdoom_status rdoom::check_flood_grids(const rdoom_flood_params *params, uint32_t n, bool pointers, const char *missing, uint32_t width,
                                      uint32_t height) {
  const auto bad_limit = [](float v) { return !(v >= 0.0f); };  // a NaN or negative
  if (!params) return rdoom::fail(RDOOM_BAD_ARG, "null params");
  if (n && !pointers) return rdoom::fail(RDOOM_BAD_ARG, "null %s with n = %u", missing, n);
  if (!width || !height) return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells (at least 1 a side)", width, height);
  if (width > RDOOM_AREA_MAX_SIDE || height > RDOOM_AREA_MAX_SIDE)
    return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells: a side is at most %u", width, height, RDOOM_AREA_MAX_SIDE);
  if ((uint64_t)width * height > MAX_CELLS)
    return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells: too many (at most %u)", width, height, MAX_CELLS);
  if (params->flags & ~RDOOM_FLOOD_TOWARDS) return rdoom::fail(RDOOM_BAD_ARG, "flood flags 0x%x: 0 or RDOOM_FLOOD_TOWARDS", params->flags);
  if (bad_limit(params->max_step)) return rdoom::fail(RDOOM_BAD_ARG, "max_step %g is a NaN or negative", (double)params->max_step);
  if (bad_limit(params->max_drop)) return rdoom::fail(RDOOM_BAD_ARG, "max_drop %g is a NaN or negative", (double)params->max_drop);
  if (bad_limit(params->clearance)) return rdoom::fail(RDOOM_BAD_ARG, "clearance %g is a NaN or negative", (double)params->clearance);
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u grids: too many for one launch", n);
  return RDOOM_OK;
}

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
                               (const float4 *)src.map->bounds, (const uint4 *)src.sectors->levels, d_levels, src.n_levels);
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
                               (const float4 *)src.map->bounds, d_levels, src.n_levels);
}

rdoom_status rdoom_flood_grid_max_cells(uint32_t *cells_out) {
  if (!cells_out) return rdoom::fail(RDOOM_BAD_ARG, "null cells_out");
  *cells_out = MAX_CELLS;
  return RDOOM_OK;
}

rdoom_status rdoom_flood_grids(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height, const int32_t *d_seeds,
                               const rdoom_flood_params *params, uint32_t *d_dist_out, uint32_t *d_count_out, void *stream) {
  if (rdoom_status s = rdoom::check_flood_grids(params, n, d_floor && d_ceiling && d_dist_out, "floor, ceiling or distance output", width, height)) return s;
  if (!n) return RDOOM_OK;
  const uint32_t cells = width * height;
  // the shortest runs that give every thread at most one run of a phase, where the grid's shape allows that
  uint32_t seg = 2;
  while (seg < MAX_SEG && ((uint64_t)height * ((width + seg - 1) / seg) > THREADS || (uint64_t)width * ((height + seg - 1) / seg) > THREADS)) seg++;
  const FloodGridArgs a{d_floor, d_ceiling, d_seeds, d_dist_out, d_count_out, width, height, cells, seg, params->flags & RDOOM_FLOOD_TOWARDS,
                        params->max_step, params->max_drop, params->clearance};
  return rdoom::launch_checked(flood_grids_kernel, dim3(n), dim3(THREADS), 0, stream, a);
}

}  // extern "C"
