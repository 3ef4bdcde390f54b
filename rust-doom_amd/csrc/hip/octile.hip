// Octile walking distance (include/rdoom.h "octile distance"): grids flooded over moves to the eight neighbours,
// an axial move costing axial_cost and a diagonal one diagonal_cost (rdoom_flood_grids_octile), and the walk down such a field
// (rdoom_flood_descend_octile).  They read floor and ceiling planes and nothing else: no world handle, no table.
//
// Arithmetic: binary32, the contract's comparisons in the contract's order; the build passes -ffp-contract=off.  The open and move
// comparisons are world_shared.hpp's, the ones flood.hip floods with and path.hip walks with.  Costs and distances are integers.
//
// flood_octile_kernel: flood_grids_kernel's shape (flood.hip) with two more phases a pass.  One 1024-thread
// workgroup per grid; a cell's word of d_dist_out holds its distance in the low 24 bits and, while the kernel runs, its eight move
// bits in the top byte.  A word is read and written whole by relaxed workgroup-scope atomic accesses; flood.hip's note on
// visibility ("the global store") holds here word for word.
//
// flood_descend_octile: path.hip's walk, one wavefront per row; lanes 0 .. 7 each test one neighbour.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::allowed;
using rdoom_dev::DescendOctileArgs;
using rdoom_dev::FloodOctileArgs;
using rdoom_dev::is_open;
using rdoom_dev::WalkLimits;

constexpr uint32_t WAVE = 64, THREADS = 1024;
constexpr uint32_t UNREACHED = RDOOM_FLOOD_GRID_UNREACHED;

// ---- a cell's word ----
constexpr uint32_t DIST_BITS = 24, DIST_MASK = (1u << DIST_BITS) - 1u;
constexpr uint32_t PENDING = DIST_MASK;  // a cell not reached so far, while the kernel runs
// the cell may be entered from the neighbour at (column - 1, row), (column + 1, row), (column, row - 1), (column, row + 1) ...
constexpr uint32_t FROM_LEFT = 1u << DIST_BITS, FROM_RIGHT = 2u << DIST_BITS, FROM_ABOVE = 4u << DIST_BITS, FROM_BELOW = 8u << DIST_BITS;
// ... and from (column - 1, row - 1), (column + 1, row + 1), (column + 1, row - 1), (column - 1, row + 1)
constexpr uint32_t FROM_UP_LEFT = 16u << DIST_BITS, FROM_DOWN_RIGHT = 32u << DIST_BITS, FROM_UP_RIGHT = 64u << DIST_BITS,
                   FROM_DOWN_LEFT = 128u << DIST_BITS;
constexpr uint32_t BATCH = 8;  // the words of a run loaded side by side before they are walked

__device__ __forceinline__ uint32_t word_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void word_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// a batch of a run walked in one direction: words w[0 .. m) of cells at, at + step, ..., the distance of the cell before them in
// `carry`.  carry + cost does not wrap: carry <= PENDING < 2^24 and cost < 2^25; from PENDING it is never below a distance
template <uint32_t BIT>
__device__ __forceinline__ bool walk(uint32_t *dist, const uint32_t (&w)[BATCH], uint32_t m, uint32_t at, int32_t step, uint32_t cost,
                                     uint32_t &carry) {
  bool fell = false;
#pragma unroll
  for (uint32_t j = 0; j < BATCH; j++) {
    if (j < m) {
      uint32_t d = w[j] & DIST_MASK;
      if ((w[j] & BIT) && carry + cost < d) {
        d = carry + cost;
        word_store(dist + (at + (int32_t)j * step), (w[j] & ~DIST_MASK) | d);
        fell = true;
      }
      carry = d;
    }
  }
  return fell;
}

// the run of cells base + k * stride, k < len: forwards with the distance of the cell before the run, if there is one, carried in
// through the FWD bits, then backwards from the cell after it through the BWD bits; every move costs `cost`.  True when a distance
// fell.  (len >= 1; with len == 1 the stride may be 0)
template <uint32_t FWD, uint32_t BWD>
__device__ __forceinline__ bool sweep(uint32_t *dist, uint32_t base, uint32_t stride, uint32_t len, bool before, bool after, uint32_t cost) {
  bool fell = false;
  uint32_t carry = before ? word_load(dist + (base - stride)) & DIST_MASK : PENDING;
  for (uint32_t k0 = 0; k0 < len; k0 += BATCH) {
    const uint32_t m = min(BATCH, len - k0), at = base + k0 * stride;
    uint32_t w[BATCH];
#pragma unroll
    for (uint32_t j = 0; j < BATCH; j++) w[j] = j < m ? word_load(dist + (at + j * stride)) : 0u;
    fell |= walk<FWD>(dist, w, m, at, (int32_t)stride, cost, carry);
  }
  const uint32_t last = base + (len - 1u) * stride;
  carry = after ? word_load(dist + (last + stride)) & DIST_MASK : PENDING;
  for (uint32_t k0 = 0; k0 < len; k0 += BATCH) {
    const uint32_t m = min(BATCH, len - k0), at = last - k0 * stride;
    uint32_t w[BATCH];
#pragma unroll
    for (uint32_t j = 0; j < BATCH; j++) w[j] = j < m ? word_load(dist + (at - j * stride)) : 0u;
    fell |= walk<BWD>(dist, w, m, at, -(int32_t)stride, cost, carry);
  }
  return fell;
}

// ---- the flood: grid blockIdx.x.  Staging is two steps with a barrier between them: the four axial move bits of every cell from
// the floats, exactly as flood.hip stages them (`towards`: the cell may be LEFT for that neighbour), with the seed's 0; then the
// four diagonal bits from the axial bits of the cell and of the two cells between it and the diagonal neighbour -- the contract's
// rule, the same formula in either direction because the axial bits are already those of the relation that is followed.  A thread
// rewrites the words it staged; what it reads of other words are their axial bits, which no one changes.
// Then passes until one changes nothing.  A pass is four phases with a barrier after each: rows, columns (runs of `seg` cells, as
// in flood.hip), then the runs of stride width + 1 and those of stride width - 1.  A diagonal run is the part of one diagonal
// inside a band of `seg` grid rows; run j of band r0 is the diagonal column - row == j - (r0 + seg - 1), the anti-diagonal
// column + row == r0 + j, j < width + seg - 1: every diagonal that meets the band, consecutive lanes on consecutive columns.  In a
// phase only a run's owner writes its cells; what it reads of another run (the one cell before and the one after, never torn)
// may be mid-pass -- values only fall and every value ever stored is the cost of a real path, so any schedule ends at the same
// fixed point, the cheapest costs.
// Termination: the loop condition is one LDS word (two, used alternately) every thread reads between two barriers, so it is
// workgroup-uniform; no thread returns early and every thread reaches every barrier; the `for` has the hard bound cells + 1 -- a
// pass relaxes every allowed move, axial and diagonal, at least once (a Bellman-Ford round) and a cheapest path has fewer than
// `cells` moves, so pass number `cells` at the latest changes nothing.  Nothing waits on another workgroup: no grid-wide barrier,
// no spin on global memory, no global read-modify-write ----
__global__ __launch_bounds__(THREADS) void flood_octile_kernel(FloodOctileArgs a) {
  __shared__ uint32_t changed[2];
  __shared__ uint32_t wave_count[THREADS / WAVE];

  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  const uint32_t W = a.width, H = a.height, cells = W * H;
  const float *floor = a.floor + (size_t)p * cells, *ceiling = a.ceiling + (size_t)p * cells;
  uint32_t *dist = a.dist_out + (size_t)p * cells;
  const bool towards = a.towards != 0;  // (a kernel argument: uniform)

  uint32_t seed = 0xFFFFFFFFu;  // outside the grid: no cell
  {
    const int32_t sc = a.seeds ? a.seeds[2 * (size_t)p] : (int32_t)(W / 2u);
    const int32_t sr = a.seeds ? a.seeds[2 * (size_t)p + 1] : (int32_t)(H / 2u);
    if ((uint32_t)sc < W && (uint32_t)sr < H) seed = (uint32_t)sr * W + (uint32_t)sc;
  }

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
    word_store(dist + i, m | (open && i == seed ? 0u : PENDING));
  }
  if (tid == 0) changed[0] = 0, changed[1] = 0;
  __syncthreads();
  for (uint32_t i = tid; i < cells; i += THREADS) {
    const uint32_t w = word_load(dist + i);
    // a bit of the cell towards a side says that side's neighbour is inside the grid, so the cells read below are
    uint32_t m = 0;
    if ((w & (FROM_LEFT | FROM_ABOVE)) == (FROM_LEFT | FROM_ABOVE) && (word_load(dist + (i - W)) & FROM_LEFT) && (word_load(dist + (i - 1)) & FROM_ABOVE))
      m |= FROM_UP_LEFT;
    if ((w & (FROM_RIGHT | FROM_ABOVE)) == (FROM_RIGHT | FROM_ABOVE) && (word_load(dist + (i - W)) & FROM_RIGHT) && (word_load(dist + (i + 1)) & FROM_ABOVE))
      m |= FROM_UP_RIGHT;
    if ((w & (FROM_LEFT | FROM_BELOW)) == (FROM_LEFT | FROM_BELOW) && (word_load(dist + (i + W)) & FROM_LEFT) && (word_load(dist + (i - 1)) & FROM_BELOW))
      m |= FROM_DOWN_LEFT;
    if ((w & (FROM_RIGHT | FROM_BELOW)) == (FROM_RIGHT | FROM_BELOW) && (word_load(dist + (i + W)) & FROM_RIGHT) && (word_load(dist + (i + 1)) & FROM_BELOW))
      m |= FROM_DOWN_RIGHT;
    if (m) word_store(dist + i, w | m);
  }
  __syncthreads();

  const uint32_t seg = a.seg;
  const uint32_t runs_per_row = (W + seg - 1) / seg, bands = (H + seg - 1) / seg;
  const uint32_t row_runs = H * runs_per_row, column_runs = W * bands;
  const uint32_t runs_per_band = W + seg - 1, diagonal_runs = bands * runs_per_band;
  const uint32_t axial = a.axial_cost, diagonal = a.diagonal_cost;
  for (uint32_t pass = 0; pass <= cells; pass++) {  // (the hard bound; the flag ends it long before)
    uint32_t *flag = &changed[pass & 1u];
    bool fell = false;
    for (uint32_t run = tid; run < row_runs; run += THREADS) {
      const uint32_t r = run / runs_per_row, c0 = (run - r * runs_per_row) * seg;
      const uint32_t len = min(seg, W - c0);
      fell |= sweep<FROM_LEFT, FROM_RIGHT>(dist, r * W + c0, 1u, len, c0 > 0, c0 + len < W, axial);
    }
    __syncthreads();
    if (tid == 0) changed[(pass + 1u) & 1u] = 0;  // the next pass's: last read before the barrier above
    for (uint32_t run = tid; run < column_runs; run += THREADS) {  // consecutive lanes: consecutive columns
      const uint32_t k = run / W, c = run - k * W, r0 = k * seg;
      const uint32_t len = min(seg, H - r0);
      fell |= sweep<FROM_ABOVE, FROM_BELOW>(dist, r0 * W + c, W, len, r0 > 0, r0 + len < H, axial);
    }
    __syncthreads();
    for (uint32_t run = tid; run < diagonal_runs; run += THREADS) {  // column - row == k: rows lo .. hi - 1 of the band
      const uint32_t b = run / runs_per_band;
      const int32_t r0 = (int32_t)(b * seg), k = (int32_t)(run - b * runs_per_band) - (r0 + (int32_t)seg - 1);
      const int32_t lo = max(r0, -k), hi = min(min(r0 + (int32_t)seg, (int32_t)H), (int32_t)W - k);
      if (lo < hi)
        fell |= sweep<FROM_UP_LEFT, FROM_DOWN_RIGHT>(dist, (uint32_t)lo * W + (uint32_t)(k + lo), W + 1u, (uint32_t)(hi - lo), lo > 0 && k + lo > 0,
                                                     hi < (int32_t)H && k + hi < (int32_t)W, diagonal);
    }
    __syncthreads();
    for (uint32_t run = tid; run < diagonal_runs; run += THREADS) {  // column + row == k
      const uint32_t b = run / runs_per_band;
      const int32_t r0 = (int32_t)(b * seg), k = r0 + (int32_t)(run - b * runs_per_band);
      const int32_t lo = max(r0, k - ((int32_t)W - 1)), hi = min(min(r0 + (int32_t)seg, (int32_t)H), k + 1);
      if (lo < hi)
        fell |= sweep<FROM_UP_RIGHT, FROM_DOWN_LEFT>(dist, (uint32_t)lo * W + (uint32_t)(k - lo), W - 1u, (uint32_t)(hi - lo),
                                                     lo > 0 && k - lo + 1 < (int32_t)W, hi < (int32_t)H && k - hi >= 0, diagonal);
    }
    if (fell) *flag = 1;
    __syncthreads();
    if (*flag == 0) break;  // one word, read by every thread after the barrier: uniform
  }

  // out: the clean distances in place, a thread the words it staged; the count by shuffles, then across the waves through LDS
  uint32_t reached = 0;
  for (uint32_t i = tid; i < cells; i += THREADS) {
    const uint32_t d = word_load(dist + i) & DIST_MASK;
    word_store(dist + i, d == PENDING ? UNREACHED : d);
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

// ---- the walk down an octile field: one wavefront per row, four rows to a 256-thread workgroup.  Lanes 0 .. 7 each test one
// neighbour b of the current cell a, in the contract's order: its distance, then the move between the two -- for a diagonal the
// four axial moves through the two cells between them, from the floats.  A ballot's lowest set bit is the contract's first
// qualifying neighbour, one scalar for the whole wave, so the walk's state is wave-uniform.
// Termination: the loop's bound is computed before the loop as min(max_moves, D(start) - stop_dist); every iteration makes one
// move to a cell whose distance is at least 1 less (a cost is at least 1), or breaks.  No barrier, no LDS, no atomic ----
constexpr uint32_t DESCEND_THREADS = 256, DESCEND_ROWS = DESCEND_THREADS / WAVE;
constexpr uint32_t MAX_PATH = 1u << 22;

template <bool TOWARDS>
__device__ __forceinline__ void descend_row(const DescendOctileArgs &a) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t p = blockIdx.x * DESCEND_ROWS + threadIdx.x / WAVE;  // the wave's row
  if (p >= a.n) return;
  const uint32_t W = a.width, H = a.height;
  const size_t grid = (size_t)p * W * H;
  const float *floor = a.floor + grid, *ceiling = a.ceiling + grid;
  const uint32_t *dist = a.dist + grid;
  int32_t *path = a.path_out ? a.path_out + (size_t)p * a.path_len * 2 : nullptr;  // (column, row) pairs, 4-byte aligned as the ABI says
  const WalkLimits lim{a.max_step, a.max_drop, a.clearance};
  // the move of the field's relation between cells x and y, y the one nearer the seed
  auto move = [&](uint32_t x, uint32_t y) {
    return TOWARDS ? allowed(floor[x], ceiling[x], floor[y], ceiling[y], lim) : allowed(floor[y], ceiling[y], floor[x], ceiling[x], lim);
  };

  int32_t col = a.starts[2 * (size_t)p], row = a.starts[2 * (size_t)p + 1];
  const bool inside = (uint32_t)col < W && (uint32_t)row < H;
  uint32_t d = inside ? dist[(uint32_t)row * W + (uint32_t)col] : UNREACHED;
  uint32_t m = 0;
  if (d == UNREACHED) col = -1, row = -1;
  else {
    // the neighbour this lane tests: lanes 0 .. 3 are (column - 1, column + 1, row - 1, row + 1), lanes 4 .. 7 the offsets
    // (-1, -1), (+1, -1), (-1, +1), (+1, +1)
    const int32_t dc = lane < 4 ? (lane == 0 ? -1 : (lane == 1 ? 1 : 0)) : ((lane & 1u) ? 1 : -1);
    const int32_t dr = lane < 4 ? (lane == 2 ? -1 : (lane == 3 ? 1 : 0)) : ((lane & 2u) ? 1 : -1);
    const uint32_t cost = lane < 4 ? a.axial_cost : a.diagonal_cost;
    const uint32_t bound = d > a.stop_dist ? min(a.max_moves, d - a.stop_dist) : 0u;
    for (; m < bound && d > a.stop_dist; m++) {
      bool ok = false;
      const uint32_t bc = (uint32_t)(col + dc), br = (uint32_t)(row + dr);  // (outside: far above W, H)
      if (lane < 8 && bc < W && br < H) {
        const uint32_t at = (uint32_t)row * W + (uint32_t)col, b = br * W + bc;
        const uint32_t db = dist[b];
        if (db <= d && d - db == cost) {  // D(b) + cost == D(a), in integers: an unreached b is above every D(a) walked from
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
      col += k < 4 ? (k == 0 ? -1 : (k == 1 ? 1 : 0)) : ((k & 1u) ? 1 : -1);
      row += k < 4 ? (k == 2 ? -1 : (k == 3 ? 1 : 0)) : ((k & 2u) ? 1 : -1);
      d -= k < 4 ? a.axial_cost : a.diagonal_cost;
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

__global__ __launch_bounds__(DESCEND_THREADS) void flood_descend_octile_kernel(DescendOctileArgs a) { descend_row<false>(a); }
__global__ __launch_bounds__(DESCEND_THREADS) void flood_descend_octile_towards_kernel(DescendOctileArgs a) { descend_row<true>(a); }

// ---- the host's side ----
// what both calls check: rdoom_flood_grids' shared arguments, then the costs
rdoom_status check_octile(const rdoom_flood_octile_params *params, uint32_t n, bool pointers, const char *missing, uint32_t width, uint32_t height) {
  rdoom_flood_params shared{};
  if (params) shared = rdoom_flood_params{params->max_step, params->max_drop, params->clearance, params->flags};
  if (rdoom_status s = rdoom::check_flood_grids(params ? &shared : nullptr, n, pointers, missing, width, height)) return s;
  const uint32_t axial = params->axial_cost, diagonal = params->diagonal_cost;
  if (axial < 1 || diagonal < axial || diagonal > 2 * (uint64_t)axial)
    return rdoom::fail(RDOOM_BAD_ARG, "costs %u and %u: 1 <= axial_cost <= diagonal_cost <= 2 * axial_cost", axial, diagonal);
  if ((uint64_t)axial * width * height > DIST_MASK)
    return rdoom::fail(RDOOM_BAD_ARG, "an axial_cost of %u on a grid of %u x %u cells: the product is at most %u", axial, width, height, DIST_MASK);
  return RDOOM_OK;
}

}  // namespace

static_assert(sizeof(rdoom_flood_octile_params) == 24, "ABI sizes");

extern "C" {

rdoom_status rdoom_flood_grids_octile(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                      const int32_t *d_seeds, const rdoom_flood_octile_params *params, uint32_t *d_dist_out,
                                      uint32_t *d_count_out, void *stream) {
  if (rdoom_status s = check_octile(params, n, d_floor && d_ceiling && d_dist_out, "floor, ceiling or distance output", width, height)) return s;
  if (!n) return RDOOM_OK;
  const FloodOctileArgs a{d_floor,  d_ceiling, d_seeds, d_count_out, d_dist_out, width, height, rdoom::flood_run_length(width, height),
                          params->flags & RDOOM_FLOOD_TOWARDS, params->axial_cost, params->diagonal_cost, params->max_step, params->max_drop,
                          params->clearance};
  return rdoom::launch_checked(flood_octile_kernel, dim3(n), dim3(THREADS), 0, stream, a);
}

rdoom_status rdoom_flood_descend_octile(const float *d_floor, const float *d_ceiling, const uint32_t *d_dist, uint32_t n, uint32_t width,
                                        uint32_t height, const int32_t *d_starts, const rdoom_flood_octile_params *params,
                                        uint32_t max_moves, uint32_t stop_dist, int32_t *d_cells_out, uint32_t *d_moves_out,
                                        int32_t *d_path_out, uint32_t path_len, void *stream) {
  if (rdoom_status s = check_octile(params, n, d_floor && d_ceiling && d_dist && d_starts && d_cells_out && d_moves_out,
                                    "floor, ceiling, distances, starts, cell output or move output", width, height))
    return s;
  if (d_path_out && (path_len == 0 || path_len > MAX_PATH))
    return rdoom::fail(RDOOM_BAD_ARG, "a path of %u entries: 1 to %u", path_len, MAX_PATH);
  if (!n) return RDOOM_OK;
  const DescendOctileArgs a{d_floor, d_ceiling, d_dist, d_starts, d_cells_out, d_moves_out, d_path_out, n, width, height,
                            d_path_out ? path_len : 0u, max_moves, stop_dist, params->axial_cost, params->diagonal_cost,
                            params->max_step, params->max_drop, params->clearance};
  const dim3 blocks((n + DESCEND_ROWS - 1) / DESCEND_ROWS);
  if (params->flags & RDOOM_FLOOD_TOWARDS)
    return rdoom::launch_checked(flood_descend_octile_towards_kernel, blocks, dim3(DESCEND_THREADS), 0, stream, a);
  return rdoom::launch_checked(flood_descend_octile_kernel, blocks, dim3(DESCEND_THREADS), 0, stream, a);
}

}  // extern "C"
