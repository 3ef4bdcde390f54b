// Every player's sector map flooded from a seed cell: the walking distance to every cell (include/rdoom.h "flood", DESIGN section
// 20): rdoom_flood_maps and rdoom_flood_max_cells.  It reads the floor and ceiling planes rdoom_world_draw_sector_maps writes and
// nothing else: no world handle, no table.
//
// Arithmetic: binary32, the contract's comparisons in the contract's order; the build passes -ffp-contract=off.
//
// One 1024-thread workgroup per player.  Staged once from global memory into dynamic LDS: per cell a byte of four bits -- the cell
// may be entered from its left, right, upper, lower neighbour -- and a 16-bit distance, 3 bytes a cell.  Then passes entirely in
// LDS until one changes nothing.  A pass is two phases with a barrier between them: in the row phase a thread owns a run of `seg`
// cells of a row and carries a distance along it left to right and back right to left; in the column phase it owns a run of a
// column, top to bottom and back.  In a phase only a run's owner writes its cells; what it reads of a neighbouring run (the one
// cell before and the one after, aligned 16-bit words) may be mid-pass -- values only fall and every value ever stored is the length
// of a real path, so any schedule ends at the same fixed point, the shortest distances.
// Termination: the loop condition is one LDS word every thread reads between two barriers, so it is workgroup-uniform, every
// thread reaches every barrier, and the pass count has the hard bound cells + 1 -- a pass relaxes every move at least once (a
// Bellman-Ford round), a distance is below the number of cells, so pass number `cells` at the latest changes nothing.
// No global atomics, no scratch; a wave stores runs of 64 consecutive cells.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::FloodArgs;

constexpr uint32_t WAVE = 64, THREADS = 1024;
constexpr uint32_t FROM_LEFT = 1, FROM_RIGHT = 2, FROM_ABOVE = 4, FROM_BELOW = 8;  // above: the stored row before
constexpr uint32_t UNREACHED = RDOOM_FLOOD_UNREACHED;
// The LDS of a launch that raises no attribute of the function is 64 KiB, static and dynamic together, and two such workgroups
// fit a CU's 160 KiB.  255 x 85 cells: 43 352 bytes of distances (rounded up to a word) + 21 675 of move bits + STATIC_LDS.
constexpr uint32_t MAX_CELLS = 21675;
constexpr uint32_t STATIC_LDS = (2 + THREADS / WAVE) * sizeof(uint32_t);
constexpr uint32_t MAX_SEG = 64;

constexpr uint32_t dist_bytes(uint32_t cells) { return (cells * 2u + 3u) & ~3u; }
static_assert(dist_bytes(MAX_CELLS) + MAX_CELLS + STATIC_LDS <= 64 * 1024, "flood: the LDS of the largest grid");
static_assert(MAX_CELLS >= 19200 && MAX_CELLS < UNREACHED, "flood: the contract's limits");

__device__ __forceinline__ bool is_open(float f, float g, float clearance) {
  return f < __builtin_inff() && f > -__builtin_inff() && g - f >= clearance;
}

// the move from a to b, b known to be open
__device__ __forceinline__ bool enters(float fa, float ga, float fb, float gb, const FloodArgs &a) {
  return is_open(fa, ga, a.clearance) && fb - fa <= a.max_step && fa - fb <= a.max_drop && fminf(ga, gb) - fmaxf(fa, fb) >= a.clearance;
}

// One run: cells base + k * stride, k < len, forwards with the distance of the cell before the run (if there is one) carried in
// through the FWD bits, then backwards from the cell after it through the BWD bits.  True when a distance fell.
template <uint32_t FWD, uint32_t BWD>
__device__ __forceinline__ bool sweep(uint16_t *dist, const uint8_t *moves, uint32_t base, uint32_t stride, uint32_t len, bool before,
                                      bool after) {
  bool fell = false;
  uint32_t carry = before ? dist[base - stride] : UNREACHED;
  for (uint32_t k = 0, at = base; k < len; k++, at += stride) {
    uint32_t d = dist[at];
    if ((moves[at] & FWD) && carry + 1u < d) dist[at] = (uint16_t)(d = carry + 1u), fell = true;
    carry = d;
  }
  const uint32_t last = base + (len - 1u) * stride;
  carry = after ? dist[last + stride] : UNREACHED;
  for (uint32_t k = 0, at = last; k < len; k++, at -= stride) {
    uint32_t d = dist[at];
    if ((moves[at] & BWD) && carry + 1u < d) dist[at] = (uint16_t)(d = carry + 1u), fell = true;
    carry = d;
  }
  return fell;
}

__global__ __launch_bounds__(THREADS) void flood_maps_kernel(FloodArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t flood_lds[];
  __shared__ uint32_t changed[2];
  __shared__ uint32_t wave_count[THREADS / WAVE];
  static_assert(sizeof changed + sizeof wave_count == STATIC_LDS, "flood: STATIC_LDS");
  uint16_t *dist = flood_lds;
  uint8_t *moves = (uint8_t *)flood_lds + dist_bytes(a.cells);

  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  const uint32_t W = a.width, H = a.height, cells = a.cells;
  const size_t map = (size_t)p * cells;
  const float *floor = a.floor + map, *ceiling = a.ceiling + map;

  uint32_t seed = 0xFFFFFFFFu;  // outside the grid: no cell
  {
    const int32_t sc = a.seeds ? a.seeds[2 * (size_t)p] : (int32_t)(W / 2u);
    const int32_t sr = a.seeds ? a.seeds[2 * (size_t)p + 1] : (int32_t)(H / 2u);
    if ((uint32_t)sc < W && (uint32_t)sr < H) seed = (uint32_t)sr * W + (uint32_t)sc;
  }

  // staging: the four move bits of every cell, the seed's 0
  for (uint32_t i = tid; i < cells; i += THREADS) {
    const uint32_t r = i / W, c = i - r * W;
    const float f = floor[i], g = ceiling[i];
    const bool open = is_open(f, g, a.clearance);
    uint32_t m = 0;
    if (open) {
      if (c > 0 && enters(floor[i - 1], ceiling[i - 1], f, g, a)) m |= FROM_LEFT;
      if (c + 1 < W && enters(floor[i + 1], ceiling[i + 1], f, g, a)) m |= FROM_RIGHT;
      if (r > 0 && enters(floor[i - W], ceiling[i - W], f, g, a)) m |= FROM_ABOVE;
      if (r + 1 < H && enters(floor[i + W], ceiling[i + W], f, g, a)) m |= FROM_BELOW;
    }
    moves[i] = (uint8_t)m;
    dist[i] = (uint16_t)((open && i == seed) ? 0u : UNREACHED);
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
      fell |= sweep<FROM_LEFT, FROM_RIGHT>(dist, moves, r * W + c0, 1u, len, c0 > 0, c0 + len < W);
    }
    __syncthreads();
    if (tid == 0) changed[(pass + 1u) & 1u] = 0;  // the next pass's: last read before the barrier above
    for (uint32_t run = tid; run < column_runs; run += THREADS) {  // consecutive lanes: consecutive columns
      const uint32_t k = run / W, c = run - k * W, r0 = k * seg;
      const uint32_t len = min(seg, H - r0);
      fell |= sweep<FROM_ABOVE, FROM_BELOW>(dist, moves, r0 * W + c, W, len, r0 > 0, r0 + len < H);
    }
    if (fell) *flag = 1;
    __syncthreads();
    if (*flag == 0) break;  // one word, read by every thread after the barrier: uniform
  }

  // out: a wave stores 64 consecutive cells at a time; the count by shuffles, then across the waves through LDS
  uint16_t *out = a.dist_out + map;
  uint32_t reached = 0;
  for (uint32_t i = tid; i < cells; i += THREADS) {
    const uint32_t d = dist[i];
    out[i] = (uint16_t)d;
    reached += d != UNREACHED;
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

bool bad_limit(float v) { return !(v >= 0.0f); }  // a NaN or negative

}  // namespace

static_assert(sizeof(rdoom_flood_params) == 16, "ABI sizes");

extern "C" {

rdoom_status rdoom_flood_max_cells(uint32_t *cells_out) {
  if (!cells_out) return rdoom::fail(RDOOM_BAD_ARG, "null cells_out");
  *cells_out = MAX_CELLS;
  return RDOOM_OK;
}

rdoom_status rdoom_flood_maps(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height, const int32_t *d_seeds,
                              const rdoom_flood_params *params, uint16_t *d_dist_out, uint32_t *d_count_out, void *stream) {
  if (!params) return rdoom::fail(RDOOM_BAD_ARG, "null params");
  if (n && (!d_floor || !d_ceiling || !d_dist_out)) return rdoom::fail(RDOOM_BAD_ARG, "null floor, ceiling or distance output with n = %u", n);
  if (!width || !height) return rdoom::fail(RDOOM_BAD_ARG, "a map of %u x %u cells (at least 1 a side)", width, height);
  if ((uint64_t)width * height > MAX_CELLS)
    return rdoom::fail(RDOOM_BAD_ARG, "a map of %u x %u cells: too many for one workgroup's LDS (at most %u)", width, height, MAX_CELLS);
  if (params->flags) return rdoom::fail(RDOOM_BAD_ARG, "flood flags 0x%x: must be 0", params->flags);
  if (bad_limit(params->max_step)) return rdoom::fail(RDOOM_BAD_ARG, "max_step %g is a NaN or negative", (double)params->max_step);
  if (bad_limit(params->max_drop)) return rdoom::fail(RDOOM_BAD_ARG, "max_drop %g is a NaN or negative", (double)params->max_drop);
  if (bad_limit(params->clearance)) return rdoom::fail(RDOOM_BAD_ARG, "clearance %g is a NaN or negative", (double)params->clearance);
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u maps: too many for one launch", n);
  if (!n) return RDOOM_OK;
  const uint32_t cells = width * height;
  // the shortest runs that give every thread at most one run of a phase, where the grid's shape allows that
  uint32_t seg = 2;
  while (seg < MAX_SEG && (height * ((width + seg - 1) / seg) > THREADS || width * ((height + seg - 1) / seg) > THREADS)) seg++;
  const FloodArgs a{d_floor, d_ceiling, d_seeds, d_dist_out, d_count_out, width, height, cells, seg, params->max_step, params->max_drop,
                    params->clearance};
  return rdoom::launch_checked(flood_maps_kernel, dim3(n), dim3(THREADS), dist_bytes(cells) + cells, stream, a);
}

}  // extern "C"
