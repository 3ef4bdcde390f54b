// The three distance floods: every player's sector map flooded from a seed cell (include/rdoom.h "flood", DESIGN section 20:
// rdoom_flood_maps, rdoom_flood_max_cells), grids of any size flooded from a seed or towards it (include/rdoom.h "goal
// distance", DESIGN section 23: rdoom_flood_grids, rdoom_flood_grid_max_cells, rdoom::check_flood_grids), and such grids flooded
// over moves to the eight neighbours, an axial move costing axial_cost and a diagonal one diagonal_cost (include/rdoom.h "octile
// distance", DESIGN section 26: rdoom_flood_grids_octile, rdoom::check_flood_octile).  They read floor and ceiling planes --
// rdoom_world_draw_sector_maps' or rdoom_world_draw_area_planes' -- and nothing else: no world handle, no table.
//
// Arithmetic: binary32, the contract's comparisons in the contract's order; the build passes -ffp-contract=off.  The open and move
// comparisons are world_shared.hpp's, the ones path.hip walks with.  Costs and distances are integers.
//
// One skeleton, `flood`, over a store: where a cell's distance and its move bits live, what a move costs and whether there are
// diagonal ones.  flood_maps_kernel keeps them in LDS (LdsStore), flood_grids_kernel and flood_octile_kernel in the output itself
// (GlobalStore, OctileStore: one template).  One 1024-thread workgroup per grid.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::allowed;
using rdoom_dev::FloodArgs;
using rdoom_dev::FloodGridArgs;
using rdoom_dev::FloodOctileArgs;
using rdoom_dev::FloodPlanes;
using rdoom_dev::is_open;
using rdoom_dev::WalkLimits;

constexpr uint32_t WAVE = 64, THREADS = 1024;
constexpr uint32_t STATIC_LDS = (2 + THREADS / WAVE) * sizeof(uint32_t);  // the skeleton's: two flags and a count per wave
constexpr uint32_t MAX_SEG = 64;

// ---- the LDS store: per cell a 16-bit distance and a byte of move bits in dynamic LDS, 3 bytes a cell, plain loads and stores;
// what an owner reads of a neighbouring run are aligned 16-bit words.  No global atomics, no scratch; the write-out copies the
// distances to global memory, a wave 64 consecutive cells at a time ----
struct LdsStore {
  static constexpr uint32_t FROM_LEFT = 1, FROM_RIGHT = 2, FROM_ABOVE = 4, FROM_BELOW = 8;  // above: the stored row before
  static constexpr uint32_t UNREACHED = RDOOM_FLOOD_UNREACHED;
  static constexpr bool DIAGONALS = false;
  static constexpr uint32_t axial() { return 1u; }  // what a move costs: a compile-time constant
  // The LDS of a launch that raises no attribute of the function is 64 KiB, static and dynamic together, and two such workgroups
  // fit a CU's 160 KiB.  255 x 85 cells: 43 352 bytes of distances (rounded up to a word) + 21 675 of move bits + STATIC_LDS.
  static constexpr uint32_t MAX_CELLS = 21675;
  static constexpr uint32_t dist_bytes(uint32_t cells) { return (cells * 2u + 3u) & ~3u; }

  uint16_t *dist;
  uint8_t *moves;
  uint16_t *out;

  __device__ __forceinline__ void stage(uint32_t i, uint32_t m, bool seeded) {
    moves[i] = (uint8_t)m;
    dist[i] = (uint16_t)(seeded ? 0u : UNREACHED);
  }

  template <uint32_t FWD, uint32_t BWD>
  __device__ __forceinline__ bool sweep(uint32_t base, uint32_t stride, uint32_t len, bool before, bool after, uint32_t cost) {
    bool fell = false;
    uint32_t carry = before ? dist[base - stride] : UNREACHED;
    for (uint32_t k = 0, at = base; k < len; k++, at += stride) {
      uint32_t d = dist[at];
      if ((moves[at] & FWD) && carry + cost < d) dist[at] = (uint16_t)(d = carry + cost), fell = true;
      carry = d;
    }
    const uint32_t last = base + (len - 1u) * stride;
    carry = after ? dist[last + stride] : UNREACHED;
    for (uint32_t k = 0, at = last; k < len; k++, at -= stride) {
      uint32_t d = dist[at];
      if ((moves[at] & BWD) && carry + cost < d) dist[at] = (uint16_t)(d = carry + cost), fell = true;
      carry = d;
    }
    return fell;
  }

  __device__ __forceinline__ bool finish(uint32_t i) {
    const uint32_t d = dist[i];
    out[i] = (uint16_t)d;
    return d != UNREACHED;
  }
};
static_assert(LdsStore::dist_bytes(LdsStore::MAX_CELLS) + LdsStore::MAX_CELLS + STATIC_LDS <= 64 * 1024, "flood: the LDS of the largest grid");
static_assert(LdsStore::MAX_CELLS >= 19200 && LdsStore::MAX_CELLS < LdsStore::UNREACHED, "flood: the contract's limits");

// ---- the global stores: always in global memory, so a grid of any size takes the same code.  A cell's word of d_dist_out holds its
// distance in the low BITS bits (PENDING: not reached so far) and, while the kernel runs, its move bits above them -- four in the
// top four of 28 + 4 (GlobalStore), or with DIAGONALS eight in the top byte of 24 + 8 (OctileStore); the write-out stores the clean
// distances in place, a thread the words it staged.  A word is read and written whole by relaxed workgroup-scope atomic accesses, so
// it is never torn.
// Visibility: the rule relied on is the AMDGPU memory model's for workgroup scope outside threadgroup-split mode.  The waves of a
// workgroup run on one CU and share its vector L1, which takes that CU's vector memory accesses in the order they were issued and
// which every store writes through; so a workgroup-scope release or acquire of global memory needs no cache maintenance and no wait
// on the vector-memory counter, and the compiler emits none: __syncthreads() is that fence pair around s_barrier and comes out as
// a bare s_barrier (with a wait for LDS only).  A word stored by a wave before the barrier was issued to the L1 before any load a
// wave issues after it, so that load reads it.  The relaxed workgroup-scope atomics (sc0 loads and stores) keep every access to a
// cell's word on that path -- the vector L1, never the scalar cache, never a register copy carried across a barrier.  No other
// workgroup touches the grid, and nothing waits for one: no grid-wide barrier, no spin on global memory, no global
// read-modify-write ----
template <uint32_t BITS, bool DIAG>
struct GridStore {
  static constexpr uint32_t DIST_BITS = BITS, DIST_MASK = (1u << DIST_BITS) - 1u;
  static constexpr uint32_t PENDING = DIST_MASK;  // a cell not reached so far, while the kernel runs
  static constexpr bool DIAGONALS = DIAG;
  // the cell may be entered from the neighbour at (column - 1, row), (column + 1, row), (column, row - 1), (column, row + 1) ...
  static constexpr uint32_t FROM_LEFT = 1u << DIST_BITS, FROM_RIGHT = 2u << DIST_BITS, FROM_ABOVE = 4u << DIST_BITS, FROM_BELOW = 8u << DIST_BITS;
  // ... and with DIAGONALS from (column - 1, row - 1), (column + 1, row + 1), (column + 1, row - 1), (column - 1, row + 1)
  static constexpr uint32_t FROM_UP_LEFT = 16u << DIST_BITS, FROM_DOWN_RIGHT = 32u << DIST_BITS, FROM_UP_RIGHT = 64u << DIST_BITS,
                            FROM_DOWN_LEFT = 128u << DIST_BITS;
  static_assert(DIST_BITS + (DIAGONALS ? 8u : 4u) == 32u, "flood: a word is a distance and the move bits");
  static constexpr uint32_t MAX_CELLS = 1u << 22;
  static constexpr uint32_t BATCH = 8;  // the words of a run loaded side by side before they are walked

  uint32_t *dist;
  uint32_t axial_cost, diagonal_cost;  // read with DIAGONALS alone: without them a move costs the constant 1

  __device__ __forceinline__ uint32_t axial() const { return DIAGONALS ? axial_cost : 1u; }
  __device__ __forceinline__ uint32_t diagonal() const { return diagonal_cost; }

  static __device__ __forceinline__ uint32_t word_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ void word_store(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

  __device__ __forceinline__ void stage(uint32_t i, uint32_t m, bool seeded) { word_store(dist + i, m | (seeded ? 0u : PENDING)); }

  // the second staging step, after a barrier: the four diagonal bits of cell i from the axial bits of the cell and of the two cells
  // between it and the diagonal neighbour -- the contract's rule, the same formula in either direction because the axial bits are
  // already those of the relation that is followed.  A thread rewrites the words it staged; what it reads of other words are their
  // axial bits, which no one changes.  A bit of the cell towards a side says that side's neighbour is inside the grid, so the cells
  // read are
  __device__ __forceinline__ void stage_diagonals(uint32_t i, uint32_t W) {
    const uint32_t w = word_load(dist + i);
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

  // a batch of a run walked in one direction: words w[0 .. m) of cells at, at + step, ..., the distance of the cell before them in
  // `carry`.  carry + cost does not wrap: carry <= PENDING < 2^28 and a cost is 1, or below 2^25 (check_flood_octile) with PENDING
  // < 2^24; from PENDING it is never below a distance
  template <uint32_t BIT>
  __device__ __forceinline__ bool walk(const uint32_t (&w)[BATCH], uint32_t m, uint32_t at, int32_t step, uint32_t cost, uint32_t &carry) {
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

  template <uint32_t FWD, uint32_t BWD>
  __device__ __forceinline__ bool sweep(uint32_t base, uint32_t stride, uint32_t len, bool before, bool after, uint32_t cost) {
    bool fell = false;
    uint32_t carry = before ? word_load(dist + (base - stride)) & DIST_MASK : PENDING;
    for (uint32_t k0 = 0; k0 < len; k0 += BATCH) {
      const uint32_t m = min(BATCH, len - k0), at = base + k0 * stride;
      uint32_t w[BATCH];
#pragma unroll
      for (uint32_t j = 0; j < BATCH; j++) w[j] = j < m ? word_load(dist + (at + j * stride)) : 0u;
      fell |= walk<FWD>(w, m, at, (int32_t)stride, cost, carry);
    }
    const uint32_t last = base + (len - 1u) * stride;
    carry = after ? word_load(dist + (last + stride)) & DIST_MASK : PENDING;
    for (uint32_t k0 = 0; k0 < len; k0 += BATCH) {
      const uint32_t m = min(BATCH, len - k0), at = last - k0 * stride;
      uint32_t w[BATCH];
#pragma unroll
      for (uint32_t j = 0; j < BATCH; j++) w[j] = j < m ? word_load(dist + (at - j * stride)) : 0u;
      fell |= walk<BWD>(w, m, at, -(int32_t)stride, cost, carry);
    }
    return fell;
  }

  __device__ __forceinline__ bool finish(uint32_t i) {
    const uint32_t d = word_load(dist + i) & DIST_MASK;
    word_store(dist + i, d == PENDING ? RDOOM_FLOOD_GRID_UNREACHED : d);
    return d != PENDING;
  }
};
using GlobalStore = GridStore<28, false>;
using OctileStore = GridStore<24, true>;
static_assert(GlobalStore::MAX_CELLS < GlobalStore::PENDING && GlobalStore::MAX_CELLS <= RDOOM_AREA_MAX_SIDE * RDOOM_AREA_MAX_SIDE,
              "flood_grids: a distance fits its 28 bits");

// ---- the skeleton: grid blockIdx.x of `a` flooded in store `s`.  The four move bits of every cell -- the cell may be entered from
// its left, right, upper, lower neighbour; `towards`: it may be LEFT for that neighbour, the same relation followed backwards --
// are computed once from the floats and staged with the seed's 0; a store with DIAGONALS then, after a barrier, adds the four
// diagonal bits (Store::stage_diagonals).  Then passes until one changes nothing.  A pass is two phases with a barrier between
// them: in the row phase a thread owns runs of `seg` cells of a row and carries a distance along each left to right and back
// right to left (Store::sweep: cells base + k * stride, k < len, every move costing `cost`, forwards with the distance of the cell
// before the run, if there is one, carried in through the FWD bits, then backwards from the cell after it through the BWD bits;
// true when a distance fell; len >= 1, and with len == 1 the stride may be 0); in the column phase it owns runs of a column, top
// to bottom and back.  With DIAGONALS two more phases follow, each after a barrier: the runs of stride width + 1, then those of
// stride width - 1.  A diagonal run is the part of one diagonal inside a band of `seg` grid rows; run j of band r0 is the diagonal
// column - row == j - (r0 + seg - 1), the anti-diagonal column + row == r0 + j, j < width + seg - 1: every diagonal that meets the
// band, consecutive lanes on consecutive columns.  In a phase only a run's owner writes its cells; what it reads of another run
// (the one cell before and the one after, never torn) may be mid-pass -- values only fall and every value ever stored is the cost
// of a real path, so any schedule ends at the same fixed point, the cheapest costs.
// Termination: the loop condition is one LDS word (two, used alternately) every thread reads between two barriers, so it is
// workgroup-uniform, no thread returns early and every thread reaches every barrier, and the `for` has the hard bound cells + 1
// -- a pass relaxes every allowed move, axial and diagonal, at least once (a Bellman-Ford round) and a cheapest path has fewer
// than `cells` moves, so pass number `cells` at the latest changes nothing.  A closed or outside seed leaves every cell
// unreached: the first pass changes nothing and is the last.
// Last the write-out (Store::finish: a cell's final distance, and whether it was reached) and the count of reached cells ----
template <class Store>
__device__ __forceinline__ void flood(Store s, const FloodPlanes &a, bool towards) {  // (towards: uniform)
  __shared__ uint32_t changed[2];
  __shared__ uint32_t wave_count[THREADS / WAVE];
  static_assert(sizeof changed + sizeof wave_count == STATIC_LDS, "flood: STATIC_LDS");

  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  const uint32_t W = a.width, H = a.height, cells = a.cells;
  const float *floor = a.floor + (size_t)p * cells, *ceiling = a.ceiling + (size_t)p * cells;

  uint32_t seed = 0xFFFFFFFFu;  // outside the grid: no cell
  {
    const int32_t sc = a.seeds ? a.seeds[2 * (size_t)p] : (int32_t)(W / 2u);
    const int32_t sr = a.seeds ? a.seeds[2 * (size_t)p + 1] : (int32_t)(H / 2u);
    if ((uint32_t)sc < W && (uint32_t)sr < H) seed = (uint32_t)sr * W + (uint32_t)sc;
  }

  // staging.  Forwards a bit says the neighbour's move INTO the cell is allowed, towards the seed that the cell's move into the
  // neighbour is
  const WalkLimits lim{a.max_step, a.max_drop, a.clearance};
  for (uint32_t i = tid; i < cells; i += THREADS) {
    const uint32_t r = i / W, c = i - r * W;
    const float f = floor[i], g = ceiling[i];
    const bool open = is_open(f, g, lim.clearance);
    uint32_t m = 0;
    if (open) {
      auto move = [&](uint32_t other) { return towards ? allowed(f, g, floor[other], ceiling[other], lim) : allowed(floor[other], ceiling[other], f, g, lim); };
      if (c > 0 && move(i - 1)) m |= Store::FROM_LEFT;
      if (c + 1 < W && move(i + 1)) m |= Store::FROM_RIGHT;
      if (r > 0 && move(i - W)) m |= Store::FROM_ABOVE;
      if (r + 1 < H && move(i + W)) m |= Store::FROM_BELOW;
    }
    s.stage(i, m, open && i == seed);
  }
  if (tid == 0) changed[0] = 0, changed[1] = 0;
  __syncthreads();
  if constexpr (Store::DIAGONALS) {
    for (uint32_t i = tid; i < cells; i += THREADS) s.stage_diagonals(i, W);
    __syncthreads();
  }

  const uint32_t seg = a.seg;
  const uint32_t runs_per_row = (W + seg - 1) / seg, bands = (H + seg - 1) / seg;
  const uint32_t row_runs = H * runs_per_row, column_runs = W * bands;
  const uint32_t runs_per_band = W + seg - 1, diagonal_runs = bands * runs_per_band;  // (DIAGONALS)
  for (uint32_t pass = 0; pass <= cells; pass++) {  // (the hard bound; the flag ends it long before)
    uint32_t *flag = &changed[pass & 1u];
    bool fell = false;
    for (uint32_t run = tid; run < row_runs; run += THREADS) {
      const uint32_t r = run / runs_per_row, c0 = (run - r * runs_per_row) * seg;
      const uint32_t len = min(seg, W - c0);
      fell |= s.template sweep<Store::FROM_LEFT, Store::FROM_RIGHT>(r * W + c0, 1u, len, c0 > 0, c0 + len < W, s.axial());
    }
    __syncthreads();
    if (tid == 0) changed[(pass + 1u) & 1u] = 0;  // the next pass's: last read before the barrier above
    for (uint32_t run = tid; run < column_runs; run += THREADS) {  // consecutive lanes: consecutive columns
      const uint32_t k = run / W, c = run - k * W, r0 = k * seg;
      const uint32_t len = min(seg, H - r0);
      fell |= s.template sweep<Store::FROM_ABOVE, Store::FROM_BELOW>(r0 * W + c, W, len, r0 > 0, r0 + len < H, s.axial());
    }
    if constexpr (Store::DIAGONALS) {
      __syncthreads();
      for (uint32_t run = tid; run < diagonal_runs; run += THREADS) {  // column - row == k: rows lo .. hi - 1 of the band
        const uint32_t b = run / runs_per_band;
        const int32_t r0 = (int32_t)(b * seg), k = (int32_t)(run - b * runs_per_band) - (r0 + (int32_t)seg - 1);
        const int32_t lo = max(r0, -k), hi = min(min(r0 + (int32_t)seg, (int32_t)H), (int32_t)W - k);
        if (lo < hi)
          fell |= s.template sweep<Store::FROM_UP_LEFT, Store::FROM_DOWN_RIGHT>((uint32_t)lo * W + (uint32_t)(k + lo), W + 1u, (uint32_t)(hi - lo),
                                                                                lo > 0 && k + lo > 0, hi < (int32_t)H && k + hi < (int32_t)W,
                                                                                s.diagonal());
      }
      __syncthreads();
      for (uint32_t run = tid; run < diagonal_runs; run += THREADS) {  // column + row == k
        const uint32_t b = run / runs_per_band;
        const int32_t r0 = (int32_t)(b * seg), k = r0 + (int32_t)(run - b * runs_per_band);
        const int32_t lo = max(r0, k - ((int32_t)W - 1)), hi = min(min(r0 + (int32_t)seg, (int32_t)H), k + 1);
        if (lo < hi)
          fell |= s.template sweep<Store::FROM_UP_RIGHT, Store::FROM_DOWN_LEFT>((uint32_t)lo * W + (uint32_t)(k - lo), W - 1u, (uint32_t)(hi - lo),
                                                                                lo > 0 && k - lo + 1 < (int32_t)W, hi < (int32_t)H && k - hi >= 0,
                                                                                s.diagonal());
      }
    }
    if (fell) *flag = 1;
    __syncthreads();
    if (*flag == 0) break;  // one word, read by every thread after the barrier: uniform
  }

  // out; the count by shuffles, then across the waves through LDS
  uint32_t reached = 0;
  for (uint32_t i = tid; i < cells; i += THREADS) reached += s.finish(i);
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

__global__ __launch_bounds__(THREADS) void flood_maps_kernel(FloodArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint16_t flood_lds[];
  flood(LdsStore{flood_lds, (uint8_t *)flood_lds + LdsStore::dist_bytes(a.planes.cells), a.dist_out + (size_t)blockIdx.x * a.planes.cells}, a.planes,
        false);
}

__global__ __launch_bounds__(THREADS) void flood_grids_kernel(FloodGridArgs a) {
  flood(GlobalStore{a.dist_out + (size_t)blockIdx.x * a.planes.cells}, a.planes, a.towards != 0);
}

__global__ __launch_bounds__(THREADS) void flood_octile_kernel(FloodOctileArgs a) {
  flood(OctileStore{a.dist_out + (size_t)blockIdx.x * a.planes.cells, a.axial_cost, a.diagonal_cost}, a.planes, a.towards != 0);
}

// ---- the host's side ----
rdoom_status check_limits(const rdoom_flood_params *params) {
  const auto bad = [](float v) { return !(v >= 0.0f); };  // a NaN or negative
  if (bad(params->max_step)) return rdoom::fail(RDOOM_BAD_ARG, "max_step %g is a NaN or negative", (double)params->max_step);
  if (bad(params->max_drop)) return rdoom::fail(RDOOM_BAD_ARG, "max_drop %g is a NaN or negative", (double)params->max_drop);
  if (bad(params->clearance)) return rdoom::fail(RDOOM_BAD_ARG, "clearance %g is a NaN or negative", (double)params->clearance);
  return RDOOM_OK;
}

FloodPlanes flood_planes(const float *d_floor, const float *d_ceiling, const int32_t *d_seeds, uint32_t *d_count_out, uint32_t width,
                         uint32_t height, const rdoom_flood_params *params) {
  return FloodPlanes{d_floor, d_ceiling, d_seeds, d_count_out, width, height, width * height, rdoom::flood_run_length(width, height),
                     params->max_step, params->max_drop, params->clearance};
}

}  // namespace

static_assert(sizeof(rdoom_flood_params) == 16 && sizeof(rdoom_flood_octile_params) == 24, "ABI sizes");

// the cells of a row or column one thread sweeps at a time: the shortest runs that give every thread at most one run of a phase,
// where the grid's shape allows that
uint32_t rdoom::flood_run_length(uint32_t width, uint32_t height) {
  uint32_t seg = 2;
  while (seg < MAX_SEG && ((uint64_t)height * ((width + seg - 1) / seg) > THREADS || (uint64_t)width * ((height + seg - 1) / seg) > THREADS)) seg++;
  return seg;
}

// what rdoom_flood_grids and rdoom_flood_descend (path.hip) check of the arguments they share
rdoom_status rdoom::check_flood_grids(const rdoom_flood_params *params, uint32_t n, bool pointers, const char *missing, uint32_t width,
                                      uint32_t height) {
  if (!params) return rdoom::fail(RDOOM_BAD_ARG, "null params");
  if (n && !pointers) return rdoom::fail(RDOOM_BAD_ARG, "null %s with n = %u", missing, n);
  if (!width || !height) return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells (at least 1 a side)", width, height);
  if (width > RDOOM_AREA_MAX_SIDE || height > RDOOM_AREA_MAX_SIDE)
    return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells: a side is at most %u", width, height, RDOOM_AREA_MAX_SIDE);
  if ((uint64_t)width * height > GlobalStore::MAX_CELLS)
    return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells: too many (at most %u)", width, height, GlobalStore::MAX_CELLS);
  if (params->flags & ~RDOOM_FLOOD_TOWARDS) return rdoom::fail(RDOOM_BAD_ARG, "flood flags 0x%x: 0 or RDOOM_FLOOD_TOWARDS", params->flags);
  if (rdoom_status s = check_limits(params)) return s;
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u grids: too many for one launch", n);
  return RDOOM_OK;
}

// what rdoom_flood_grids_octile and rdoom_flood_descend_octile (path.hip) check: the arguments above, then the costs
rdoom_status rdoom::check_flood_octile(const rdoom_flood_octile_params *params, uint32_t n, bool pointers, const char *missing, uint32_t width,
                                       uint32_t height) {
  rdoom_flood_params shared{};
  if (params) shared = rdoom_flood_params{params->max_step, params->max_drop, params->clearance, params->flags};
  if (rdoom_status s = rdoom::check_flood_grids(params ? &shared : nullptr, n, pointers, missing, width, height)) return s;
  const uint32_t axial = params->axial_cost, diagonal = params->diagonal_cost;
  if (axial < 1 || diagonal < axial || diagonal > 2 * (uint64_t)axial)
    return rdoom::fail(RDOOM_BAD_ARG, "costs %u and %u: 1 <= axial_cost <= diagonal_cost <= 2 * axial_cost", axial, diagonal);
  if ((uint64_t)axial * width * height > OctileStore::DIST_MASK)
    return rdoom::fail(RDOOM_BAD_ARG, "an axial_cost of %u on a grid of %u x %u cells: the product is at most %u", axial, width, height,
                       OctileStore::DIST_MASK);
  return RDOOM_OK;
}

// what rdoom_grid_walk_lines (line.hip) checks: the arguments above (RDOOM_LINE_REVERSED is the one flag bit), then the targets
rdoom_status rdoom::check_walk_lines(const rdoom_flood_params *params, uint32_t n, bool pointers, uint32_t width, uint32_t height, uint32_t n_to) {
  static_assert(RDOOM_LINE_REVERSED == RDOOM_FLOOD_TOWARDS, "check_flood_grids admits the one flag bit");
  if (rdoom_status s = rdoom::check_flood_grids(params, n, pointers, "floor, ceiling, starts, targets or clear output", width, height)) return s;
  if (!n_to) return rdoom::fail(RDOOM_BAD_ARG, "n_to is 0: at least one target a row");
  if ((uint64_t)n * n_to > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u rows of %u targets: too many lines for one launch", n, n_to);
  return RDOOM_OK;
}

// what rdoom_path_straighten (line.hip) checks: the arguments above, then the look-ahead and the two lengths
rdoom_status rdoom::check_path_straighten(const rdoom_flood_params *params, uint32_t n, bool pointers, uint32_t width, uint32_t height,
                                          uint32_t path_len, uint32_t max_look, uint32_t corner_len) {
  constexpr uint32_t MAX_LEN = 1u << 22;
  if (rdoom_status s = rdoom::check_flood_grids(params, n, pointers, "floor, ceiling, starts, path, corner output or count output", width, height))
    return s;
  if (!max_look || max_look > RDOOM_STRAIGHTEN_MAX_LOOK)
    return rdoom::fail(RDOOM_BAD_ARG, "a max_look of %u: 1 to %u", max_look, RDOOM_STRAIGHTEN_MAX_LOOK);
  if (!path_len || path_len > MAX_LEN) return rdoom::fail(RDOOM_BAD_ARG, "a path of %u entries: 1 to %u", path_len, MAX_LEN);
  if (!corner_len || corner_len > MAX_LEN) return rdoom::fail(RDOOM_BAD_ARG, "a corner_len of %u entries: 1 to %u", corner_len, MAX_LEN);
  return RDOOM_OK;
}

extern "C" {

rdoom_status rdoom_flood_max_cells(uint32_t *cells_out) {
  if (!cells_out) return rdoom::fail(RDOOM_BAD_ARG, "null cells_out");
  *cells_out = LdsStore::MAX_CELLS;
  return RDOOM_OK;
}

rdoom_status rdoom_flood_grid_max_cells(uint32_t *cells_out) {
  if (!cells_out) return rdoom::fail(RDOOM_BAD_ARG, "null cells_out");
  *cells_out = GlobalStore::MAX_CELLS;
  return RDOOM_OK;
}

rdoom_status rdoom_flood_maps(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height, const int32_t *d_seeds,
                              const rdoom_flood_params *params, uint16_t *d_dist_out, uint32_t *d_count_out, void *stream) {
  if (!params) return rdoom::fail(RDOOM_BAD_ARG, "null params");
  if (n && (!d_floor || !d_ceiling || !d_dist_out)) return rdoom::fail(RDOOM_BAD_ARG, "null floor, ceiling or distance output with n = %u", n);
  if (!width || !height) return rdoom::fail(RDOOM_BAD_ARG, "a map of %u x %u cells (at least 1 a side)", width, height);
  if ((uint64_t)width * height > LdsStore::MAX_CELLS)
    return rdoom::fail(RDOOM_BAD_ARG, "a map of %u x %u cells: too many for one workgroup's LDS (at most %u)", width, height, LdsStore::MAX_CELLS);
  if (params->flags) return rdoom::fail(RDOOM_BAD_ARG, "flood flags 0x%x: must be 0", params->flags);
  if (rdoom_status s = check_limits(params)) return s;
  if (n > 0x7FFFFFFFu) return rdoom::fail(RDOOM_BAD_ARG, "%u maps: too many for one launch", n);
  if (!n) return RDOOM_OK;
  const FloodArgs a{flood_planes(d_floor, d_ceiling, d_seeds, d_count_out, width, height, params), d_dist_out};
  return rdoom::launch_checked(flood_maps_kernel, dim3(n), dim3(THREADS), LdsStore::dist_bytes(a.planes.cells) + a.planes.cells, stream, a);
}

rdoom_status rdoom_flood_grids(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height, const int32_t *d_seeds,
                               const rdoom_flood_params *params, uint32_t *d_dist_out, uint32_t *d_count_out, void *stream) {
  if (rdoom_status s = rdoom::check_flood_grids(params, n, d_floor && d_ceiling && d_dist_out, "floor, ceiling or distance output", width, height)) return s;
  if (!n) return RDOOM_OK;
  const FloodGridArgs a{flood_planes(d_floor, d_ceiling, d_seeds, d_count_out, width, height, params), d_dist_out,
                        params->flags & RDOOM_FLOOD_TOWARDS};
  return rdoom::launch_checked(flood_grids_kernel, dim3(n), dim3(THREADS), 0, stream, a);
}

rdoom_status rdoom_flood_grids_octile(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                      const int32_t *d_seeds, const rdoom_flood_octile_params *params, uint32_t *d_dist_out,
                                      uint32_t *d_count_out, void *stream) {
  if (rdoom_status s = rdoom::check_flood_octile(params, n, d_floor && d_ceiling && d_dist_out, "floor, ceiling or distance output", width, height))
    return s;
  if (!n) return RDOOM_OK;
  const rdoom_flood_params limits{params->max_step, params->max_drop, params->clearance, params->flags};
  const FloodOctileArgs a{{flood_planes(d_floor, d_ceiling, d_seeds, d_count_out, width, height, &limits), d_dist_out,
                           params->flags & RDOOM_FLOOD_TOWARDS},
                          params->axial_cost, params->diagonal_cost};
  return rdoom::launch_checked(flood_octile_kernel, dim3(n), dim3(THREADS), 0, stream, a);
}

}  // extern "C"
