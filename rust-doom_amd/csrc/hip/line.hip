// Straight walks on the grid (include/rdoom.h "straight walks"): the chain of grid moves that the segment between
// two cell centres makes, tested move by move under the floods' open and move rules (rdoom_grid_walk_lines), and a listed path
// pulled straight with it -- the farthest cell of the path a straight walk reaches, again and again (rdoom_path_straighten).
//
// Arithmetic: the chain is exact integers, every product below 2^28.  The open and move comparisons are world_shared.hpp's, the
// ones flood.hip floods with; the one binary32 sum, a straightened path's length, is the contract's operations in the contract's
// order, and the build passes -ffp-contract=off.
//
// The chain in closed form.  With dl crossings of the longer axis and ds <= dl of the shorter, long crossing L lies at parameter
// (2L + 1) / (2 dl) and short crossing j at (2j + 1) / (2 ds).  Put N = (2L + 1) * ds + dl, q = N / (2 dl) and r = N % (2 dl):
//   the short crossings strictly before long crossing L number (N - 1) / (2 dl), that is q - (r == 0);
//   long crossing L passes through a cell corner, together with short crossing q - 1, exactly when r == 0;
//   the short crossings at or before long crossing L - 1 number (N - 2 ds) / (2 dl), that is q - (r < 2 ds), and none for L == 0.
// The last two differ by at most one, because short crossings lie at least as far apart as long ones: between two long crossings
// there is at most one short crossing, and none lies after the last long one.  So step L of a line -- test_step below, the one
// function both kernels walk with -- is that short crossing if there is one, an axial move, and then long crossing L, an axial move
// or, through a corner, the diagonal one with its four axial moves; the steps 0 .. dl - 1 in order are the contract's chain.
//
// walk_lines: one wavefront per line, four lines to a 256-thread workgroup.  Lane l of chunk c takes step 64 c + l; a ballot's
// lowest set bit is the chain's first refused move, and its lane hands out the cell that move starts from.
// Termination: the chunk loop runs at most ceil(dl / 64) times, dl < the grid's longer side, and breaks at the first chunk with a
// refusal.  No barrier, no LDS, no atomic; nothing waits on anything.
//
// path_straighten: one wavefront per row, four rows to a workgroup.  The row's m -- the entries before the first that is no cell of
// the grid -- is found by ballots over chunks of 64 entries.  Then the up to max_look candidates ahead are taken in chunks of 64
// from the far end; a lane walks its own candidate's line step by step, and the highest set bit of the first chunk's ballot that
// has one is the contract's k*.  The walk's state -- the cell a, the index i, the count, the length -- is wave-uniform.
// Termination: the scan for m runs over path_len entries; every turn of the outer loop adds k* + 1 >= 1 to i and ends at i >= m
// or at corner_len corners; the chunk loop takes at most ceil(max_look / 64) turns and a lane's walk at most dl steps.  No
// barrier, no LDS, no atomic.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::allowed;
using rdoom_dev::is_open;
using rdoom_dev::StraightenArgs;
using rdoom_dev::WalkLimits;
using rdoom_dev::WalkLinesArgs;

constexpr uint32_t WAVE = 64;
constexpr uint32_t THREADS = 256, WAVES = THREADS / WAVE;

// a line from cell a, inside the grid, to a cell inside the grid, as its steps see it: cell (L, j) -- L crossings of the longer
// axis made, j of the shorter -- is word at0 + L * long_step + j * short_step of the planes
struct Line {
  const float *floor, *ceiling;  // the row's planes
  uint32_t width;
  int32_t ca, ra;                  // a
  int32_t long_dc, long_dr;        // a crossing of the longer axis as (column, row): (+-1, 0) or (0, +-1)
  int32_t short_dc, short_dr;      // and one of the shorter axis
  uint32_t dl, ds;                 // their numbers: ds <= dl
};

__device__ __forceinline__ Line line_of(const float *floor, const float *ceiling, uint32_t width, int32_t ca, int32_t ra, int32_t cb, int32_t rb) {
  const int32_t sx = (cb > ca) - (cb < ca), sy = (rb > ra) - (rb < ra);
  const uint32_t dx = (uint32_t)(sx * (cb - ca)), dy = (uint32_t)(sy * (rb - ra));
  const bool across = dx >= dy;  // the longer axis is the columns'
  return Line{floor, ceiling, width, ca, ra, across ? sx : 0, across ? 0 : sy, across ? 0 : sx, across ? sy : 0, across ? dx : dy, across ? dy : dx};
}

// step L < dl of the line (the header's closed forms): true when its moves are allowed; otherwise (col, row) is the cell the first
// refused one starts from.  Every cell read lies in the box a and b span
template <bool REVERSED>
__device__ __forceinline__ bool test_step(const Line &ln, const WalkLimits &lim, uint32_t L, int32_t &col, int32_t &row) {
  const uint32_t two = 2u * ln.dl, N = (2u * L + 1u) * ln.ds + ln.dl;
  const uint32_t q = N / two, r = N - q * two;
  const bool corner = r == 0;
  const uint32_t before = q - (corner ? 1u : 0u);                          // short crossings strictly before long crossing L
  const uint32_t made = L == 0 ? 0u : q - (r < 2u * ln.ds ? 1u : 0u);    // and those at or before long crossing L - 1

  int32_t c = ln.ca + (int32_t)L * ln.long_dc + (int32_t)made * ln.short_dc, w = ln.ra + (int32_t)L * ln.long_dr + (int32_t)made * ln.short_dr;
  // the chain's move from cell (xc, xr) to cell (yc, yr)
  auto move = [&](int32_t xc, int32_t xr, int32_t yc, int32_t yr) {
    const uint32_t x = (uint32_t)xr * ln.width + (uint32_t)xc, y = (uint32_t)yr * ln.width + (uint32_t)yc;
    return REVERSED ? allowed(ln.floor[y], ln.ceiling[y], ln.floor[x], ln.ceiling[x], lim)
                    : allowed(ln.floor[x], ln.ceiling[x], ln.floor[y], ln.ceiling[y], lim);
  };
  col = c, row = w;
  if (made < before) {  // the one short crossing since the last long one
    if (!move(c, w, c + ln.short_dc, w + ln.short_dr)) return false;
    c += ln.short_dc, w += ln.short_dr;
    col = c, row = w;
  }
  const int32_t lc = c + ln.long_dc, lr = w + ln.long_dr;
  if (!corner) return move(c, w, lc, lr);
  const int32_t sc = c + ln.short_dc, sr = w + ln.short_dr, dc = lc + ln.short_dc, dr = lr + ln.short_dr;
  return move(c, w, lc, lr) && move(lc, lr, dc, dr) && move(c, w, sc, sr) && move(sc, sr, dc, dr);
}

// ---- rdoom_grid_walk_lines ----
template <bool REVERSED>
__device__ __forceinline__ void walk_line(const WalkLinesArgs &a) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t id = blockIdx.x * WAVES + threadIdx.x / WAVE;  // the wave's line: < 2^31 + WAVES
  if (id >= a.lines) return;
  const uint32_t p = id / a.n_to;
  const uint32_t W = a.width, H = a.height;
  const size_t grid = (size_t)p * W * H;
  const WalkLimits lim{a.max_step, a.max_drop, a.clearance};
  const int32_t ca = a.from[2 * (size_t)p], ra = a.from[2 * (size_t)p + 1];
  const int32_t cb = a.to[2 * (size_t)id], rb = a.to[2 * (size_t)id + 1];

  bool clear = false;
  int32_t stop_c = -1, stop_r = -1;
  if ((uint32_t)ca < W && (uint32_t)ra < H && (uint32_t)cb < W && (uint32_t)rb < H) {
    const Line ln = line_of(a.floor + grid, a.ceiling + grid, W, ca, ra, cb, rb);
    const uint32_t at = (uint32_t)ra * W + (uint32_t)ca;
    clear = is_open(ln.floor[at], ln.ceiling[at], lim.clearance);
    stop_c = ca, stop_r = ra;
    if (clear) {
      for (uint32_t base = 0; base < ln.dl; base += WAVE) {
        const uint32_t L = base + lane;
        int32_t c = 0, r = 0;
        const bool refused = L < ln.dl && !test_step<REVERSED>(ln, lim, L, c, r);
        const uint64_t refusals = __builtin_amdgcn_ballot_w64(refused);
        if (refusals) {
          const int first = __builtin_ctzll(refusals);
          stop_c = __shfl(c, first, WAVE), stop_r = __shfl(r, first, WAVE);
          clear = false;
          break;
        }
      }
      if (clear) stop_c = cb, stop_r = rb;
    }
  }
  if (lane == 0) {
    a.clear_out[id] = clear ? 1 : 0;
    if (a.stop_out) a.stop_out[2 * (size_t)id] = stop_c, a.stop_out[2 * (size_t)id + 1] = stop_r;
  }
}

__global__ __launch_bounds__(THREADS) void walk_lines_kernel(WalkLinesArgs a) { walk_line<false>(a); }
__global__ __launch_bounds__(THREADS) void walk_lines_reversed_kernel(WalkLinesArgs a) { walk_line<true>(a); }

// ---- rdoom_path_straighten ----
template <bool REVERSED>
__device__ __forceinline__ void straighten_row(const StraightenArgs &a) {
  const uint32_t lane = threadIdx.x & (WAVE - 1);
  const uint32_t p = blockIdx.x * WAVES + threadIdx.x / WAVE;  // the wave's row
  if (p >= a.n) return;
  const uint32_t W = a.width, H = a.height;
  const size_t grid = (size_t)p * W * H;
  const float *floor = a.floor + grid, *ceiling = a.ceiling + grid;
  const int32_t *path = a.path + (size_t)p * a.path_len * 2;
  int32_t *corners = a.corners_out + (size_t)p * a.corner_len * 2;
  const WalkLimits lim{a.max_step, a.max_drop, a.clearance};

  int32_t ca = a.starts[2 * (size_t)p], ra = a.starts[2 * (size_t)p + 1];
  uint32_t count = 0;
  float length = 0.0f;
  if ((uint32_t)ca < W && (uint32_t)ra < H) {
    // m: the entries before the first that is no cell of the grid
    uint32_t m = a.path_len;
    for (uint32_t base = 0; base < a.path_len; base += WAVE) {
      const uint32_t k = base + lane;
      const bool outside = k < a.path_len && !((uint32_t)path[2 * (size_t)k] < W && (uint32_t)path[2 * (size_t)k + 1] < H);
      const uint64_t ends = __builtin_amdgcn_ballot_w64(outside);
      if (ends) {
        m = base + (uint32_t)__builtin_ctzll(ends);
        break;
      }
    }
    uint32_t i = 0;
    while (i < m && count < a.corner_len) {
      const uint32_t at = (uint32_t)ra * W + (uint32_t)ca;
      if (!is_open(floor[at], ceiling[at], lim.clearance)) break;  // no line from a closed cell is clear
      const uint32_t K = min(a.max_look, m - i);
      uint32_t best = K;  // k*, or K: none
      for (uint32_t top = K; top > 0 && best == K;) {
        const uint32_t low = top > WAVE ? top - WAVE : 0u;
        const uint32_t k = low + lane;
        bool clear = k < top;
        if (clear) {
          const Line ln = line_of(floor, ceiling, W, ca, ra, path[2 * (size_t)(i + k)], path[2 * (size_t)(i + k) + 1]);
          int32_t c, r;
          for (uint32_t L = 0; L < ln.dl && clear; L++) clear = test_step<REVERSED>(ln, lim, L, c, r);
        }
        const uint64_t reached = __builtin_amdgcn_ballot_w64(clear);
        if (reached) best = low + 63u - (uint32_t)__builtin_clzll(reached);
        top = low;
      }
      if (best == K) break;
      const int32_t cc = path[2 * (size_t)(i + best)], cr = path[2 * (size_t)(i + best) + 1];
      const int32_t dc = cc - ca, dr = cr - ra;
      length += __builtin_sqrtf((float)(dc * dc + dr * dr));
      if (lane == 0) corners[2 * (size_t)count] = cc, corners[2 * (size_t)count + 1] = cr;
      ca = cc, ra = cr;
      i += best + 1u, count++;
    }
  }
  // the entries no corner filled: words 2 * count on, disjoint from the ones lane 0 stored in the loop
  for (size_t k = 2 * (size_t)count + lane; k < 2 * (size_t)a.corner_len; k += WAVE) corners[k] = -1;  // a lane a word
  if (lane == 0) {
    a.count_out[p] = count;
    if (a.length_out) a.length_out[p] = length;
  }
}

__global__ __launch_bounds__(THREADS) void path_straighten_kernel(StraightenArgs a) { straighten_row<false>(a); }
__global__ __launch_bounds__(THREADS) void path_straighten_reversed_kernel(StraightenArgs a) { straighten_row<true>(a); }

}  // namespace

extern "C" {

rdoom_status rdoom_grid_walk_lines(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                   const int32_t *d_from, const int32_t *d_to, uint32_t n_to, const rdoom_flood_params *params,
                                   uint8_t *d_clear_out, int32_t *d_stop_out, void *stream) {
  if (rdoom_status s = rdoom::check_walk_lines(params, n, d_floor && d_ceiling && d_from && d_to && d_clear_out, width, height, n_to)) return s;
  if (!n) return RDOOM_OK;
  const WalkLinesArgs a{d_floor, d_ceiling, d_from, d_to, d_clear_out, d_stop_out, n * n_to, n_to, width, height,
                        params->max_step, params->max_drop, params->clearance};
  const dim3 blocks((a.lines + WAVES - 1) / WAVES);
  if (params->flags & RDOOM_LINE_REVERSED) return rdoom::launch_checked(walk_lines_reversed_kernel, blocks, dim3(THREADS), 0, stream, a);
  return rdoom::launch_checked(walk_lines_kernel, blocks, dim3(THREADS), 0, stream, a);
}

rdoom_status rdoom_path_straighten(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                   const int32_t *d_starts, const int32_t *d_path, uint32_t path_len, const rdoom_flood_params *params,
                                   uint32_t max_look, int32_t *d_corners_out, uint32_t corner_len, uint32_t *d_count_out,
                                   float *d_length_out, void *stream) {
  if (rdoom_status s = rdoom::check_path_straighten(params, n, d_floor && d_ceiling && d_starts && d_path && d_corners_out && d_count_out, width,
                                                    height, path_len, max_look, corner_len))
    return s;
  if (!n) return RDOOM_OK;
  const StraightenArgs a{d_floor, d_ceiling, d_starts, d_path, d_corners_out, d_count_out, d_length_out, n, width, height, path_len, max_look,
                         corner_len, params->max_step, params->max_drop, params->clearance};
  const dim3 blocks((n + WAVES - 1) / WAVES);
  // a forward field's path is listed from the far end back to the player: its lines are walked against the listed direction
  if (params->flags & RDOOM_FLOOD_TOWARDS) return rdoom::launch_checked(path_straighten_kernel, blocks, dim3(THREADS), 0, stream, a);
  return rdoom::launch_checked(path_straighten_reversed_kernel, blocks, dim3(THREADS), 0, stream, a);
}

}  // extern "C"
