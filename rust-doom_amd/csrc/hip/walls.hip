// Wall distance (include/rdoom.h "wall distance"): the squared distance, in cells, from every cell of a grid of
// floor and ceiling planes to the nearest blocking cell, exact up to a radius R and capped there, and the same planes with every
// cell within sqrt(close_d2) of a blocking cell made void (rdoom_wall_distance).  It reads the planes the floods read and nothing
// else: no world handle, no table.
//
// Arithmetic: the one float operation is the contract's "Open", world_shared.hpp's, the one the floods use; the build passes
// -ffp-contract=off.  Everything after it is integers.
//
// wall_distance_kernel: one 256-thread workgroup per WALL_TILE_X x WALL_TILE_Y tile of one row's grid.  The exact transform is
// separable, and the cap makes both phases local to the tile and a halo of R cells on every side:
//   staging  the open byte of every cell of the tile and its halo, (TX + 2R) x (TY + 2R) of them, computed once from the two floats;
//            a cell outside the grid is blocking, or open with RDOOM_WALL_EDGE_OPEN.  Lanes take consecutive columns.
//   phase 1  g(x, y), for every column x of the haloed tile and every row y of the tile: the vertical distance to the nearest
//            blocking cell of the column, R + 1 where there is none within R.  A thread owns SEG rows of one column and runs down
//            them from R rows above, counting the cells since the last blocking one, then up them from R rows below: 2 (R + SEG)
//            steps, whatever the data.  Only the owner touches its g, so the two runs need no barrier between them.
//   phase 2  D2(x, y) = min over |dx| <= R of dx * dx + g(x + dx, y)^2, a lane a column, a wave a row at a time.  A g of R + 1
//            gives a term above R * R, which is reported as RDOOM_WALL_FAR like every other value above R * R, so "none within R"
//            needs no case of its own.  The 64 lanes of a wave read 64 consecutive bytes of one row of g: sixteen banks, four
//            lanes to a word, no conflict.
// Then the stores: a lane a column, so the 16-bit distances and the plane words of a row go out as whole lines.  The plane words
// of the tile's own cells are loaded a second time here, as words, rather than kept from staging: they were read by this workgroup
// a moment ago and the tile is 16 KiB, so the load is served by the cache, and keeping them would double the LDS.
// Termination: every loop's bound is a function of R and the tile's constants; there is no data-dependent exit, no atomic, and no
// word one workgroup writes is read by another.  The two barriers stand outside every condition: every thread reaches both.
#include <hip/hip_runtime.h>

#include "../common.hpp"
#include "kernels.hpp"
#include "world_shared.hpp"

#pragma clang fp contract(off)

namespace {

using rdoom_dev::is_open;
using rdoom_dev::WallArgs;

constexpr uint32_t WAVE = 64, THREADS = 256;
constexpr uint32_t TX = rdoom_dev::WALL_TILE_X, TY = rdoom_dev::WALL_TILE_Y;
constexpr uint32_t RMAX = RDOOM_WALL_MAX_RADIUS;
constexpr uint32_t SEG = 8;  // rows of a column one thread owns in phase 1
constexpr uint32_t MAX_BLOCKS = 0xFFFFFFu;  // workgroups of one launch: blocks x threads stays below 2^32
static_assert(TX == WAVE && TY % SEG == 0 && TY % (THREADS / WAVE) == 0, "wall_distance: a lane a column, whole segments, whole waves");
static_assert(RMAX + 1 <= 0xFF && 2 * (RMAX + 1) * (RMAX + 1) < RDOOM_WALL_FAR, "wall_distance: g fits a byte, a term fits the output");
static_assert((TX + 2 * RMAX) * (TY + 2 * RMAX) + (TX + 2 * RMAX) * TY <= 64 * 1024, "wall_distance: the largest radius fits the LDS");

__global__ __launch_bounds__(THREADS) void wall_distance_kernel(WallArgs a) {
  __shared__ uint8_t open_s[(TX + 2 * RMAX) * (TY + 2 * RMAX)];  // 1: the cell does not block; pitch TX + 2R
  __shared__ uint8_t g_s[(TX + 2 * RMAX) * TY];                  // phase 1's g; pitch TX + 2R

  const uint32_t tid = threadIdx.x;
  const uint32_t W = a.width, H = a.height, R = a.radius;
  const uint32_t p = blockIdx.x / a.tiles, t = blockIdx.x - p * a.tiles;
  const uint32_t ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
  const uint32_t x0 = tx * TX, y0 = ty * TY;  // the tile's first cell: inside the grid
  const uint32_t HW = TX + 2 * R, HH = TY + 2 * R;
  const size_t grid = (size_t)p * W * H;
  const float *floor = a.floor + grid, *ceiling = a.ceiling + grid;

  // staging: haloed cell (hx, hy) is grid cell (x0 + hx - R, y0 + hy - R), modulo 2^32, so a cell before the grid is far above W, H
  for (uint32_t i = tid; i < HW * HH; i += THREADS) {
    const uint32_t hy = i / HW, hx = i - hy * HW;
    const uint32_t gx = x0 + hx - R, gy = y0 + hy - R;
    bool open = a.edge_open != 0;
    if (gx < W && gy < H) {
      const uint32_t at = gy * W + gx;
      open = is_open(floor[at], ceiling[at], a.clearance);
    }
    open_s[i] = open ? 1 : 0;
  }
  __syncthreads();

  // phase 1: column hx of the haloed tile, rows ys .. ys + SEG - 1 of the tile (haloed rows ys + R ..)
  const uint32_t far = R + 1;
  for (uint32_t it = tid; it < HW * (TY / SEG); it += THREADS) {
    const uint32_t seg = it / HW, hx = it - seg * HW;
    const uint32_t ys = seg * SEG;
    uint32_t d = far;
    for (uint32_t k = 0; k < R + SEG; k++) {  // downwards from haloed row ys, the tile's row ys - R
      d = open_s[(ys + k) * HW + hx] ? min(d + 1u, far) : 0u;
      if (k >= R) g_s[(ys + k - R) * HW + hx] = (uint8_t)d;
    }
    d = far;
    for (uint32_t k = 0; k < R + SEG; k++) {  // upwards from haloed row ys + SEG - 1 + 2R, the tile's row ys + SEG - 1 + R
      d = open_s[(ys + SEG - 1 + 2 * R - k) * HW + hx] ? min(d + 1u, far) : 0u;
      if (k >= R) {
        const uint32_t at = (ys + SEG - 1 + R - k) * HW + hx;
        g_s[at] = (uint8_t)min((uint32_t)g_s[at], d);
      }
    }
  }
  __syncthreads();

  // phase 2 and the stores: lane = column, the wave's rows wave, wave + 4, ...
  const uint32_t lane = tid & (WAVE - 1), gx = x0 + lane;
  const uint32_t r2 = R * R;
  for (uint32_t y = tid / WAVE; y < TY; y += THREADS / WAVE) {
    const uint32_t gy = y0 + y;
    if (gy >= H) break;  // (wave-uniform, and no barrier follows)
    const uint8_t *row = g_s + y * HW + lane;  // row[dx] is g(lane + dx - R, y)
    uint32_t d2 = 0xFFFFFFFFu;
    for (uint32_t dx = 0; dx <= 2 * R; dx++) {
      const uint32_t g = row[dx], off = dx > R ? dx - R : R - dx;
      d2 = min(d2, off * off + g * g);
    }
    if (gx >= W) continue;
    const size_t at = grid + (size_t)gy * W + gx;
    if (a.dist2_out) a.dist2_out[at] = d2 <= r2 ? (uint16_t)d2 : (uint16_t)RDOOM_WALL_FAR;
    if (a.floor_out) {
      // the words as they are, a NaN's payload and a zero's sign with them
      const uint32_t f = ((const uint32_t *)a.floor)[at], c = ((const uint32_t *)a.ceiling)[at];
      const bool shut = d2 <= a.close_d2;
      ((uint32_t *)a.floor_out)[at] = shut ? 0x7F800000u : f;    // +inf
      ((uint32_t *)a.ceiling_out)[at] = shut ? 0xFF800000u : c;  // -inf
    }
  }
}

// whether [a, a + bytes) and [b, b + bytes) share a byte
bool overlap(const void *a, const void *b, uint64_t bytes) {
  const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

}  // namespace

extern "C" {

rdoom_status rdoom_wall_distance(const float *d_floor, const float *d_ceiling, uint32_t n, uint32_t width, uint32_t height,
                                 const rdoom_wall_params *params, uint16_t *d_dist2_out, float *d_floor_out, float *d_ceiling_out,
                                 void *stream) {
  if (!params) return rdoom::fail(RDOOM_BAD_ARG, "null params");
  if (n && (!d_floor || !d_ceiling)) return rdoom::fail(RDOOM_BAD_ARG, "null floor or ceiling with n = %u", n);
  if (!d_dist2_out && !d_floor_out && !d_ceiling_out) return rdoom::fail(RDOOM_BAD_ARG, "no output: distances, or both planes, or all three");
  if (!d_floor_out != !d_ceiling_out) return rdoom::fail(RDOOM_BAD_ARG, "one output plane without the other: both or neither");
  if (!width || !height) return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells (at least 1 a side)", width, height);
  if (width > RDOOM_AREA_MAX_SIDE || height > RDOOM_AREA_MAX_SIDE)
    return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells: a side is at most %u", width, height, RDOOM_AREA_MAX_SIDE);
  uint32_t max_cells = 0;
  if (rdoom_status s = rdoom_flood_grid_max_cells(&max_cells)) return s;
  if ((uint64_t)width * height > max_cells)
    return rdoom::fail(RDOOM_BAD_ARG, "a grid of %u x %u cells: too many (at most %u)", width, height, max_cells);
  if (params->radius < 1 || params->radius > RDOOM_WALL_MAX_RADIUS)
    return rdoom::fail(RDOOM_BAD_ARG, "a radius of %u cells: 1 to %u", params->radius, RDOOM_WALL_MAX_RADIUS);
  if (params->close_d2 > params->radius * params->radius)
    return rdoom::fail(RDOOM_BAD_ARG, "close_d2 %u is above the radius squared, %u: nothing beyond the radius is known", params->close_d2,
                       params->radius * params->radius);
  if (params->flags & ~RDOOM_WALL_EDGE_OPEN) return rdoom::fail(RDOOM_BAD_ARG, "wall flags 0x%x: 0 or RDOOM_WALL_EDGE_OPEN", params->flags);
  if (!(params->clearance >= 0.0f)) return rdoom::fail(RDOOM_BAD_ARG, "clearance %g: not a number or negative", (double)params->clearance);
  const uint32_t tiles_x = (width + TX - 1) / TX, tiles = tiles_x * ((height + TY - 1) / TY);
  if ((uint64_t)n * tiles > MAX_BLOCKS)
    return rdoom::fail(RDOOM_BAD_ARG, "%u grids of %u tiles: too many for one launch (at most %u tiles)", n, tiles, MAX_BLOCKS);
  const uint64_t bytes = (uint64_t)n * width * height * sizeof(float);
  for (const float *out : {d_floor_out, d_ceiling_out})
    if (out && bytes && (overlap(out, d_floor, bytes) || overlap(out, d_ceiling, bytes)))
      return rdoom::fail(RDOOM_BAD_ARG, "an output plane overlaps an input plane: the kernel reads neighbours, there is no in-place form");
  if (!n) return RDOOM_OK;
  const WallArgs a{d_floor, d_ceiling, d_dist2_out, d_floor_out, d_ceiling_out, width, height, tiles_x, tiles, params->radius, params->close_d2,
                   params->flags & RDOOM_WALL_EDGE_OPEN, params->clearance};
  return rdoom::launch_checked(wall_distance_kernel, dim3(n * tiles), dim3(THREADS), 0, stream, a);
}

}  // extern "C"
