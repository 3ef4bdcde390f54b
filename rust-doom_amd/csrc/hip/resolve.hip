// RGB resolve (rdoom_batch_resolve_rgb): the frames of a batch's last render as RGB8 / RGBA8, the colours the reference's
// window shows -- PLAYPAL 0 of the pose's level where a primitive was drawn (static.frag / sky.frag / sprite.frag end in
// texture(u_palette, ...).rgb), the GL clear colour (0.06, 0.07, 0.09) = (15, 18, 23) where nothing was (window.rs:40-44).
//
// Coverage comes from what the render leaves on the device, read the way fragment_kernel reads it:
//   1. the quadrant table, when the render's plan left out the visibility words of described quadrants
//      (FragmentPlan::skip_described_vis): an entry that is a record (QTAB_HANDLED or not) = every pixel drawn; the visibility
//      words under it are another render's and are never read;
//   2. otherwise the pixel's visibility word (NONE = background);
//   3. then the alpha-leak fixup list: fixup_kernel wrote the final record of exactly those pixels into vis[o] and fb[o] --
//      also inside described quadrants (raster.hip: RASTER_MASKED_BORDER) -- so resolve_fix_kernel rewrites them from there.
//
// Bandwidth-bound: 1 B/px of palette indices read, 3-4 B/px written, 2 B/px of visibility words read only in quadrants the
// table does not describe.  A wave resolves one 32 x 32 quadrant, 16 pixels a lane (one 16-byte index load, 48 / 64 bytes
// stored), so the table entry is one scalar load and a described quadrant issues no visibility-word loads at all.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {
namespace {

constexpr uint32_t CLEAR_WORD = RDOOM_CLEAR_R | (RDOOM_CLEAR_G << 8) | (RDOOM_CLEAR_B << 16);  // alpha 0, as the clear colour's
constexpr uint32_t RESOLVE_QROWS = 4;  // quadrant rows per workgroup (one palette staging per 16 K pixels)
constexpr uint32_t RF_QTAB = 1u, RF_TOP_DOWN = 2u, RF_DWORD = 4u;  // resolve flags

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // 16-byte accesses at dword alignment: rows of any pitch that is a multiple of 4

template <int BPP>
__device__ __forceinline__ void store_pixel(uint8_t *p, uint32_t c) {
  p[0] = (uint8_t)c;
  p[1] = (uint8_t)(c >> 8);
  p[2] = (uint8_t)(c >> 16);
  if (BPP == 4) p[3] = (uint8_t)(c >> 24);
}

// 16 pixels a lane: c[i] = R | G << 8 | B << 16 | A << 24.  RGB8 packs four pixels into three dwords.
template <int BPP>
__device__ __forceinline__ void store_run(uint8_t *dst, const uint32_t (&c)[16], bool dword) {
  if (!dword) {  // (RGB8 rows of a width that is not a multiple of 4, or an output that is not dword aligned)
#pragma unroll
    for (int i = 0; i < 16; i++) store_pixel<BPP>(dst + i * BPP, c[i]);
    return;
  }
  u32x4_a4 *d = reinterpret_cast<u32x4_a4 *>(dst);
  if (BPP == 4) {
#pragma unroll
    for (int g = 0; g < 4; g++) d[g] = u32x4{c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
  } else {
    uint32_t w[12];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const uint32_t p0 = c[4 * g], p1 = c[4 * g + 1], p2 = c[4 * g + 2], p3 = c[4 * g + 3];
      w[3 * g] = (p0 & 0xFFFFFFu) | (p1 << 24);
      w[3 * g + 1] = ((p1 >> 8) & 0xFFFFu) | (p2 << 16);
      w[3 * g + 2] = ((p2 >> 16) & 0xFFu) | (p3 << 8);
    }
#pragma unroll
    for (int g = 0; g < 3; g++) d[g] = u32x4{w[4 * g], w[4 * g + 1], w[4 * g + 2], w[4 * g + 3]};
  }
}

// grid: per frame, groups_x x row_groups workgroups; a workgroup = 4 waves = 4 quadrants side by side, RESOLVE_QROWS rows of them
template <int BPP, bool VIS16>
__global__ __launch_bounds__(256) void resolve_kernel(const uint8_t *__restrict__ fb, const void *__restrict__ vis,
                                                      const uint32_t *__restrict__ qtab, const PoseConst *__restrict__ poses,
                                                      const uint32_t *__restrict__ palettes, uint8_t *__restrict__ out,
                                                      uint32_t first, uint32_t groups_x, uint32_t groups_per_frame,
                                                      uint32_t width, uint32_t pitch, uint32_t height, uint32_t tiles_x,
                                                      uint32_t n_tiles, uint32_t flags) {
  __shared__ uint32_t pal[256];
  const uint32_t f = blockIdx.x / groups_per_frame, g = blockIdx.x - f * groups_per_frame;
  const uint32_t pose = first + f;
  pal[threadIdx.x] = palettes[(size_t)poses[pose].level * 256u + threadIdx.x];  // the pose's PLAYPAL 0, staged once
  __syncthreads();
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
  const uint32_t qx = gx * 4u + wave;
  if (qx * 32u >= width) return;  // (wave-uniform; no barrier follows)
  const uint32_t x0 = qx * 32u + (lane & 1u) * 16u;  // two lanes per row of the quadrant, 32 rows
  const size_t frame = (size_t)pitch * height;
  const uint8_t *pfb = fb + (size_t)pose * frame;
  const uint16_t *pv16 = reinterpret_cast<const uint16_t *>(vis) + (size_t)pose * frame;
  const uint32_t *pv32 = reinterpret_cast<const uint32_t *>(vis) + (size_t)pose * frame;
  constexpr uint32_t NONE_ID = VIS16 ? 0xFFFFu : NONE;
  for (uint32_t k = 0; k < RESOLVE_QROWS; k++) {
    const uint32_t qy = gy * RESOLVE_QROWS + k;
    if (qy * 32u >= height) break;
    // the table first: a described quadrant has no visibility words of this render
    uint32_t ent = NONE;
    if (flags & RF_QTAB) ent = qtab[((size_t)pose * n_tiles + (qy >> 1) * tiles_x + (qx >> 1)) * 4u + (qy & 1u) * 2u + (qx & 1u)];
    const bool described = ent != NONE;
    const uint32_t y = qy * 32u + (lane >> 1);
    if (y >= height || x0 >= width) continue;
    const uint32_t yo = (flags & RF_TOP_DOWN) ? height - 1u - y : y;
    const size_t o = (size_t)y * pitch + x0;
    uint8_t *dst = out + (((size_t)f * height + yo) * width + x0) * BPP;
    if (x0 + 16u <= width) {
      const u32x4 idx = *reinterpret_cast<const u32x4_a4 *>(pfb + o);
      uint32_t drawn = 0xFFFFu;  // bit i: pixel x0 + i shows a primitive
      if (!described) {
        drawn = 0u;
        if (VIS16) {
          const u32x4 a = *reinterpret_cast<const u32x4_a4 *>(pv16 + o), b = *reinterpret_cast<const u32x4_a4 *>(pv16 + o + 8);
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const uint32_t w = i < 4 ? a[i] : b[i - 4];
            drawn |= ((w & 0xFFFFu) != NONE_ID ? 1u : 0u) << (2 * i);
            drawn |= ((w >> 16) != NONE_ID ? 1u : 0u) << (2 * i + 1);
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const u32x4 w = *reinterpret_cast<const u32x4_a4 *>(pv32 + o + 4 * j);
#pragma unroll
            for (int i = 0; i < 4; i++) drawn |= (w[i] != NONE_ID ? 1u : 0u) << (4 * j + i);
          }
        }
      }
      uint32_t c[16];
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint32_t p = pal[(idx[i >> 2] >> (8 * (i & 3))) & 0xFFu];  // (looked up whether drawn or not: no branch per pixel)
        c[i] = ((drawn >> i) & 1u) ? p : CLEAR_WORD;
      }
      store_run<BPP>(dst, c, (flags & RF_DWORD) != 0u);
    } else {  // the row's last pixels (a width that is not a multiple of 16)
      for (uint32_t i = 0; i < width - x0; i++) {
        const bool d = described || (VIS16 ? (uint32_t)pv16[o + i] : pv32[o + i]) != NONE_ID;
        store_pixel<BPP>(dst + i * BPP, d ? pal[pfb[o + i]] : CLEAR_WORD);
      }
    }
  }
}

// The pixels fixup_kernel re-resolved (its final record is in vis[o], its index in fb[o]), for the frames in range.  Runs after
// resolve_kernel on the same stream and overwrites what the table said for them.
template <int BPP, bool VIS16>
__global__ __launch_bounds__(256) void resolve_fix_kernel(const uint8_t *__restrict__ fb, const void *__restrict__ vis,
                                                          const PoseConst *__restrict__ poses, const uint32_t *__restrict__ palettes,
                                                          const uint32_t *__restrict__ fix_count, const uint2 *__restrict__ fix_list,
                                                          uint32_t fix_cap, uint8_t *__restrict__ out, uint32_t first,
                                                          uint32_t count, uint32_t width, uint32_t pitch, uint32_t height,
                                                          uint32_t flags) {
  const uint32_t total = *fix_count;
  if (total > fix_cap) return;  // fixup_kernel did not run: the render's status says so (device_flags)
  for (uint32_t item = blockIdx.x * 256u + threadIdx.x; item < total; item += gridDim.x * 256u) {
    const uint2 it = fix_list[item];  // (pose, row * pitch + column)
    if (it.x - first >= count) continue;
    const uint32_t y = it.y / pitch, x = it.y - y * pitch;
    if (x >= width || y >= height) continue;
    const size_t o = (size_t)it.x * pitch * height + it.y;
    const uint32_t v = VIS16 ? (uint32_t)reinterpret_cast<const uint16_t *>(vis)[o] : reinterpret_cast<const uint32_t *>(vis)[o];
    const uint32_t c = v != (VIS16 ? 0xFFFFu : NONE) ? palettes[(size_t)poses[it.x].level * 256u + fb[o]] : CLEAR_WORD;
    const uint32_t yo = (flags & RF_TOP_DOWN) ? height - 1u - y : y;
    store_pixel<BPP>(out + (((size_t)(it.x - first) * height + yo) * width + x) * BPP, c);
  }
}

template <int BPP, bool VIS16>
void launch_pair(hipStream_t st, uint32_t grid, const ResolveArgs &a, uint32_t groups_x, uint32_t groups_per_frame, uint32_t tiles_x,
                 uint32_t n_tiles, uint32_t flags) {
  hipLaunchKernelGGL((resolve_kernel<BPP, VIS16>), dim3(grid), dim3(256), 0, st, a.fb, a.vis, a.qtab, a.poses, a.palettes, a.out,
                     a.first, groups_x, groups_per_frame, (uint32_t)a.width, (uint32_t)a.pitch, (uint32_t)a.height, tiles_x, n_tiles,
                     flags);
  hipLaunchKernelGGL((resolve_fix_kernel<BPP, VIS16>), dim3(64), dim3(256), 0, st, a.fb, a.vis, a.poses, a.palettes, a.fix_count,
                     a.fix_list, a.fix_cap, a.out, a.first, a.count, (uint32_t)a.width, (uint32_t)a.pitch, (uint32_t)a.height, flags);
}

}  // namespace

rdoom_status launch_resolve(hipStream_t st, const ResolveArgs &a) {
  if (a.count == 0) return RDOOM_OK;
  const uint32_t tiles_x = ((uint32_t)a.width + TILE_W - 1u) / TILE_W, tiles_y = ((uint32_t)a.height + TILE_H - 1u) / TILE_H;
  const uint32_t groups_x = ((uint32_t)a.width + 127u) / 128u;
  const uint32_t row_groups = ((uint32_t)a.height + 32u * RESOLVE_QROWS - 1u) / (32u * RESOLVE_QROWS);
  const uint32_t groups_per_frame = groups_x * row_groups;
  const uint64_t grid = (uint64_t)groups_per_frame * a.count;
  if (grid > 0x7FFFFFFFull) return rdoom::fail(RDOOM_BAD_ARG, "resolve of %u frames too large for one launch", a.count);
  const bool dword = ((uintptr_t)a.out & 3u) == 0u && (a.bpp == 4u || a.width % 4 == 0);
  const uint32_t flags = (a.use_qtab ? RF_QTAB : 0u) | (a.top_down ? RF_TOP_DOWN : 0u) | (dword ? RF_DWORD : 0u);
  const uint32_t n_tiles = tiles_x * tiles_y;
  if (a.bpp == 4u)
    a.vis16 ? launch_pair<4, true>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags)
            : launch_pair<4, false>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags);
  else
    a.vis16 ? launch_pair<3, true>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags)
            : launch_pair<3, false>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // namespace rdoom_dev
