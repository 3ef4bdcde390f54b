// RGB resolve (rdoom_batch_resolve_rgb): the frames of a batch's last render as RGB8 / RGBA8, the colours the reference's
// window shows -- PLAYPAL 0 of the pose's level where a primitive was drawn (static.frag / sky.frag / sprite.frag end in
// texture(u_palette, ...).rgb), the GL clear colour (0.06, 0.07, 0.09) = (15, 18, 23) where nothing was (window.rs:40-44).
//
// Coverage -- drawn or clear -- comes from what the render leaves on the device, by render_walk.hpp's walk: the quadrant table
// (an entry that is a record, QTAB_HANDLED or not = every pixel drawn), the visibility words, then the fixup list, whose pixels
// resolve_fix_kernel rewrites from vis[o] and fb[o].
//
// Bandwidth-bound: 1 B/px of palette indices read, 3-4 B/px written, 2 B/px of visibility words read only in quadrants the
// table does not describe.  A wave resolves one 32 x 32 quadrant, 16 pixels a lane (one 16-byte index load, 48 / 64 bytes
// stored), so the table entry is one scalar load and a described quadrant issues no visibility-word loads at all.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "render_walk.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {
namespace {

constexpr uint32_t CLEAR_WORD = RDOOM_CLEAR_R | (RDOOM_CLEAR_G << 8) | (RDOOM_CLEAR_B << 16);  // alpha 0, as the clear colour's

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

template <int BPP, bool VIS16>
__global__ __launch_bounds__(256) void resolve_kernel(const uint8_t *__restrict__ fb, const void *__restrict__ vis,
                                                      const uint32_t *__restrict__ qtab, const PoseConst *__restrict__ poses,
                                                      const uint32_t *__restrict__ palettes, uint8_t *__restrict__ out,
                                                      uint32_t first, uint32_t groups_x, uint32_t groups_per_frame,
                                                      uint32_t width, uint32_t pitch, uint32_t height, uint32_t tiles_x,
                                                      uint32_t n_tiles, uint32_t flags) {
  __shared__ uint32_t pal[256];
  const WalkLane l = walk_lane(first, groups_x, groups_per_frame);
  pal[threadIdx.x] = palettes[(size_t)poses[l.pose].level * 256u + threadIdx.x];  // the pose's PLAYPAL 0, staged once
  __syncthreads();
  const uint32_t qx = l.qx, x0 = l.x0;
  if (qx * 32u >= width) return;  // (wave-uniform; no barrier follows)
  const size_t frame = (size_t)pitch * height;
  const uint8_t *pfb = fb + (size_t)l.pose * frame;
  const void *pvis = vis_of_pose<VIS16>(vis, l.pose, frame);
  for (uint32_t k = 0; k < WALK_QROWS; k++) {
    const uint32_t qy = l.gy * WALK_QROWS + k;
    if (qy * 32u >= height) break;
    const bool described = quadrant_entry(qtab, flags, l.pose, n_tiles, tiles_x, qx, qy) != NONE;
    const uint32_t y = qy * 32u + (l.lane >> 1);
    if (y >= height || x0 >= width) continue;
    const uint32_t yo = (flags & WF_TOP_DOWN) ? height - 1u - y : y;
    const size_t o = (size_t)y * pitch + x0;
    uint8_t *dst = out + (((size_t)l.f * height + yo) * width + x0) * BPP;
    if (x0 + 16u <= width) {
      const u32x4 idx = *reinterpret_cast<const u32x4_a4 *>(pfb + o);
      uint32_t drawn = 0xFFFFu;  // bit i: pixel x0 + i shows a primitive
      if (!described) drawn = vis_run_drawn<VIS16>(pvis, o);
      uint32_t c[16];
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint32_t p = pal[(idx[i >> 2] >> (8 * (i & 3))) & 0xFFu];  // (looked up whether drawn or not: no branch per pixel)
        c[i] = ((drawn >> i) & 1u) ? p : CLEAR_WORD;
      }
      store_run<BPP>(dst, c, (flags & WF_DWORD) != 0u);
    } else {  // the row's last pixels (a width that is not a multiple of 16)
      for (uint32_t i = 0; i < width - x0; i++) {
        const bool d = described || vis_word<VIS16>(pvis, o + i) != VisWord<VIS16>::none;
        store_pixel<BPP>(dst + i * BPP, d ? pal[pfb[o + i]] : CLEAR_WORD);
      }
    }
  }
}

// Runs after resolve_kernel on the same stream and overwrites what the table said for the fixup list's pixels.
template <int BPP, bool VIS16>
__global__ __launch_bounds__(256) void resolve_fix_kernel(const uint8_t *__restrict__ fb, const void *__restrict__ vis,
                                                          const PoseConst *__restrict__ poses, const uint32_t *__restrict__ palettes,
                                                          const uint32_t *__restrict__ fix_count, const uint2 *__restrict__ fix_list,
                                                          uint32_t fix_cap, uint8_t *__restrict__ out, uint32_t first,
                                                          uint32_t count, uint32_t width, uint32_t pitch, uint32_t height,
                                                          uint32_t flags) {
  walk_fix_list<VIS16>(vis, fix_count, fix_list, fix_cap, first, count, width, pitch, height,
                       [&](uint32_t pose, uint32_t x, uint32_t y, uint32_t, bool drawn) {
                         const size_t o = (size_t)pose * pitch * height + (y * pitch + x);
                         const uint32_t c = drawn ? palettes[(size_t)poses[pose].level * 256u + fb[o]] : CLEAR_WORD;
                         const uint32_t yo = (flags & WF_TOP_DOWN) ? height - 1u - y : y;
                         store_pixel<BPP>(out + (((size_t)(pose - first) * height + yo) * width + x) * BPP, c);
                       });
}

template <int BPP, bool VIS16>
void launch_pair(hipStream_t st, const ResolveArgs &a, const WalkLaunch &g) {
  hipLaunchKernelGGL((resolve_kernel<BPP, VIS16>), dim3(g.grid), dim3(256), 0, st, a.fb, a.vis, a.qtab, a.poses, a.palettes, a.out,
                     a.first, g.groups_x, g.groups_per_frame, a.width, a.pitch, a.height, g.tiles_x, g.n_tiles, g.flags);
  hipLaunchKernelGGL((resolve_fix_kernel<BPP, VIS16>), dim3(64), dim3(256), 0, st, a.fb, a.vis, a.poses, a.palettes, a.fix_count,
                     a.fix_list, a.fix_cap, a.out, a.first, a.count, a.width, a.pitch, a.height, g.flags);
}

}  // namespace

rdoom_status launch_resolve(hipStream_t st, const ResolveArgs &a) {
  if (a.count == 0) return RDOOM_OK;
  const bool dword = ((uintptr_t)a.out & 3u) == 0u && (a.bpp == 4u || a.width % 4 == 0);
  WalkLaunch g;
  if (rdoom_status rs = walk_launch(a, "resolve", dword, &g)) return rs;
  if (a.bpp == 4u)
    a.vis16 ? launch_pair<4, true>(st, a, g) : launch_pair<4, false>(st, a, g);
  else
    a.vis16 ? launch_pair<3, true>(st, a, g) : launch_pair<3, false>(st, a, g);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // namespace rdoom_dev

