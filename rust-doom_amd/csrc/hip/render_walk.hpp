// How the read-back passes walk what a render leaves on the device: resolve.hip (RGB), planes.hip (depth, label, primitive id and
// the thing plane) and observe.hip (reduced colour and depth) find a pixel's winning record by one rule, defined here once:
//   1. the quadrant table, when the render's plan left out the visibility words of described quadrants
//      (FragmentPlan::skip_described_vis): the entry IS the record of every pixel of the quadrant, so its index is wave-uniform and
//      the record's words come by scalar loads; the visibility words under it are another render's and are never read;
//   2. otherwise the pixel's visibility word (NONE = nothing drawn);
//   3. then the alpha-leak fixup list: fixup_kernel left the final record of exactly those pixels in vis[o] (and its index in
//      fb[o]), also inside described quadrants (raster.hip: RASTER_MASKED_BORDER), so a second kernel rewrites them from there.
// Grid of a main pass: per frame, groups_x x row_groups workgroups; a workgroup = 4 waves = 4 quadrants of 32 x 32 side by side,
// WALK_QROWS rows of them; two lanes a row of the quadrant, a run of 16 pixels a lane.  The frame source every pass takes from a
// batch (FrameSource) is kernels.hpp's, with the argument structs that derive from it.  One definition each, for
// player_quat.hpp's reason.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace rdoom_dev {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // 16-byte accesses at dword alignment: tight rows, pitches that are multiples of 4

constexpr uint32_t WALK_QROWS = 4;  // quadrant rows per workgroup (one palette staging per 16 K pixels)
constexpr uint32_t WF_QTAB = 1u, WF_TOP_DOWN = 2u, WF_DWORD = 4u;  // the flags word of both kernels of a pass

// ---- the host's side: the launch geometry of a main pass ----------------------------------------------------------------------
struct WalkLaunch {
  uint32_t tiles_x, n_tiles, groups_x, groups_per_frame, grid, flags;
};

// `what`: the caller's noun for the refusal; `dword`: the pass may store its runs as dwords (WF_DWORD)
inline rdoom_status walk_launch(const FrameSource &s, const char *what, bool dword, WalkLaunch *out) {
  const uint32_t tiles_x = (s.width + TILE_W - 1u) / TILE_W, tiles_y = (s.height + TILE_H - 1u) / TILE_H;
  const uint32_t groups_x = (s.width + 127u) / 128u;
  const uint32_t row_groups = (s.height + 32u * WALK_QROWS - 1u) / (32u * WALK_QROWS);
  const uint32_t groups_per_frame = groups_x * row_groups;
  const uint64_t grid = (uint64_t)groups_per_frame * s.count;
  if (grid > 0x7FFFFFFFull) return rdoom::fail(RDOOM_BAD_ARG, "%s of %u frames too large for one launch", what, s.count);
  const uint32_t flags = (s.use_qtab ? WF_QTAB : 0u) | (s.top_down ? WF_TOP_DOWN : 0u) | (dword ? WF_DWORD : 0u);
  *out = WalkLaunch{tiles_x, tiles_x * tiles_y, groups_x, groups_per_frame, (uint32_t)grid, flags};
  return RDOOM_OK;
}

// ---- a lane's place ------------------------------------------------------------------------------------------------------------
struct WalkLane {
  uint32_t f, pose;  // frame of the range, pose of the batch
  uint32_t gy, qx;   // row group of the frame; quadrant column (the wave's: uniform).  The wave is outside when qx * 32 >= width
  uint32_t lane, x0; // lane of the wave; first column of the lane's run
};

__device__ __forceinline__ WalkLane walk_lane(uint32_t first, uint32_t groups_x, uint32_t groups_per_frame) {
  WalkLane l;
  l.f = blockIdx.x / groups_per_frame;
  const uint32_t g = blockIdx.x - l.f * groups_per_frame;
  l.pose = first + l.f;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  l.lane = threadIdx.x & 63u;
  l.gy = g / groups_x;
  l.qx = (g - l.gy * groups_x) * 4u + wave;
  l.x0 = l.qx * 32u + (l.lane & 1u) * 16u;  // two lanes per row of the quadrant, 32 rows
  return l;
}

// the table's entry of quadrant (qx, qy) of a pose's frame, NONE where the table is not used: a described quadrant has no
// visibility words of this render.  pose < the batch's poses, the quadrant inside the frame.
__device__ __forceinline__ uint32_t quadrant_entry(const uint32_t *__restrict__ qtab, uint32_t flags, uint32_t pose, uint32_t n_tiles,
                                                   uint32_t tiles_x, uint32_t qx, uint32_t qy) {
  if (!(flags & WF_QTAB)) return NONE;
  return qtab[((size_t)pose * n_tiles + (qy >> 1) * tiles_x + (qx >> 1)) * 4u + (qy & 1u) * 2u + (qx & 1u)];
}

// ---- visibility words of either width; o counts words ------------------------------------------------------------------------
template <bool VIS16>
struct VisWord {
  static constexpr uint32_t none = VIS16 ? 0xFFFFu : NONE;  // nothing drawn
};

template <bool VIS16>
__device__ __forceinline__ uint32_t vis_word(const void *__restrict__ vis, size_t o) {
  return VIS16 ? (uint32_t)reinterpret_cast<const uint16_t *>(vis)[o] : reinterpret_cast<const uint32_t *>(vis)[o];
}

// the first word of a pose's frame (frame = pitch * height words)
template <bool VIS16>
__device__ __forceinline__ const void *vis_of_pose(const void *__restrict__ vis, uint32_t pose, size_t frame) {
  return reinterpret_cast<const uint8_t *>(vis) + (size_t)pose * frame * (VIS16 ? 2u : 4u);
}

// a lane's run: the 16 words from o on (o a multiple of 4 words)
template <bool VIS16>
__device__ __forceinline__ void vis_run(const void *__restrict__ vis, size_t o, uint32_t (&w)[16]) {
  if (VIS16) {
    const uint16_t *p = reinterpret_cast<const uint16_t *>(vis) + o;
    const u32x4 a = *reinterpret_cast<const u32x4_a4 *>(p), b = *reinterpret_cast<const u32x4_a4 *>(p + 8);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t ww = i < 4 ? a[i] : b[i - 4];
      w[2 * i] = ww & 0xFFFFu, w[2 * i + 1] = ww >> 16;
    }
  } else {
    const uint32_t *p = reinterpret_cast<const uint32_t *>(vis) + o;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const u32x4 ww = *reinterpret_cast<const u32x4_a4 *>(p + 4 * j);
#pragma unroll
      for (int i = 0; i < 4; i++) w[4 * j + i] = ww[i];
    }
  }
}

// bit i: pixel i of that run shows a primitive
template <bool VIS16>
__device__ __forceinline__ uint32_t vis_run_drawn(const void *__restrict__ vis, size_t o) {
  uint32_t w[16], drawn = 0u;
  vis_run<VIS16>(vis, o, w);
#pragma unroll
  for (int i = 0; i < 16; i++) drawn |= (w[i] != VisWord<VIS16>::none ? 1u : 0u) << i;
  return drawn;
}

// ---- the fixup list ------------------------------------------------------------------------------------------------------------
// The body of a pass's second kernel (64 workgroups of 256 threads, after the main kernel on the same stream): use(pose, x, y, word,
// drawn) for every pixel fixup_kernel re-resolved in frames [first, first + count) -- its final record is `word` = vis[o], its index
// in fb[o], o = pose * pitch * height + (y * pitch + x), the sum in brackets being the item's word as it stands.  pose is a pose of
// the range, so below the batch's poses.
template <bool VIS16, class Use>
__device__ __forceinline__ void walk_fix_list(const void *__restrict__ vis, const uint32_t *__restrict__ fix_count,
                                              const uint2 *__restrict__ fix_list, uint32_t fix_cap, uint32_t first, uint32_t count,
                                              uint32_t width, uint32_t pitch, uint32_t height, Use use) {
  const uint32_t total = *fix_count;
  if (total > fix_cap) return;  // fixup_kernel did not run: the render's status says so (device_flags)
  for (uint32_t item = blockIdx.x * 256u + threadIdx.x; item < total; item += gridDim.x * 256u) {
    const uint2 it = fix_list[item];  // (pose, row * pitch + column)
    if (it.x - first >= count) continue;
    const uint32_t y = it.y / pitch, x = it.y - y * pitch;
    if (x >= width || y >= height) continue;
    const uint32_t w = vis_word<VIS16>(vis, (size_t)it.x * pitch * height + it.y);
    use(it.x, x, y, w, w != VisWord<VIS16>::none);
  }
}

}  // namespace rdoom_dev
