// Per-pixel planes of a batch's last render (rdoom_batch_resolve_plane): depth (the winning fragment's v_dist, binary32), label
// (kind | object id << 4, u16) and primitive id (u32).  A second resolve pass over what the render leaves on the device anyway;
// the render kernels are not involved and nobody who does not ask pays for it.
//
// The winning record of a pixel is found the way resolve.hip finds "drawn or clear":
//   1. the quadrant table, when the render's plan left out the visibility words of described quadrants: the entry IS the record
//      of every pixel of the quadrant, so its index is wave-uniform -- the record's words come by scalar loads and no
//      visibility word is read (those under a described quadrant are another render's);
//   2. otherwise the pixel's visibility word (NONE = nothing drawn).  A lane owns a run of 16 pixels; neighbours mostly share a
//      record, so a record is gathered only where the word differs from the previous pixel's;
//   3. then the alpha-leak fixup list: fixup_kernel left the final record of exactly those pixels in vis[o], also inside
//      described quadrants, so plane_fix_kernel rewrites them from there.
// What a record gives: RasterRec::flags (primitive id, kind), ShadeRec::wp (the 1/w plane: depth = 1 / plane at the pixel centre,
// F1 of DESIGN section 3 -- the bits texel_coords calls `dist`); the label's object id is LevelTri::packed of the primitive.
//
// Bandwidth-bound: 2-4 B/px written, 2 or 4 B/px of visibility words read outside described quadrants, plus the record gathers
// (one cache line per distinct record of a run).  No LDS, no scratch.  A wave resolves one 32 x 32 quadrant, two lanes a row.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "plane_record.hpp"  // RecVal, fetch_record, plane_value, DEPTH_FAR: shared with observe.hip

#pragma clang fp contract(off)

namespace rdoom_dev {
namespace {

constexpr uint32_t PLANE_QROWS = 4;  // quadrant rows per workgroup, as resolve.hip
constexpr uint32_t PF_QTAB = 1u, PF_TOP_DOWN = 2u, PF_DWORD = 4u;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // 16-byte accesses at dword alignment (tight rows of any width)

template <uint32_t PLANE>
struct PlaneOf;
template <>
struct PlaneOf<RDOOM_PLANE_DEPTH> {
  typedef uint32_t elem;  // (the float's bits)
  static constexpr uint32_t none = DEPTH_FAR;
};
template <>
struct PlaneOf<RDOOM_PLANE_LABEL> {
  typedef uint16_t elem;
  static constexpr uint32_t none = RDOOM_LABEL_NONE;
};
template <>
struct PlaneOf<RDOOM_PLANE_PRIMITIVE> {
  typedef uint32_t elem;
  static constexpr uint32_t none = NONE;
};

template <uint32_t PLANE>
__device__ __forceinline__ void store_run(typename PlaneOf<PLANE>::elem *dst, const uint32_t (&c)[16], bool dword) {
  if (sizeof(typename PlaneOf<PLANE>::elem) == 4) {  // rows of dwords are dword aligned whatever the width
    u32x4_a4 *d = reinterpret_cast<u32x4_a4 *>(dst);
#pragma unroll
    for (int g = 0; g < 4; g++) d[g] = u32x4{c[4 * g], c[4 * g + 1], c[4 * g + 2], c[4 * g + 3]};
  } else if (dword) {
    u32x4_a4 *d = reinterpret_cast<u32x4_a4 *>(dst);
#pragma unroll
    for (int g = 0; g < 2; g++)
      d[g] = u32x4{c[8 * g] | (c[8 * g + 1] << 16), c[8 * g + 2] | (c[8 * g + 3] << 16), c[8 * g + 4] | (c[8 * g + 5] << 16),
                   c[8 * g + 6] | (c[8 * g + 7] << 16)};
  } else {  // (u16 rows of an odd width: every other row starts on an odd halfword)
#pragma unroll
    for (int i = 0; i < 16; i++) dst[i] = (typename PlaneOf<PLANE>::elem)c[i];
  }
}

// grid: per frame, groups_x x row_groups workgroups; a workgroup = 4 waves = 4 quadrants side by side, PLANE_QROWS rows of them
template <uint32_t PLANE, bool VIS16>
__global__ __launch_bounds__(256) void plane_kernel(const void *__restrict__ vis, const uint32_t *__restrict__ qtab,
                                                    const PoseConst *__restrict__ poses, const TriRec *__restrict__ recs,
                                                    uint32_t cap, const LevelTri *__restrict__ tris,
                                                    const LevelSlice *__restrict__ slices,
                                                    typename PlaneOf<PLANE>::elem *__restrict__ out, uint32_t first,
                                                    uint32_t groups_x, uint32_t groups_per_frame, uint32_t width, uint32_t pitch,
                                                    uint32_t height, uint32_t tiles_x, uint32_t n_tiles, uint32_t flags) {
  typedef typename PlaneOf<PLANE>::elem elem;
  constexpr uint32_t NONE_VAL = PlaneOf<PLANE>::none;
  constexpr uint32_t NONE_ID = VIS16 ? 0xFFFFu : NONE;
  const uint32_t f = blockIdx.x / groups_per_frame, g = blockIdx.x - f * groups_per_frame;
  const uint32_t pose = first + f;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
  const uint32_t gy = g / groups_x, gx = g - gy * groups_x;
  const uint32_t qx = gx * 4u + wave;
  if (qx * 32u >= width) return;
  const uint32_t x0 = qx * 32u + (lane & 1u) * 16u;  // two lanes per row of the quadrant, 32 rows
  const size_t frame = (size_t)pitch * height;
  const uint16_t *pv16 = reinterpret_cast<const uint16_t *>(vis) + (size_t)pose * frame;
  const uint32_t *pv32 = reinterpret_cast<const uint32_t *>(vis) + (size_t)pose * frame;
  const TriRec *prec = recs + (size_t)pose * cap;
  const LevelTri *ptris = tris;
  if (PLANE == RDOOM_PLANE_LABEL) ptris = tris + slices[poses[pose].level].first_tri;  // (scalar loads: one pose per workgroup)
  for (uint32_t k = 0; k < PLANE_QROWS; k++) {
    const uint32_t qy = gy * PLANE_QROWS + k;
    if (qy * 32u >= height) break;
    // the table first: a described quadrant has no visibility words of this render
    uint32_t ent = NONE;
    if (flags & PF_QTAB) ent = qtab[((size_t)pose * n_tiles + (qy >> 1) * tiles_x + (qx >> 1)) * 4u + (qy & 1u) * 2u + (qx & 1u)];
    const bool described = ent != NONE;
    RecVal qrec{0.0f, 0.0f, 0.0f, 0u};
    if (described) {  // wave-uniform: the record's words by scalar loads
      const uint32_t rec = min((uint32_t)__builtin_amdgcn_readfirstlane((int)(ent & ENTRY_REC_MASK)), cap - 1u);
      qrec = fetch_record<PLANE>(prec, rec, ptris);
    }
    const uint32_t y = qy * 32u + (lane >> 1);
    if (y >= height || x0 >= width) continue;
    const uint32_t yo = (flags & PF_TOP_DOWN) ? height - 1u - y : y;
    const size_t o = (size_t)y * pitch + x0;
    const float py = (float)y + 0.5f;
    elem *dst = out + ((size_t)f * height + yo) * width + x0;
    if (x0 + 16u <= width) {
      uint32_t c[16];
      if (described) {
#pragma unroll
        for (int i = 0; i < 16; i++) c[i] = plane_value<PLANE>(qrec, (float)(x0 + i) + 0.5f, py);
      } else {
        uint32_t w[16];
        if (VIS16) {
          const u32x4 a = *reinterpret_cast<const u32x4_a4 *>(pv16 + o), b = *reinterpret_cast<const u32x4_a4 *>(pv16 + o + 8);
#pragma unroll
          for (int i = 0; i < 8; i++) {
            const uint32_t ww = i < 4 ? a[i] : b[i - 4];
            w[2 * i] = ww & 0xFFFFu, w[2 * i + 1] = ww >> 16;
          }
        } else {
#pragma unroll
          for (int j = 0; j < 4; j++) {
            const u32x4 ww = *reinterpret_cast<const u32x4_a4 *>(pv32 + o + 4 * j);
#pragma unroll
            for (int i = 0; i < 4; i++) w[4 * j + i] = ww[i];
          }
        }
        uint32_t prev = NONE_ID;
        RecVal rv{0.0f, 0.0f, 0.0f, 0u};
#pragma unroll
        for (int i = 0; i < 16; i++) {
          if (w[i] != NONE_ID && w[i] != prev) {  // a new record in this run
            rv = fetch_record<PLANE>(prec, min(w[i], cap - 1u), ptris);
            prev = w[i];
          }
          c[i] = w[i] == NONE_ID ? NONE_VAL : plane_value<PLANE>(rv, (float)(x0 + i) + 0.5f, py);
        }
      }
      store_run<PLANE>(dst, c, (flags & PF_DWORD) != 0u);
    } else {  // the row's last pixels (a width that is not a multiple of 16)
      uint32_t prev = NONE_ID;
      RecVal rv = qrec;
      for (uint32_t i = 0; i < width - x0; i++) {
        uint32_t v = NONE_VAL;
        if (described) {
          v = plane_value<PLANE>(qrec, (float)(x0 + i) + 0.5f, py);
        } else {
          const uint32_t w = VIS16 ? (uint32_t)pv16[o + i] : pv32[o + i];
          if (w != NONE_ID) {
            if (w != prev) rv = fetch_record<PLANE>(prec, min(w, cap - 1u), ptris), prev = w;
            v = plane_value<PLANE>(rv, (float)(x0 + i) + 0.5f, py);
          }
        }
        dst[i] = (elem)v;
      }
    }
  }
}

// The pixels fixup_kernel re-resolved (its final record is in vis[o]), for the frames in range.  Runs after plane_kernel on the
// same stream and overwrites what the table or an earlier visibility word said for them.
template <uint32_t PLANE, bool VIS16>
__global__ __launch_bounds__(256) void plane_fix_kernel(const void *__restrict__ vis, const PoseConst *__restrict__ poses,
                                                        const TriRec *__restrict__ recs, uint32_t cap,
                                                        const LevelTri *__restrict__ tris, const LevelSlice *__restrict__ slices,
                                                        const uint32_t *__restrict__ fix_count, const uint2 *__restrict__ fix_list,
                                                        uint32_t fix_cap, typename PlaneOf<PLANE>::elem *__restrict__ out,
                                                        uint32_t first, uint32_t count, uint32_t width, uint32_t pitch,
                                                        uint32_t height, uint32_t flags) {
  typedef typename PlaneOf<PLANE>::elem elem;
  const uint32_t total = *fix_count;
  if (total > fix_cap) return;  // fixup_kernel did not run: the render's status says so (device_flags)
  for (uint32_t item = blockIdx.x * 256u + threadIdx.x; item < total; item += gridDim.x * 256u) {
    const uint2 it = fix_list[item];  // (pose, row * pitch + column)
    if (it.x - first >= count) continue;
    const uint32_t y = it.y / pitch, x = it.y - y * pitch;
    if (x >= width || y >= height) continue;
    const size_t o = (size_t)it.x * pitch * height + it.y;
    const uint32_t w = VIS16 ? (uint32_t)reinterpret_cast<const uint16_t *>(vis)[o] : reinterpret_cast<const uint32_t *>(vis)[o];
    uint32_t v = PlaneOf<PLANE>::none;
    if (w != (VIS16 ? 0xFFFFu : NONE)) {
      const LevelTri *ptris = tris;
      if (PLANE == RDOOM_PLANE_LABEL) ptris = tris + slices[poses[it.x].level].first_tri;
      const RecVal rv = fetch_record<PLANE>(recs + (size_t)it.x * cap, min(w, cap - 1u), ptris);
      v = plane_value<PLANE>(rv, (float)x + 0.5f, (float)y + 0.5f);
    }
    const uint32_t yo = (flags & PF_TOP_DOWN) ? height - 1u - y : y;
    out[((size_t)(it.x - first) * height + yo) * width + x] = (elem)v;
  }
}

template <uint32_t PLANE, bool VIS16>
void launch_pair(hipStream_t st, uint32_t grid, const PlaneArgs &a, uint32_t groups_x, uint32_t groups_per_frame, uint32_t tiles_x,
                 uint32_t n_tiles, uint32_t flags) {
  typedef typename PlaneOf<PLANE>::elem elem;
  hipLaunchKernelGGL((plane_kernel<PLANE, VIS16>), dim3(grid), dim3(256), 0, st, a.vis, a.qtab, a.poses, a.recs, a.cap, a.tris,
                     a.slices, (elem *)a.out, a.first, groups_x, groups_per_frame, (uint32_t)a.width, (uint32_t)a.pitch,
                     (uint32_t)a.height, tiles_x, n_tiles, flags);
  hipLaunchKernelGGL((plane_fix_kernel<PLANE, VIS16>), dim3(64), dim3(256), 0, st, a.vis, a.poses, a.recs, a.cap, a.tris, a.slices,
                     a.fix_count, a.fix_list, a.fix_cap, (elem *)a.out, a.first, a.count, (uint32_t)a.width, (uint32_t)a.pitch,
                     (uint32_t)a.height, flags);
}

template <uint32_t PLANE>
void launch_plane_of(hipStream_t st, uint32_t grid, const PlaneArgs &a, uint32_t groups_x, uint32_t groups_per_frame,
                     uint32_t tiles_x, uint32_t n_tiles, uint32_t flags) {
  a.vis16 ? launch_pair<PLANE, true>(st, grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags)
          : launch_pair<PLANE, false>(st, grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags);
}

}  // namespace

size_t plane_element_bytes(uint32_t plane) { return plane == RDOOM_PLANE_LABEL ? 2u : 4u; }

rdoom_status launch_plane(hipStream_t st, const PlaneArgs &a) {
  if (a.count == 0) return RDOOM_OK;
  if (a.cap == 0) return rdoom::fail(RDOOM_BAD_ARG, "internal: a batch without records");
  const uint32_t tiles_x = ((uint32_t)a.width + TILE_W - 1u) / TILE_W, tiles_y = ((uint32_t)a.height + TILE_H - 1u) / TILE_H;
  const uint32_t groups_x = ((uint32_t)a.width + 127u) / 128u;
  const uint32_t row_groups = ((uint32_t)a.height + 32u * PLANE_QROWS - 1u) / (32u * PLANE_QROWS);
  const uint32_t groups_per_frame = groups_x * row_groups;
  const uint64_t grid = (uint64_t)groups_per_frame * a.count;
  if (grid > 0x7FFFFFFFull) return rdoom::fail(RDOOM_BAD_ARG, "planes of %u frames too large for one launch", a.count);
  // u16 rows: pairs of pixels go out as dwords when every row starts on one
  const bool dword = ((uintptr_t)a.out & 3u) == 0u && a.width % 2 == 0;
  const uint32_t flags = (a.use_qtab ? PF_QTAB : 0u) | (a.top_down ? PF_TOP_DOWN : 0u) | (dword ? PF_DWORD : 0u);
  const uint32_t n_tiles = tiles_x * tiles_y;
  switch (a.plane) {
    case RDOOM_PLANE_DEPTH: launch_plane_of<RDOOM_PLANE_DEPTH>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags); break;
    case RDOOM_PLANE_LABEL: launch_plane_of<RDOOM_PLANE_LABEL>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags); break;
    case RDOOM_PLANE_PRIMITIVE: launch_plane_of<RDOOM_PLANE_PRIMITIVE>(st, (uint32_t)grid, a, groups_x, groups_per_frame, tiles_x, n_tiles, flags); break;
    default: return rdoom::fail(RDOOM_BAD_ARG, "unknown plane %u", a.plane);
  }
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // namespace rdoom_dev
