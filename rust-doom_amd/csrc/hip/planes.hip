// Per-pixel planes of a batch's last render: depth (the winning fragment's v_dist, binary32), label (kind | object id << 4, u16) and
// primitive id (u32) for rdoom_batch_resolve_plane, and the thing plane (the thing of the winning decor triangle, -1 elsewhere, u32;
// PLANE_THING, internal) for rdoom_batch_resolve_thing_plane.  A second resolve pass over what the render leaves on the device anyway;
// the render kernels are not involved and nobody who does not ask pays for it.
//
// The winning record of a pixel is found by render_walk.hpp's walk: the quadrant table (a described quadrant's record by scalar
// loads, no visibility word read), the visibility words, then the fixup list.  What is this unit's own: along a lane's run of 16
// pixels neighbours mostly share a record, so a record is gathered only where the word differs from the previous pixel's.
// What a record gives is plane_record.hpp's: RasterRec::flags (primitive id, kind), ShadeRec::wp (the 1/w plane: depth = 1 / plane
// at the pixel centre, F1 of DESIGN section 3 -- the bits texel_coords calls `dist`); the label's object id is LevelTri::packed of
// the primitive, the thing of a decor primitive its word in DeviceLevelView::tri_thing.
//
// Bandwidth-bound: 2-4 B/px written, 2 or 4 B/px of visibility words read outside described quadrants, plus the record gathers
// (one cache line per distinct record of a run).  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "plane_record.hpp"  // RecVal, LevelTables, fetch_record, plane_value, DEPTH_FAR: shared with observe.hip
#include "render_walk.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {
namespace {

template <uint32_t PLANE>
struct PlaneOf {  // RDOOM_PLANE_PRIMITIVE, PLANE_THING
  typedef uint32_t elem;
  static constexpr uint32_t none = NONE;
};
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

template <uint32_t PLANE, bool VIS16>
__global__ __launch_bounds__(256) void plane_kernel(const void *__restrict__ vis, const uint32_t *__restrict__ qtab,
                                                    const PoseConst *__restrict__ poses, const TriRec *__restrict__ recs,
                                                    uint32_t cap, const LevelTri *__restrict__ tris,
                                                    const uint32_t *__restrict__ tri_thing, const LevelSlice *__restrict__ slices,
                                                    typename PlaneOf<PLANE>::elem *__restrict__ out, uint32_t first,
                                                    uint32_t groups_x, uint32_t groups_per_frame, uint32_t width, uint32_t pitch,
                                                    uint32_t height, uint32_t tiles_x, uint32_t n_tiles, uint32_t flags) {
  typedef typename PlaneOf<PLANE>::elem elem;
  constexpr uint32_t NONE_VAL = PlaneOf<PLANE>::none;
  constexpr uint32_t NONE_ID = VisWord<VIS16>::none;
  const WalkLane l = walk_lane(first, groups_x, groups_per_frame);
  const uint32_t qx = l.qx, x0 = l.x0;
  if (qx * 32u >= width) return;
  const void *pvis = vis_of_pose<VIS16>(vis, l.pose, (size_t)pitch * height);
  const TriRec *prec = recs + (size_t)l.pose * cap;
  const LevelTables lt = level_tables<PLANE>(tris, tri_thing, slices, poses, l.pose);  // (scalar loads: one pose per workgroup)
  for (uint32_t k = 0; k < WALK_QROWS; k++) {
    const uint32_t qy = l.gy * WALK_QROWS + k;
    if (qy * 32u >= height) break;
    const uint32_t ent = quadrant_entry(qtab, flags, l.pose, n_tiles, tiles_x, qx, qy);
    const bool described = ent != NONE;
    RecVal qrec{0.0f, 0.0f, 0.0f, 0u};
    if (described) {  // wave-uniform: the record's words by scalar loads
      const uint32_t rec = min((uint32_t)__builtin_amdgcn_readfirstlane((int)(ent & ENTRY_REC_MASK)), cap - 1u);
      qrec = fetch_record<PLANE>(prec, rec, lt);
    }
    const uint32_t y = qy * 32u + (l.lane >> 1);
    if (y >= height || x0 >= width) continue;
    const uint32_t yo = (flags & WF_TOP_DOWN) ? height - 1u - y : y;
    const size_t o = (size_t)y * pitch + x0;
    const float py = (float)y + 0.5f;
    elem *dst = out + ((size_t)l.f * height + yo) * width + x0;
    if (x0 + 16u <= width) {
      uint32_t c[16];
      if (described) {
#pragma unroll
        for (int i = 0; i < 16; i++) c[i] = plane_value<PLANE>(qrec, (float)(x0 + i) + 0.5f, py);
      } else {
        uint32_t w[16];
        vis_run<VIS16>(pvis, o, w);
        uint32_t prev = NONE_ID;
        RecVal rv{0.0f, 0.0f, 0.0f, 0u};
#pragma unroll
        for (int i = 0; i < 16; i++) {
          if (w[i] != NONE_ID && w[i] != prev) {  // a new record in this run
            rv = fetch_record<PLANE>(prec, min(w[i], cap - 1u), lt);
            prev = w[i];
          }
          c[i] = w[i] == NONE_ID ? NONE_VAL : plane_value<PLANE>(rv, (float)(x0 + i) + 0.5f, py);
        }
      }
      store_run<PLANE>(dst, c, (flags & WF_DWORD) != 0u);
    } else {  // the row's last pixels (a width that is not a multiple of 16)
      uint32_t prev = NONE_ID;
      RecVal rv = qrec;
      for (uint32_t i = 0; i < width - x0; i++) {
        uint32_t v = NONE_VAL;
        if (described) {
          v = plane_value<PLANE>(qrec, (float)(x0 + i) + 0.5f, py);
        } else {
          const uint32_t w = vis_word<VIS16>(pvis, o + i);
          if (w != NONE_ID) {
            if (w != prev) rv = fetch_record<PLANE>(prec, min(w, cap - 1u), lt), prev = w;
            v = plane_value<PLANE>(rv, (float)(x0 + i) + 0.5f, py);
          }
        }
        dst[i] = (elem)v;
      }
    }
  }
}

// Runs after plane_kernel on the same stream and overwrites what the table or an earlier visibility word said for the fixup
// list's pixels.
template <uint32_t PLANE, bool VIS16>
__global__ __launch_bounds__(256) void plane_fix_kernel(const void *__restrict__ vis, const PoseConst *__restrict__ poses,
                                                        const TriRec *__restrict__ recs, uint32_t cap,
                                                        const LevelTri *__restrict__ tris, const uint32_t *__restrict__ tri_thing,
                                                        const LevelSlice *__restrict__ slices,
                                                        const uint32_t *__restrict__ fix_count, const uint2 *__restrict__ fix_list,
                                                        uint32_t fix_cap, typename PlaneOf<PLANE>::elem *__restrict__ out,
                                                        uint32_t first, uint32_t count, uint32_t width, uint32_t pitch,
                                                        uint32_t height, uint32_t flags) {
  typedef typename PlaneOf<PLANE>::elem elem;
  walk_fix_list<VIS16>(vis, fix_count, fix_list, fix_cap, first, count, width, pitch, height,
                       [&](uint32_t pose, uint32_t x, uint32_t y, uint32_t w, bool drawn) {
                         uint32_t v = PlaneOf<PLANE>::none;
                         if (drawn) {
                           const LevelTables lt = level_tables<PLANE>(tris, tri_thing, slices, poses, pose);
                           const RecVal rv = fetch_record<PLANE>(recs + (size_t)pose * cap, min(w, cap - 1u), lt);
                           v = plane_value<PLANE>(rv, (float)x + 0.5f, (float)y + 0.5f);
                         }
                         const uint32_t yo = (flags & WF_TOP_DOWN) ? height - 1u - y : y;
                         out[((size_t)(pose - first) * height + yo) * width + x] = (elem)v;
                       });
}

template <uint32_t PLANE, bool VIS16>
void launch_pair(hipStream_t st, const PlaneArgs &a, const WalkLaunch &g) {
  typedef typename PlaneOf<PLANE>::elem elem;
  hipLaunchKernelGGL((plane_kernel<PLANE, VIS16>), dim3(g.grid), dim3(256), 0, st, a.vis, a.qtab, a.poses, a.recs, a.cap, a.tris,
                     a.tri_thing, a.slices, (elem *)a.out, a.first, g.groups_x, g.groups_per_frame, a.width, a.pitch, a.height, g.tiles_x,
                     g.n_tiles, g.flags);
  hipLaunchKernelGGL((plane_fix_kernel<PLANE, VIS16>), dim3(64), dim3(256), 0, st, a.vis, a.poses, a.recs, a.cap, a.tris, a.tri_thing,
                     a.slices, a.fix_count, a.fix_list, a.fix_cap, (elem *)a.out, a.first, a.count, a.width, a.pitch, a.height, g.flags);
}

template <uint32_t PLANE>
void launch_plane_of(hipStream_t st, const PlaneArgs &a, const WalkLaunch &g) {
  a.vis16 ? launch_pair<PLANE, true>(st, a, g) : launch_pair<PLANE, false>(st, a, g);
}

}  // namespace

size_t plane_element_bytes(uint32_t plane) { return plane == RDOOM_PLANE_LABEL ? 2u : 4u; }

rdoom_status launch_plane(hipStream_t st, const PlaneArgs &a) {
  if (a.count == 0) return RDOOM_OK;
  if (a.plane == PLANE_THING && !a.tri_thing) {  // a handle without a table: no pixel names a thing
    HIP_TRY(hipMemsetAsync(a.out, 0xFF, (size_t)a.count * a.height * a.width * sizeof(int32_t), st));
    return RDOOM_OK;
  }
  if (a.cap == 0) return rdoom::fail(RDOOM_BAD_ARG, "internal: a batch without records");
  // u16 rows: pairs of pixels go out as dwords when every row starts on one
  const bool dword = ((uintptr_t)a.out & 3u) == 0u && a.width % 2 == 0;
  WalkLaunch g;
  if (rdoom_status rs = walk_launch(a, a.plane == PLANE_THING ? "thing planes" : "planes", dword, &g)) return rs;
  switch (a.plane) {
    case RDOOM_PLANE_DEPTH: launch_plane_of<RDOOM_PLANE_DEPTH>(st, a, g); break;
    case RDOOM_PLANE_LABEL: launch_plane_of<RDOOM_PLANE_LABEL>(st, a, g); break;
    case RDOOM_PLANE_PRIMITIVE: launch_plane_of<RDOOM_PLANE_PRIMITIVE>(st, a, g); break;
    case PLANE_THING: launch_plane_of<PLANE_THING>(st, a, g); break;
    default: return rdoom::fail(RDOOM_BAD_ARG, "unknown plane %u", a.plane);
  }
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

}  // namespace rdoom_dev
