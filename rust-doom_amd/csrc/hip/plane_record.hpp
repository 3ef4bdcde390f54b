// What the plane kernels (planes.hip) and the observation kernels (observe.hip) take from a pixel's winning record: one place for
// the loads and for the depth formula, so that both passes give the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hpp"

#pragma clang fp contract(off)

namespace rdoom_dev {

constexpr uint32_t DEPTH_FAR = 0x7F800000u;  // +inf: sky (sky.frag has no v_dist) and pixels nothing was drawn to

// what a plane keeps of a record: depth the 1/w plane and the kind, the others their finished value
struct RecVal {
  float w0, w1, w2;
  uint32_t v;
};

// The tables of the pose's level that a record's primitive id indexes.  tris: the level's first triangle (the label).  things: the
// level's words of DeviceLevelView::tri_thing, ntri >= 1 its triangles (the thing plane; never null there: a handle without a table
// takes no kernel).  Depth and primitive id read neither.
struct LevelTables {
  const LevelTri *tris;
  const uint32_t *things;
  uint32_t ntri;
};

// With a wave-uniform pose these are scalar loads.
template <uint32_t PLANE>
__device__ __forceinline__ LevelTables level_tables(const LevelTri *__restrict__ tris, const uint32_t *__restrict__ tri_thing,
                                                    const LevelSlice *__restrict__ slices, const PoseConst *__restrict__ poses, uint32_t pose) {
  LevelTables t{tris, tri_thing, 0u};
  if (PLANE == RDOOM_PLANE_LABEL) t.tris = tris + slices[poses[pose].level].first_tri;
  if (PLANE == PLANE_THING) {
    const LevelSlice &sl = slices[poses[pose].level];
    t.things = tri_thing + sl.first_tri, t.ntri = sl.ntri;
  }
  return t;
}

// rec < cap (the callers clamp).  With a wave-uniform `rec` every load here is a scalar load.  The thing plane's second load is made
// for a decor record only; the primitive id of a record is below ntri by construction (set-up writes tri - first_tri of a triangle
// of the pose's slice) and is clamped all the same: one word per triangle of the slice is all the table holds.  RDOOM_NO_THING is
// 0xFFFFFFFF: -1 as it stands.
template <uint32_t PLANE>
__device__ __forceinline__ RecVal fetch_record(const TriRec *__restrict__ prec, uint32_t rec, const LevelTables &t) {
  RecVal r{0.0f, 0.0f, 0.0f, 0u};
  const uint32_t rf = prec[rec].r.flags;
  const uint32_t kind = (rf >> 27) & 3u, prim = rf & 0xFFFFFFu;
  if (PLANE == RDOOM_PLANE_DEPTH) {
    const uint4 w = *reinterpret_cast<const uint4 *>(&prec[rec].s);  // (wp[0], wp[1], wp[2], up[0])
    r.w0 = __uint_as_float(w.x), r.w1 = __uint_as_float(w.y), r.w2 = __uint_as_float(w.z);
    r.v = kind;
  } else if (PLANE == RDOOM_PLANE_LABEL) {
    r.v = kind | ((t.tris[prim].packed >> 20) << 4);
  } else if (PLANE == PLANE_THING) {
    r.v = kind != RDOOM_KIND_DECOR ? NONE : t.things[min(prim, t.ntri - 1u)];
  } else {
    r.v = prim;
  }
  return r;
}

template <uint32_t PLANE>
__device__ __forceinline__ uint32_t plane_value(const RecVal &r, float px, float py) {
  if (PLANE != RDOOM_PLANE_DEPTH) return r.v;
  const float d = 1.0f / fmaf(r.w0, px, fmaf(r.w1, py, r.w2));  // F1: IEEE division, as texel_coords without RCP_EXACT
  return r.v == RDOOM_KIND_SKY ? DEPTH_FAR : __float_as_uint(d);
}

}  // namespace rdoom_dev
