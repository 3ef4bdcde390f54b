// What the world's kernels (world.hip) and the map's (automap.hip) share: the pick of a lane's level, the checked launch, the
// device check of a handle, and the map's side of a world handle.  One definition each, for player_quat.hpp's reason.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../common.hpp"
#include "kernels.hpp"

namespace rdoom_dev {

// `use(slot)` for the level record of a lane on level `lv`: the wave's one slot as a wave-uniform value when every lane of the
// wave is on the same level, so that what `use` loads from that record are scalar loads; the lane's own otherwise
template <class Use>
__device__ __forceinline__ void with_level(uint32_t lv, Use use) {
  const uint32_t u = __builtin_amdgcn_readfirstlane(lv);
  if (__builtin_amdgcn_ballot_w64(lv != u) == 0) use(u);
  else use(lv);
}

}  // namespace rdoom_dev

namespace rdoom {

// kernel(args...) on `stream`, and the error of a launch that could not be queued
template <class Kernel, class... Args>
rdoom_status launch_checked(Kernel kernel, dim3 grid, dim3 block, size_t lds_bytes, void *stream, Args... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t)stream, args...);
  HIP_TRY(hipGetLastError());
  return RDOOM_OK;
}

// noun: "the world" or "the world set"
template <class Handle>
rdoom_status check_device(const Handle *h, const char *noun) {
  if (!h->on_device) return rdoom::fail(RDOOM_BAD_ARG, "%s was created with RDOOM_WORLD_HOST_ONLY: it has no device copy", noun);
  int cur = -1;
  HIP_TRY(hipGetDevice(&cur));
  if (cur != h->device) return rdoom::fail(RDOOM_BAD_ARG, "%s lives on device %d, the current device is %d", noun, h->device, cur);
  return RDOOM_OK;
}

// The device copy of a line table (rdoom_map_line), a structure of arrays private to automap.hip: a world's, or a world set's
// levels one after the other with `levels[slot]` = (first line, number of lines).
struct MapDevice {
  float4 *seg = nullptr;      // a.x, a.z, b.x, b.z
  float4 *heights = nullptr;  // front floor, front ceiling, back floor, back ceiling
  uint4 *ids = nullptr;       // the objects of those four
  uint32_t *flags = nullptr;  // the linedef's flags; bit 16: the front side is present, bit 17: the back side
  uint2 *levels = nullptr;    // a world set's slots (a world: one entry)
  uint32_t n_lines = 0, n_levels = 0;
};
// automap.hip: `lines` with `n_levels` (first, count) ranges on the current device; releases what it allocated
rdoom_status map_upload(const std::vector<rdoom_map_line> &lines, const std::vector<uint2> &levels, MapDevice &out);
void map_free(MapDevice &d);

// what automap.hip needs of a world or world-set handle (world.hip owns the handles)
struct MapSource {
  const MapDevice *map;
  uint32_t game_objects;  // the n_objects its game calls need at least
  bool on_device;
  int device;
};
MapSource map_source(const rdoom_world *w);
MapSource map_source(const rdoom_worldset *s);

}  // namespace rdoom
