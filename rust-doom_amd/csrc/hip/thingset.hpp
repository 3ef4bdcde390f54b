// The device thing set (include/rdoom.h "things"): the handle things.hip creates and destroys, and that the sensing launches
// (things.hip), the thing maps (thingmap.hip) and the stamp into the area planes (stamp.hip) read.  One definition, for
// player_quat.hpp's reason.
#pragma once
#include <hip/hip_runtime.h>

#include "../common.hpp"

struct rdoom_thingset {
  rdoom::DeviceArray<rdoom_thing> d_things;  // the levels' records, one level after the other
  rdoom::DeviceArray<uint2> d_levels;        // a slot's (first record, number of records)
  uint2 level0 = {};                         // slot 0's, on the host: a single world's launch passes it by value
  uint32_t n_levels = 0, words = 1, max_object_id = 0;
  int device = -1;
};
