// Sanitizer driver of the handles' FAILURE paths (csrc/hip/device_memory.hpp: every handle owns its device memory, events and
// streams) -- test infrastructure.  Built by tests/test_host_sanitizers.py: every HIP unit with -Xarch_host
// -fsanitize=address,undefined, the host sources and this file with -fsanitize=address,undefined, linked into one program.  The
// test runs it with no device visible, so every create fails at its first call of the runtime, after the host side of the create
// has run; what a create built by then must be released (LeakSanitizer at exit) and *out must stay null.
//   handle_errors <iwad> <metadata>
// A program that does find a device prints "SKIP" and creates nothing: a sanitized binary never touches a GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rdoom.h"

static int failures = 0;
#define CHECK(cond)                                                                              \
  do {                                                                                           \
    if (!(cond)) {                                                                               \
      std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, rdoom_last_error()); \
      failures++;                                                                                \
    }                                                                                            \
  } while (0)

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  int32_t devices = 0;
  if (rdoom_device_count(&devices) == RDOOM_OK && devices > 0) {
    std::printf("SKIP: %d device(s) visible\n", devices);
    return 0;
  }
  rdoom_wad *wad = nullptr;
  CHECK(rdoom_wad_open(argv[1], argv[2], &wad) == RDOOM_OK);
  if (!wad) return 1;

  // ---- the renderer's level and level set, from real descriptors ----
  rdoom_built *built[3] = {};
  rdoom_level_desc descs[3];
  const rdoom_level_desc *desc_ptrs[3];
  for (uint32_t k = 0; k < 3; k++) {
    CHECK(rdoom_wad_build_level(wad, k, 0, &built[k]) == RDOOM_OK);
    if (!built[k]) return 1;
    CHECK(rdoom_built_desc(built[k], &descs[k]) == RDOOM_OK);
    desc_ptrs[k] = &descs[k];
  }
  rdoom_level *level = reinterpret_cast<rdoom_level *>(1);
  CHECK(rdoom_level_create(&descs[1], &level) == RDOOM_HIP_ERROR && level == nullptr);
  level = reinterpret_cast<rdoom_level *>(1);
  CHECK(rdoom_levelset_create(desc_ptrs, 3, &level) == RDOOM_HIP_ERROR && level == nullptr);
  rdoom_batch *batch = nullptr;
  CHECK(rdoom_batch_create(nullptr, 128, 80, 4, &batch) == RDOOM_BAD_ARG && batch == nullptr);

  // ---- worlds: no device copy without a device; host-only handles are whole, and refuse device calls ----
  const uint32_t indices[2] = {0, 1};
  rdoom_world *world = reinterpret_cast<rdoom_world *>(1);
  CHECK(rdoom_world_create(wad, 1, 0, &world) == RDOOM_HIP_ERROR && world == nullptr);
  rdoom_worldset *set = reinterpret_cast<rdoom_worldset *>(1);
  CHECK(rdoom_worldset_create(wad, indices, 2, 0, &set) == RDOOM_HIP_ERROR && set == nullptr);
  CHECK(rdoom_world_create(wad, 1, RDOOM_WORLD_HOST_ONLY, &world) == RDOOM_OK && world != nullptr);
  CHECK(rdoom_worldset_create(wad, indices, 2, RDOOM_WORLD_HOST_ONLY, &set) == RDOOM_OK && set != nullptr);
  if (!world || !set) return 1;
  const float dir[3] = {0.0f, 0.0f, -1.0f};  // (checked for null only: nothing is queued for n = 0 players)
  CHECK(rdoom_world_cast_rays(world, nullptr, 0, dir, 1, 100.0f, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == RDOOM_BAD_ARG &&
        std::strstr(rdoom_last_error(), "RDOOM_WORLD_HOST_ONLY"));
  CHECK(rdoom_worldset_cast_rays(set, nullptr, nullptr, 0, dir, 1, 100.0f, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) ==
            RDOOM_BAD_ARG &&
        std::strstr(rdoom_last_error(), "RDOOM_WORLD_HOST_ONLY"));

  // ---- the light set and the thing set, from the tables the host built ----
  const rdoom_light_info *infos[3] = {};
  uint32_t info_counts[3] = {};
  for (uint32_t k = 0; k < 3; k++) CHECK(rdoom_built_light_infos(built[k], &infos[k], &info_counts[k]) == RDOOM_OK);
  rdoom_lightset *lights = reinterpret_cast<rdoom_lightset *>(1);
  CHECK(rdoom_lightset_create(infos, info_counts, 3, &lights) == RDOOM_HIP_ERROR && lights == nullptr);
  rdoom_map_things map_things{};
  CHECK(rdoom_world_map_things(world, &map_things) == RDOOM_OK);
  rdoom_thingset *things = reinterpret_cast<rdoom_thingset *>(1);
  CHECK(rdoom_thingset_create(&map_things.things, &map_things.n_things, 1, &things) == RDOOM_HIP_ERROR && things == nullptr);

  rdoom_world_destroy(world);
  rdoom_worldset_destroy(set);
  rdoom_level_destroy(nullptr);
  rdoom_batch_destroy(nullptr);
  rdoom_world_destroy(nullptr);
  rdoom_worldset_destroy(nullptr);
  rdoom_lightset_destroy(nullptr);
  rdoom_thingset_destroy(nullptr);
  for (rdoom_built *b : built) rdoom_built_destroy(b);
  rdoom_wad_close(wad);
  std::printf("%s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
