// game::world::WorldBuilder (game/src/world.rs:211-409): the collision volume the reference's player sweeps its head and
// feet against, built by the same level walk that drives the renderer's Builder.  Host only: the device copy and the sweep /
// player-step kernels live in csrc/hip/world.hip.
#pragma once
#include <cstdint>
#include <vector>

#include "game_level.hpp"

namespace rdoom::game {

// Node { partition: Line2f, positive: i32, negative: i32 } (world.rs:139-143) with the children as Child::pack writes them
// (world.rs:152-163): a node index > 0, or minus a chunk index.  A child that was never linked stays 0 = Leaf(0).
struct WorldNode {
  float origin[2], displace[2], length;
  int32_t positive, negative;
};
struct WorldChunk {  // world.rs:124-128
  uint32_t tri_start, tri_end;
};
struct WorldTriangle {  // world.rs:135-141: indices into verts; `normal` too
  uint32_t v1, v2, v3, normal;
};
struct WorldDynamic {  // one DynamicChunk per moving object with triangles (world.rs:212-237), by ascending ObjectId
  uint32_t object_id, tri_start, tri_end;
};

struct World {
  std::vector<WorldNode> nodes;
  std::vector<WorldChunk> chunks;
  std::vector<WorldTriangle> triangles;  // the static world's (object 0), then each dynamic chunk's, as build() orders them
  std::vector<float> verts;              // xyz triples: polygon vertices, each polygon followed by its normal
  std::vector<WorldDynamic> dynamics;
  uint32_t n_static_triangles = 0;
  uint32_t n_objects = 1;    // 1 + the largest ObjectId of a dynamic chunk
  uint32_t node_depth = 0;   // nodes on the longest root-to-node path
  // the level's triggers and their move effects (LevelAnalysis of the same walk), as the C ABI lays them out
  std::vector<rdoom_trigger> triggers;
  std::vector<rdoom_move_effect> effects;
  uint32_t game_objects = 1;  // max(1, LevelAnalysis::num_objects)
  // the level's line table for the top-down map (include/rdoom.h rdoom_map_line): one record per linedef with both vertices
  std::vector<rdoom_map_line> map_lines;
  // the level's sector table (include/rdoom.h rdoom_map_sectors): a record per SECTORS entry; per chunk (at least one entry) the
  // sector of the sub-sector behind it and its range of solid edges
  std::vector<rdoom_map_sector> map_sectors;
  std::vector<uint32_t> leaf_sector;
  std::vector<rdoom_map_leaf_edges> leaf_edges;
  std::vector<rdoom_map_edge> map_edges;
  // the level's thing table (include/rdoom.h "things"): a record per THINGS entry the walk sends down its decor branch, in lump order
  std::vector<rdoom_thing> things;
  // which of them are solid (include/rdoom.h "solid things"): max(1, ceil(things / 32)) words, bit i % 32 of word i / 32 for thing i
  std::vector<uint32_t> thing_obstacles;
  // the level's spawn table (include/rdoom.h "spawn"): an entry per floor triangle with an area, in the order of `triangles`
  std::vector<rdoom_spawn_entry> spawn;
  float start_pos[3] = {0, 0, 0};  // the player's start, as the renderer's Builder takes it (rdoom_built_start)
  float start_yaw = 0.0f;
};

// Several levels' worlds at once (a world set): each level's World as build_world makes it, and the levels concatenated with
// every index rebased, for the device.  Slot s holds archive level archive_index[s]; its destination is the slot holding
// archive_index[s] + 1, or NO_DESTINATION.
constexpr uint32_t NO_DESTINATION = 0xFFFFFFFFu;
struct WorldSetLevel {
  uint32_t archive_index, destination;
  uint32_t node_base, chunk_base, triangle_base, vert_base, dynamic_base, trigger_base, effect_base, map_base;  // in the concatenation
};
struct WorldSet {
  std::vector<World> levels;
  std::vector<WorldSetLevel> table;
  // the concatenation: node children, chunk and dynamic triangle ranges, triangle vertex indices and trigger effect ranges
  // rebased (the map lines are concatenated as they are: their object ids are each level's own).  A child packed as 0 (Leaf(0), never linked or not) becomes minus its own level's chunk base, so it still reads as
  // that level's leaf 0.
  // The sector tables are not concatenated here: they stay with `levels`, and the device copy lays them out one after the other.
  World all;
  uint32_t game_objects = 1;  // the largest of the levels' game_objects
  uint32_t node_depth = 0;    // the deepest level's
};

// build_world for each of n archive levels, then the concatenation.  Throws WadError(RDOOM_BAD_ARG) on an empty list, an
// index out of range or a duplicate index, and what build_world throws.
WorldSet build_world_set(const LoadedWad &w, const uint32_t *level_indices, size_t n);

// WorldBuilder::new + LevelWalker::walk + WorldBuilder::build.  Throws WadError(RDOOM_BAD_LEVEL) on a level without a BSP.
World build_world(const LoadedWad &w, size_t level_index);
// the spawn table of the collision arrays (include/rdoom.h "spawn"): a pure function of triangles and verts
std::vector<rdoom_spawn_entry> build_spawn_table(const World &w);
// the archive behind a C handle (csrc/host/wad_api.cpp)
const LoadedWad *loaded_wad(const rdoom_wad *wad);

}  // namespace rdoom::game
