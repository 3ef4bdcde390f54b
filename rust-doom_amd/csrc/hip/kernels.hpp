// Launchers of the renderer's kernels, one translation unit per kernel (setup.hip, bin.hip, raster.hip,
// fragment.hip); renderer.hip (the C ABI) strings them together on the caller's stream.
#pragma once
#include "device_memory.hpp"  // HIP_TRY
#include "records.hpp"

namespace rdoom_dev {

constexpr uint32_t MAX_TILES = 8192;     // tiles per frame the binning kernel keeps counters for
// A tile whose list is longer than one batch of the rasteriser (one entry per lane) gets a list per 32 x 32 quadrant (bin.hip):
// tile header word y carries TILE_SPLIT, word x points at (first entry, count) x 4 in the pose's entry array
// (LONG_LIST 32 / 64 / 128: 64 gives the fastest rasteriser at 1080p, at 320 x 200 and on the large level, profiles/r04_ab.txt, item 7)
constexpr uint32_t LONG_LIST = 64, TILE_SPLIT = 0x80000000u;
constexpr int RASTER_CENSUS = 6;  // counters launch_raster hands back under the hook raster_stats

// Kernel 1: vertex stage, triangle setup, near-to-far record order (setup.hip)
rdoom_status launch_setup(hipStream_t st, uint32_t n_poses, const DeviceLevelView &lv, const PoseConst *poses,
                          const ObjectConst *objects, uint32_t n_objects, int width, int height, uint32_t kinds_mask,
                          TriRec *recs, uint32_t *visible, uint32_t *counts, uint32_t *ghist, uint32_t cap,
                          uint32_t *mismatch_flag,  // set when the set-up kernel rejects a triangle the cull kernel kept
                          // rows of thing bits, hidden_stride words per pose, or null (rdoom_batch_set_hidden_things): the cull
                          // kernel drops the decor triangles of the things set in a pose's row (lv.tri_thing names them)
                          const uint32_t *hidden, uint32_t hidden_stride);
size_t setup_histogram_bytes(uint32_t max_poses);  // scratch of the counting sort (per pose: one counter per depth bucket)
// Kernel 1b: per-tile triangle lists (bin.hip).  *launched = false: the frame has too many tiles for the kernel's LDS counters --
// nothing was launched and the caller must flag every pose as "bins incomplete".  A launch that FAILS is an error.
rdoom_status launch_bin(hipStream_t st, uint32_t n_poses, const TriRec *recs, const uint32_t *counts,
                        uint32_t cap, int tiles_x, int tiles_y, uint2 *tile_hdr, uint32_t *entries, uint32_t entry_cap,
                        uint2 *hits, uint32_t *overflow,
                        bool want_split, bool *launched, bool *used_split);  // lists of more than LONG_LIST entries per quadrant, if the counters fit (bin.hip)
// Kernel 2: tiled rasteriser -> visibility words (raster.hip)
rdoom_status launch_raster(hipStream_t st, uint32_t n_poses, const DeviceLevelView &lv, const TriRec *recs,
                           const uint32_t *counts, uint32_t cap, int width, int height, int tiles_x,
                           int tiles_y, const uint2 *tile_hdr, const uint32_t *entries, uint32_t entry_cap,
                           const uint32_t *overflow, uint32_t *vis, bool vis16, uint32_t *prim_out,
                           uint32_t *qtab,  // qtab (optional): per (pose, tile, quadrant) the record all its pixels show, or NONE
                           uint2 *qpair,    // beside the table: settle_kernel's pair descriptors, as many (internal to the two kernels)
                           bool skip_described_vis,  // no visibility words for quadrants the table describes (FragmentPlan)
                           bool split_lists,  // the binning kernel stored long lists per quadrant (launch_bin's answer for this render)
                           bool bins_launched,  // the binning kernel ran (its overflow flags are this render's): settle_kernel may read the lists
                           // under the hook raster_stats (else zeros): fast masked bodies, their winners, replayed lanes, general masked
                           // bodies; pairs settle_kernel proved and the tile's wave expanded, pairs the wave found itself
                           uint64_t (&census)[RASTER_CENSUS]);
// How the fragment kernel will walk a frame of this size, decided ONCE per render from the debug hooks (rasteriser and
// fragment kernel must agree on who reads the quadrant table): quads per lane, log2(units per block row), blocks per
// workgroup wave, the test hook leak_mod, and qtab_mode (0: table unused; 1 / 2: a wave block lies in one / two quadrants).
struct FragmentPlan {
  int nq;
  uint32_t bwl, chunk, leak_mod, qtab_mode;
  // the rasteriser may leave out the visibility words of quadrants the table describes: every reader consults the table first
  bool skip_described_vis;
  // fragment_quadrant_kernel shades the described quadrants whose record qualifies before fragment_kernel runs
  bool quadrant_path;
  // test hooks carried in the kernel's qtab_mode argument: no half lanes (a mixed run lists both quads); count half lanes and listed quads
  bool no_half_runs, count;
};
FragmentPlan plan_fragment(int width, int pitch, int height, bool have_qtab);
// Kernels 3 + 4: fragment kernel -> palette indices, then the alpha-leak fixup (fragment.hip)
rdoom_status launch_fragment(hipStream_t st, uint32_t n_poses, const DeviceLevelView &lv, const TriRec *recs,
                             const uint32_t *counts, uint32_t cap, const PoseConst *poses,
                             int width, int pitch,  // the frame's width; pixels between rows of visibility words / framebuffer bytes
                             int height, int tiles_x, int tiles_y, const uint2 *tile_hdr,
                             const uint32_t *entries, uint32_t entry_cap, const uint32_t *overflow, uint32_t *vis,
                             bool vis16, uint32_t *prim_out, const float *ndc_tab, uint8_t *fb, uint32_t *fix_count,
                             uint2 *fix_list, uint32_t fix_cap, uint32_t *qtab, void *d_frag_const,
                             bool *frag_const_ready, const FragmentPlan &plan);  // d_frag_const: fragment_const_bytes() of device memory owned by the batch
size_t fragment_const_bytes();
size_t fragment_counts_offset();  // in d_frag_const: three words the fragment kernel counts into under the hook frag_count (FragmentPlan::count)

// What the read-back passes below take from a batch: the last render as it lies on the device and the frames asked for.
// render_walk.hpp has the walk over it that they share.
struct FrameSource {
  const uint8_t *fb;
  const void *vis;
  bool vis16;
  const uint32_t *qtab;
  bool use_qtab;  // the render's FragmentPlan::skip_described_vis: a described quadrant's visibility words are stale
  const PoseConst *poses;
  const TriRec *recs;  // cap records per pose
  uint32_t cap;
  const uint32_t *fix_count;
  const uint2 *fix_list;
  uint32_t fix_cap;
  uint32_t width, pitch, height;
  uint32_t first, count;  // frames [first, first + count) of the last render
  bool top_down;
};

// Kernels 5 + 6: those frames -> RGB8 / RGBA8, then the pixels of the fixup list (resolve.hip)
struct ResolveArgs : FrameSource {
  const uint32_t *palettes;  // per level of the set: 256 words R | G << 8 | B << 16 | 0xFF << 24
  uint32_t bpp;  // 3 or 4
  uint8_t *out;  // count x height x width x bpp bytes
};
rdoom_status launch_resolve(hipStream_t st, const ResolveArgs &args);

// Kernels 7 + 8: one per-pixel plane (RDOOM_PLANE_*, or PLANE_THING) of those frames, from the quadrant table, the visibility words
// and the pose's records, then the pixels of the fixup list (planes.hip).  Kernels 28 and 29 were the thing plane's own pair; it is
// a fourth instantiation of this one now.
constexpr uint32_t PLANE_THING = 4u;  // internal (rdoom_batch_resolve_thing_plane; include/rdoom_frame_things.h has the contract): per
                                      // pixel the thing of the winning decor triangle, -1 elsewhere
struct PlaneArgs : FrameSource {
  const LevelTri *tris;  // the label's object ids: LevelTri::packed of slices[pose.level].first_tri + primitive id
  const LevelSlice *slices;
  const uint32_t *tri_thing;  // PLANE_THING only: DeviceLevelView::tri_thing, or null: every element is -1
  uint32_t plane;  // RDOOM_PLANE_DEPTH / LABEL / PRIMITIVE, PLANE_THING
  void *out;  // count x height x width elements of plane_element_bytes(plane), aligned to the element
};
size_t plane_element_bytes(uint32_t plane);
rdoom_status launch_plane(hipStream_t st, const PlaneArgs &args);

// Kernels 10 + 11: reduced-size observations (RDOOM_OBS_*) of those frames -- the mean colour, its grey value or the smallest depth
// of every fx x fy cell -- from what kernels 5 to 8 read, then the cells that hold a pixel of the fixup list (observe.hip).
// `recs` is read by RDOOM_OBS_DEPTH_MIN only.
struct ObserveArgs : FrameSource {
  const uint32_t *palettes;  // as ResolveArgs; not read by RDOOM_OBS_DEPTH_MIN
  uint32_t format;  // RDOOM_OBS_*
  uint32_t fx, fy;  // 1, 2, 4 or 8 each
  void *out;  // count frames of (height / fy) x (width / fx) cells, aligned to the element
};
size_t observation_cell_bytes(uint32_t format);  // bytes per cell: 3 (both RGB8 layouts), 1 (grey), 4 (depth)
rdoom_status launch_observe(hipStream_t st, const ObserveArgs &args);

// Kernel 0 of rdoom_batch_render_players, and all of rdoom_poses_from_players_device: players' states -> cameras (frames.hip).
// One lane per (player, object); every output is optional.
struct PlayerFrameArgs {
  const rdoom_player_state *states;
  uint32_t n;                 // players
  uint32_t lanes;             // lanes per player: the offsets' row length (n_objects), or 1 without offsets
  const float *offsets;       // n x lanes x xyz, or null (lanes == 1)
  float proj[16], zk, time;   // player_projection's, and u_time
  const uint32_t *levels;     // level of each player, or null (level 0)
  uint32_t n_slices;          // levels of the batch's set: a level >= n_slices is rendered as 0 and recorded in *error_word
  uint32_t *error_word;
  const uint8_t *lights;      // 256 bytes per level slot at lights_stride (0: one shared table)
  uint32_t lights_stride;
  PoseConst *pose_consts;     // n records, or null (then nothing below is written either)
  ObjectConst *object_consts; // n x n_render_objects records, or null
  uint32_t n_render_objects;
  rdoom_pose *poses_out;      // n poses, or null
  float *modelviews_out;      // n x lanes x 16 floats, or null
  const float *times;         // per-player u_time (the clocked entry points), or null: `time` for every player.  With `times`,
                              // `lights` is null and PoseConst::lights is left to launch_light_tables
};
rdoom_status launch_player_frames(hipStream_t st, const PlayerFrameArgs &args);
// the camera's projection for a width x height frame (rdoom_pose_from_player's, bit for bit) and render_impl's depth constant zk
rdoom_status player_projection(uint32_t width, uint32_t height, float proj[16], float *zk);


// Kernel 9: 256-byte light tables of n players from their clocks (lights.hip; include/rdoom.h "device light set" has the contract).
// Row p -- `stride` bytes after row p - 1, 4-byte aligned -- is Lights::fill_buffer_at(times[p]) of level levels[p] of the set.
struct LightSetView {
  const rdoom_light_info *infos;  // device: the levels' info lists, one after the other
  const uint2 *ranges;            // device: per level (first info, count <= 255)
  uint32_t n_levels;
  int device;
};
const LightSetView *lightset_view(const rdoom_lightset *set);
struct LightTableArgs {
  LightSetView set;
  const uint32_t *levels;  // or null: slot 0
  const float *times;
  uint32_t n;
  uint8_t *out;
  uint32_t stride;         // bytes between rows: 256 (rdoom_lightset_tables) or sizeof(PoseConst) (the clocked render)
  uint32_t fallback;       // the slot a player outside the set takes: >= n_levels gives a row of zeros, 0 what the render shows
};
rdoom_status launch_light_tables(hipStream_t st, const LightTableArgs &args);

// Kernels 12, 16 and 20: the three distance floods (flood.hip; include/rdoom.h "flood", "goal distance" and "octile distance" have
// the contracts).  One workgroup per grid.  What all take:
struct FloodPlanes {
  const float *floor, *ceiling;  // n x height x width each, as rdoom_world_draw_sector_maps or rdoom_world_draw_area_planes stores them
  const int32_t *seeds;          // n x (column, row), or null: (width / 2, height / 2)
  uint32_t *count_out;           // n, or null
  uint32_t width, height, cells; // cells = width * height
  uint32_t seg;                  // cells of a row, column or diagonal one thread sweeps at a time
  float max_step, max_drop, clearance;
};
// 12: every player's sector map flooded from its seed; cells <= rdoom_flood_max_cells.  Dynamic LDS: a 16-bit distance and a byte
// of move bits per cell.
struct FloodArgs {
  FloodPlanes planes;
  uint16_t *dist_out;  // n x height x width
};
// 16: grids of any size flooded from a seed or towards it; cells <= rdoom_flood_grid_max_cells.  The distances live in dist_out,
// the four move bits of a cell in the top four bits of its word while the kernel runs.
struct FloodGridArgs {
  FloodPlanes planes;
  uint32_t *dist_out;  // n x height x width
  uint32_t towards;    // RDOOM_FLOOD_TOWARDS: the move relation is followed backwards
};
// 20: such grids flooded over moves to the eight neighbours.  The eight move bits of a cell live in the top byte of its word while
// the kernel runs.
struct FloodOctileArgs : FloodGridArgs {
  uint32_t axial_cost, diagonal_cost;
};

// Kernel 13: players reset at seeded random points of their level's floor (spawn.hip; include/rdoom.h "spawn" has the contract).  One
// lane per player; the sector tables are SectorDevice's, the spawn tables SpawnDevice's (world_shared.hpp).
struct SpawnArgs {
  rdoom_player_state *states;
  const float *offsets;     // n x n_objects x xyz, or null
  const uint8_t *mask;      // n, or null: every player
  const uint32_t *episode;  // n, or null: 0
  uint32_t *tries_out;      // n, or null
  const float4 *nodes, *edges, *sectors;
  const uint4 *leaves;
  const float *cumulative;
  const float4 *corners;
  uint32_t n, n_objects;
  uint32_t key0, key1;  // the seed's low and high words
  float margin, clearance, max_step;
  uint32_t flags;
};

// Kernels 14 and 15: the planes and cells of the walking distance over a whole level (goal.hip; include/rdoom.h "goal distance" has
// the contract; its flood is kernel 16 above).
// 14: a level's sector, floor and ceiling planes on its explored-area grid, one thread per cell.
struct AreaPlaneArgs {
  const float *offsets;   // n x n_objects x xyz, or null
  const uint32_t *area;   // n x 2 x stride words (reveal_area's rows), or null: every cell shows
  uint16_t *sector_out;   // each n x height x width, or null
  float *floor_out, *ceiling_out;
  const float4 *nodes, *edges, *sectors;  // SectorDevice's arrays
  const uint4 *leaves;
  uint32_t n_objects, stride, width, height, blocks;  // blocks: workgroups per row of planes
  float cell;
};
// 15: the cell of the explored-area grid every player stands in, one lane per player.
struct AreaCellArgs {
  const rdoom_player_state *states;
  int32_t *cells_out;  // n x (ix, iz)
  uint32_t n;
  float cell;
};

// Kernels 17, 18 and 21: waypoints and frontiers (path.hip; include/rdoom.h "waypoints and frontiers" and "octile distance" have the
// contracts).
// 17: a flood's field walked downhill from a start, one wavefront per row; lanes 0 .. 3 test one neighbour each.
struct DescendArgs {
  const float *floor, *ceiling;  // n x height x width each: the planes the field was flooded from
  const uint32_t *dist;          // n x height x width: rdoom_flood_grids' distances
  const int32_t *starts;         // n x (column, row)
  int32_t *cells_out;            // n x (column, row)
  uint32_t *moves_out;           // n
  int32_t *path_out;             // n x path_len x (column, row), or null
  uint32_t n, width, height, path_len;
  uint32_t max_moves, stop_dist;
  float max_step, max_drop, clearance;
};
// 21: an octile field (rdoom_flood_grids_octile's distances) walked the same way; lanes 0 .. 7 test one neighbour each.
struct DescendOctileArgs : DescendArgs {
  uint32_t axial_cost, diagonal_cost;
};
// 18: the frontier of every player's explored area, one workgroup per row; a thread takes 32 cells, a word of the bit planes, at a
// time.
struct FrontierArgs {
  const uint32_t *area;  // n x 2 x stride words (reveal_area's rows)
  const uint32_t *dist;  // n x height x width: rdoom_flood_grids' distances
  int32_t *cell_out;     // n x (ix, iz)
  uint32_t *dist_out;    // n, or null
  uint32_t *count_out;   // n, or null
  uint8_t *mask_out;     // n x height x width, or null
  uint32_t stride, width, height;
  float cell;
};

// Kernel 19: the squared distance to the nearest blocking cell, capped at a radius, and the planes with the cells near a wall made
// void (walls.hip; include/rdoom.h "wall distance" has the contract).  One workgroup per WALL_TILE_X x WALL_TILE_Y tile of one row's
// grid; static LDS for the tile and a halo of the largest radius.
constexpr uint32_t WALL_TILE_X = 64, WALL_TILE_Y = 32;
struct WallArgs {
  const float *floor, *ceiling;       // n x height x width each
  uint16_t *dist2_out;                // n x height x width, or null
  float *floor_out, *ceiling_out;     // n x height x width each, or both null
  uint32_t width, height;
  uint32_t tiles_x, tiles;            // tiles across a grid, tiles of a grid
  uint32_t radius, close_d2;          // R in cells; D2 <= close_d2 is void in the output planes
  uint32_t edge_open;                 // RDOOM_WALL_EDGE_OPEN: cells outside the grid do not block
  float clearance;
};

// Kernels 22 and 23: straight walks on the grid (line.hip; include/rdoom.h "straight walks" has the contract).
// 22: the chain of grid moves of the segment between two cell centres tested, one wavefront per line; a lane takes one crossing of
// the longer axis and the crossing of the shorter one before it.
struct WalkLinesArgs {
  const float *floor, *ceiling;  // n x height x width each: rdoom_flood_grids' planes
  const int32_t *from;           // n x (column, row)
  const int32_t *to;             // n x n_to x (column, row)
  uint8_t *clear_out;            // n x n_to
  int32_t *stop_out;             // n x n_to x (column, row), or null
  uint32_t lines, n_to;          // lines = n * n_to
  uint32_t width, height;
  float max_step, max_drop, clearance;
};
// 23: a listed path pulled straight, one wavefront per row; a lane walks the line to one candidate cell of the path.
struct StraightenArgs {
  const float *floor, *ceiling;  // n x height x width each
  const int32_t *starts;         // n x (column, row)
  const int32_t *path;           // n x path_len x (column, row)
  int32_t *corners_out;          // n x corner_len x (column, row)
  uint32_t *count_out;           // n
  float *length_out;             // n, or null
  uint32_t n, width, height, path_len, max_look, corner_len;
  float max_step, max_drop, clearance;
};

// Kernel 24: what each player sees, touches and collects of its level's things (things.hip; include/rdoom.h "things" has the
// contract).  One 256-thread workgroup per player; a thread takes one thing of a pass of 256, and the pass's candidates for sight
// go through sight.hpp's sight_limits as rays.
struct ThingSenseArgs {
  const rdoom_player_state *states;
  const float *offsets;          // n x n_objects x xyz, or null
  const rdoom_thing *things;     // the set's records, level after level
  uint32_t *collected;           // n x stride words, or null: read as they stand, then OR-ed into
  uint32_t *visible_out;         // n x stride words, or null
  uint32_t *touched_out;         // n x stride words, or null
  rdoom_thing_nearest *nearest_out;  // n x 8 records, or null
  uint32_t *new_out;             // n x 8, or null
  uint32_t n_objects, stride;
  float max_range, cos_half_fov, touch_radius, touch_below, touch_above;
  uint32_t collect_mask;
};

// Kernel 26: a level's solid things stamped into the area planes (stamp.hip; include/rdoom.h "solid things on the grid" has the
// contract).  One 256-thread workgroup per STAMP_TILE_X x STAMP_TILE_Y tile of one row's planes; a lane is a column, a thread takes
// four cells of it.
constexpr uint32_t STAMP_TILE_X = 64, STAMP_TILE_Y = 16;
struct StampArgs {
  const rdoom_thing *things;      // the set's records, level after level
  const float *offsets;           // n x n_objects x xyz, or null
  const uint32_t *solid;          // levels x stride words, or null: every thing is solid
  const uint32_t *hidden;         // n x stride words, or null: nothing is hidden
  const uint32_t *floor, *ceiling;       // n x height x width words each: the planes, read as the words they are
  uint32_t *floor_out, *ceiling_out;     // n x height x width each, or both null; the inputs themselves: in place
  int32_t *index_out;             // n x height x width, or null
  uint32_t n_objects, stride, width, height, tiles_x, tiles;  // tiles: per row of planes
  float cell, grow, below, above; // below = -block_below
};

// Kernel 27: the range sensor's rays against a level's things as vertical cylinders, after the world cast (raythings.hip;
// include/rdoom_rays.h has the contract).  One 256-thread workgroup per player; a thread takes one thing of a pass of 256, the
// things in reach go into a list in LDS, and the list is folded over the rays 64 at a time, a quarter of it per wave.
struct RayThingArgs {
  const rdoom_player_state *states;
  const float *dirs;              // n_rays x xyz, camera frame
  const float *offsets;           // n x n_objects x xyz, or null
  const rdoom_thing *things;      // the set's records, level after level
  const uint32_t *select;         // levels x stride words, or null: every thing
  const uint32_t *hidden;         // n x stride words, or null: nothing is hidden
  const float *frac_in;           // n x n_rays, or null: +inf; may be frac_out itself
  float *frac_out;                // n x n_rays
  int32_t *thing_out;             // n x n_rays, or null
  uint32_t n_rays, n_objects, stride, category_mask;
  float max_range, grow;
  float height[8];
};

// Kernels 30 to 32, rdoom_frame_things' three (the table's empty records, the reduction of an id plane with a 64-slot table in LDS
// per workgroup, the bit rows), take no handle: their arguments are the entry point's, in framethings.hip
// (include/rdoom_frame_things.h has the contract).  The thing plane they reduce is kernels 7 + 8's PLANE_THING.

}  // namespace rdoom_dev
